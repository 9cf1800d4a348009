"""GPU: whole-step attention with prefill chunks (aic_step_attention, csrc/prefill_attn.hip) against the fp32 oracle
(oracle.spec_oracle.verify_attention, which takes any q_len) at the project's bar: atol 1e-3, rtol 2^-8.
Random Q / K / V bound the accuracy of the values, not single-key masks (one key carries ~1/ctx of a row's weight): the
mask edges are pinned on planted-key fixtures in tests/test_gpu_attention_planted.py."""
import numpy as np
import pytest
import torch

from oracle import spec_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128
TOL = dict(atol=1e-3, rtol=2 ** -8)


def _ops():
    from arcticinference_amd import ops
    return ops


def _case(q_lens, ctxs, Hq, Hkv, bs, seed, q_pad=0, fp8=False):
    """Random q [T, Hq, D] (token stride Hq * D + q_pad), paged caches with a shuffled block table."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(c + bs - 1) // bs for c in ctxs]
    total = sum(nblk) + 3
    perm = torch.randperm(total, generator=g)
    bt = torch.zeros(len(ctxs), max(nblk), dtype=torch.int32)
    k = 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[k:k + n].to(torch.int32)
        k += n
    kc = torch.randn(total, bs, Hkv, D, generator=g)
    vc = torch.randn(total, bs, Hkv, D, generator=g)
    T = sum(q_lens)
    qbuf = torch.randn(T, Hq * D + q_pad, generator=g).to(torch.bfloat16)
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    ks = vs = None
    if fp8:
        ks, vs = 0.043, 0.021
        kc, vc = O.fp8_sat(kc / ks, "e4m3"), O.fp8_sat(vc / vs, "e4m3")
    else:
        kc, vc = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    return qbuf, kc, vc, bt, qsl, ks, vs


def _run(q_lens, ctxs, Hq, Hkv, bs, seed, q_pad=0, fp8=False, heads=None, out=None):
    """(got [T, Hq, D] f32, want f32): want from the oracle, on the kv heads `heads` only when given (the q heads of
    those groups, and K / V sliced to them, keep the fp32 reference small)."""
    ops = _ops()
    qbuf, kc, vc, bt, qsl, ks, vs = _case(q_lens, ctxs, Hq, Hkv, bs, seed, q_pad, fp8)
    T = sum(q_lens)
    q = qbuf.to(DEV)[:, :Hq * D].unflatten(1, (Hq, D))
    kw = {}
    if fp8:
        kw = dict(k_scale=torch.tensor([ks], device=DEV), v_scale=torch.tensor([vs], device=DEV))
    got = ops.step_attention(q, kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV),
                             torch.tensor(qsl, device=DEV), max(ctxs), D ** -0.5, q_lens_host=q_lens, out=out, **kw)
    got = got.float().cpu()
    qc = qbuf[:, :Hq * D].reshape(T, Hq, D)
    sc = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    if heads is None:
        return got, O.verify_attention(qc, kc, vc, bt, ctxs, qsl, D ** -0.5, **sc)
    G = Hq // Hkv
    outs = []
    for h in heads:
        want = O.verify_attention(qc[:, h * G:(h + 1) * G].contiguous(), kc[:, :, h:h + 1].contiguous(),
                                  vc[:, :, h:h + 1].contiguous(), bt, ctxs, qsl, D ** -0.5, **sc)
        outs.append((got[:, h * G:(h + 1) * G], want))
    return outs


def _check(got, want, what):
    err = (got - want).abs().max()
    assert torch.allclose(got, want, **TOL), f"{what}: max abs err {err}"


# q_len x context (first chunk, later chunks, a context that is not a multiple of the 32-token tile); block size, group
# size and cache dtype rotate over the cases
_QLENS = [34, 35, 64, 127, 128, 129, 500, 2048]
_BS = [16, 32, 48]
_GROUPS = [(4, 1), (16, 4), (8, 1)]      # (Hq, Hkv): G = 4, 4, 8
_SINGLE = []
for i, ql in enumerate(_QLENS):
    for j, ctx in enumerate([ql, ql + 1000, max(4096, ql), ql + 77]):
        Hq, Hkv = _GROUPS[(i + j) % 3]
        _SINGLE.append(dict(q_len=ql, ctx=ctx, bs=_BS[(i + 2 * j) % 3], Hq=Hq, Hkv=Hkv, fp8=(i + j) % 2 == 1))


@pytest.mark.parametrize("cfg", _SINGLE, ids=lambda c: f"q{c['q_len']}-c{c['ctx']}-bs{c['bs']}-G{c['Hq'] // c['Hkv']}"
                         f"-{'fp8' if c['fp8'] else 'bf16'}")
def test_single_prefill_request(cfg):
    got, want = _run([cfg["q_len"]], [cfg["ctx"]], cfg["Hq"], cfg["Hkv"], cfg["bs"], seed=cfg["q_len"] + cfg["ctx"],
                     fp8=cfg["fp8"])
    _check(got, want, cfg)


@pytest.mark.parametrize("bs", [16, 32, 48])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_block_size_group_size_and_cache_dtype(bs, G, fp8):
    got, want = _run([100, 37], [300, 37], 2 * G, 2, bs, seed=bs * 10 + G, fp8=fp8)
    _check(got, want, (bs, G, fp8))


def test_several_prefill_requests_of_different_lengths():
    q_lens, ctxs = [300, 34, 1000, 64, 129], [300, 1500, 2100, 64, 700]
    got, want = _run(q_lens, ctxs, 32, 8, 16, seed=5)
    _check(got, want, "several")


@pytest.mark.parametrize("where", ["front", "middle", "end"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_mixed_step_decodes_long_drafts_and_chunks(where, fp8):
    dec_q, dec_c = [1, 4, 33, 2, 9, 1, 17], [900, 1300, 2000, 64, 700, 5, 333]
    chunks_q, chunks_c = [256, 48], [1256, 48]
    if where == "front":
        q_lens, ctxs = chunks_q + dec_q, chunks_c + dec_c
    elif where == "middle":
        q_lens, ctxs = dec_q[:3] + chunks_q[:1] + dec_q[3:] + chunks_q[1:], dec_c[:3] + chunks_c[:1] + dec_c[3:] + chunks_c[1:]
    else:
        q_lens, ctxs = dec_q + chunks_q, dec_c + chunks_c
    got, want = _run(q_lens, ctxs, 32, 8, 16, seed=11, fp8=fp8)
    _check(got, want, where)


@pytest.mark.parametrize("q_lens,ctxs", [([200], [1200]), ([4, 200, 2], [300, 1200, 50])])
def test_strided_q(q_lens, ctxs):
    """q as a view into a wider buffer (the Ulysses receive buffer): token stride > Hq * D."""
    got, want = _run(q_lens, ctxs, 8, 2, 16, seed=3, q_pad=3 * D)
    _check(got, want, "strided")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_split_key_range_small_chunk_long_context(fp8):
    """64 query tokens at an 8192-token context on one kv head (4 workgroups): the key range is split and merged."""
    got, want = _run([64], [8192], 8, 1, 16, seed=8, fp8=fp8)
    _check(got, want, "split")


def test_unsplit_path_full_grid():
    """1024 tokens of 32 query heads over 8 kv heads: 256 workgroups, no split."""
    got, want = _run([1024], [1024], 32, 8, 16, seed=9)
    _check(got, want, "unsplit")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_llama8b_chunk_2048_at_4096_sampled_heads(fp8):
    """Full size (Llama-3.1-8B: Hq 32, Hkv 8; a 2048-token chunk ending a 4096-token prompt), checked on two kv heads."""
    for got, want in _run([2048], [4096], 32, 8, 16, seed=10, fp8=fp8, heads=[0, 5]):
        _check(got, want, "llama8b")


# ---- invariants ----------------------------------------------------------------------------------------------------
def _mixed_inputs(seed=12):
    q_lens, ctxs = [3, 600, 1, 33, 100, 5], [500, 1600, 2, 900, 100, 4000]
    qbuf, kc, vc, bt, qsl, _, _ = _case(q_lens, ctxs, 32, 8, 16, seed)
    T = sum(q_lens)
    q = qbuf.to(DEV).reshape(T, 32, D)
    args = (q, kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV),
            torch.tensor(qsl, device=DEV), max(ctxs), D ** -0.5)
    return q_lens, ctxs, args


def test_two_identical_calls_are_bit_identical():
    ops = _ops()
    q_lens, _, args = _mixed_inputs()
    a = ops.step_attention(*args, q_lens_host=q_lens)
    b = ops.step_attention(*args, q_lens_host=q_lens)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_decode_rows_match_the_decode_only_call():
    ops = _ops()
    q_lens, ctxs, args = _mixed_inputs()
    q, kc, vc, bt, sl, qsl, max_seq, scale = args
    got = ops.step_attention(*args, q_lens_host=q_lens).float()
    dec = [i for i, n in enumerate(q_lens) if n <= 33]
    starts = np.concatenate([[0], np.cumsum(q_lens)])
    rows = torch.tensor(np.concatenate([np.arange(starts[i], starts[i + 1]) for i in dec]), device=DEV)
    dq = [q_lens[i] for i in dec]
    dqsl = torch.tensor(np.concatenate([[0], np.cumsum(dq)]).astype(np.int32), device=DEV)
    want = ops.verify_attention(q[rows].contiguous(), kc, vc, bt[dec].contiguous(), sl[dec].contiguous(), dqsl, max(dq),
                                max(ctxs[i] for i in dec), scale, q_lens_host=dq).float()
    assert torch.allclose(got[rows], want, **TOL), (got[rows] - want).abs().max()


def test_poisoned_output_is_fully_overwritten():
    ops = _ops()
    q_lens, _, args = _mixed_inputs()
    out = torch.full_like(args[0], float("nan"))
    ops.step_attention(*args, q_lens_host=q_lens, out=out)
    assert not torch.isnan(out.float()).any()


def test_workspace_query_mixed_vs_parts():
    from arcticinference_amd import _native as N
    ws = N.lib().aic_step_attention_workspace_bytes
    n_dec = sum(1 + (i % 33) for i in range(63))
    assert ws(n_dec, 1, 2048, 32, 8, 128, 64) <= ws(n_dec, 0, 0, 32, 8, 128, 64) + ws(0, 1, 2048, 32, 8, 128, 64)
