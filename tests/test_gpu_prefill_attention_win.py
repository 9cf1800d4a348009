"""GPU: the prefill body on gpt-oss-class layers (aic_step_attention_win): head size 64, sliding windows and attention
sinks, against the fp32 oracle (oracle.spec_oracle.verify_attention, which defines both for any q_len) at the project's
bar, atol 1e-3, rtol 2^-8."""
import numpy as np
import pytest
import torch

from oracle import spec_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(atol=1e-3, rtol=2 ** -8)


def _ops():
    from arcticinference_amd import ops
    return ops


def _case(q_lens, ctxs, Hq, Hkv, D, bs, seed, fp8=False, v_shift=0.0):
    """Random q [T, Hq, D], paged caches with a shuffled block table (+ 3 spare pages)."""
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
    vc = torch.randn(total, bs, Hkv, D, generator=g) + v_shift
    q = torch.randn(sum(q_lens), Hq, D, generator=g).to(torch.bfloat16)
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    ks = vs = None
    if fp8:
        ks, vs = 0.043, 0.021
        kc, vc = O.fp8_sat(kc / ks, "e4m3"), O.fp8_sat(vc / vs, "e4m3")
    else:
        kc, vc = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    return q, kc, vc, bt, qsl, ks, vs


def _sinks(Hq, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Hq, generator=g) * 2 + shift).float()


def _call(c, q_lens, ctxs, window, sinks, out=None, kv=None, **extra):
    q, kc, vc, bt, qsl, ks, vs = c
    kc, vc = kv if kv is not None else (kc, vc)
    kw = dict(extra)
    if ks is not None:
        kw.update(k_scale=torch.tensor([ks], device=DEV), v_scale=torch.tensor([vs], device=DEV))
    if window is not None:
        kw["sliding_window"] = window
    if sinks is not None:
        kw["sinks"] = sinks.to(DEV)
    D = q.shape[2]
    return _ops().step_attention(q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV),
                                 torch.tensor(ctxs, dtype=torch.int32, device=DEV), torch.tensor(qsl, device=DEV),
                                 max(ctxs), D ** -0.5, q_lens_host=q_lens, out=out, **kw)


def _want(c, ctxs, window, sinks, heads=None):
    """The oracle on every kv head, or on the kv heads `heads` only (their query heads, K / V and sinks sliced)."""
    q, kc, vc, bt, qsl, ks, vs = c
    D = q.shape[2]
    sc = dict(k_scale=ks, v_scale=vs) if ks is not None else {}
    if heads is None:
        return O.verify_attention(q, kc, vc, bt, ctxs, qsl, D ** -0.5, sliding_window=window or 0, sinks=sinks, **sc)
    Hq, Hkv = q.shape[1], kc.shape[2]
    G = Hq // Hkv
    outs = []
    for h in heads:
        s = None if sinks is None else sinks[h * G:(h + 1) * G].contiguous()
        outs.append((h, O.verify_attention(q[:, h * G:(h + 1) * G].contiguous(), kc[:, :, h:h + 1].contiguous(),
                                           vc[:, :, h:h + 1].contiguous(), bt, ctxs, qsl, D ** -0.5,
                                           sliding_window=window or 0, sinks=s, **sc)))
    return outs


def _check(got, want, what):
    got = got.float().cpu()
    assert torch.allclose(got, want, **TOL), f"{what}: max abs err {float((got - want).abs().max())}"


def _run(q_lens, ctxs, Hq, Hkv, D, bs, seed, window, sinks, fp8=False, heads=None, v_shift=0.0):
    c = _case(q_lens, ctxs, Hq, Hkv, D, bs, seed, fp8, v_shift)
    got = _call(c, q_lens, ctxs, window, sinks).float().cpu()
    if heads is None:
        _check(got, _want(c, ctxs, window, sinks), (q_lens, ctxs, window, sinks is not None))
        return
    G = Hq // Hkv
    for h, want in _want(c, ctxs, window, sinks, heads):
        _check(got[:, h * G:(h + 1) * G], want, (q_lens, ctxs, window, sinks is not None, h))


# ---- gpt-oss layers ------------------------------------------------------------------------------------------------
# Hq 64 / Hkv 8 / D 64 (gpt-oss-120b on one rank) and the SP = 8 slice of it (8 query heads on 1 kv head)
@pytest.mark.parametrize("sinks", [True, False], ids=["sinks", "nosinks"])
@pytest.mark.parametrize("window", [128, 0], ids=["W128", "full"])
@pytest.mark.parametrize("heads", [(64, 8), (8, 1)], ids=["Hq64-Hkv8", "sp8-Hq8-Hkv1"])
def test_gpt_oss_layers_several_prefill_requests(heads, window, sinks):
    Hq, Hkv = heads
    bs = 16 if window else 32
    q_lens, ctxs = [300, 34, 129, 700], [1300, 34, 700, 700]
    s = _sinks(Hq, 1) if sinks else None
    _run(q_lens, ctxs, Hq, Hkv, 64, bs, seed=Hq + window, window=window, sinks=s,
         heads=[0, 7] if Hkv == 8 else None)


@pytest.mark.parametrize("bs", [16, 32])
def test_gpt_oss_chunk_2048_at_4096_sampled_heads(bs):
    """Full-size gpt-oss chunk (Hq 64 / Hkv 8 / D 64, 2048 tokens ending a 4096-token prompt) on a W = 128 layer with
    sinks, checked on two kv heads."""
    _run([2048], [4096], 64, 8, 64, bs, seed=bs, window=128, sinks=_sinks(64, 2), heads=[1, 6])


# ---- window edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 31, 32, 33])
@pytest.mark.parametrize("sinks", [True, False], ids=["sinks", "nosinks"])
def test_small_windows(window, sinks):
    """W = 1: every row sees only itself; W around the 32-token tile."""
    s = _sinks(16, 3) if sinks else None
    _run([200, 64], [900, 64], 16, 2, 64, 16, seed=window, window=window, sinks=s)


def test_window_larger_than_every_context_is_bit_identical_to_no_window():
    q_lens, ctxs = [300, 40], [1000, 900]
    c = _case(q_lens, ctxs, 16, 2, 64, 16, seed=4)
    s = _sinks(16, 4)
    a = _call(c, q_lens, ctxs, 0, s)
    b = _call(c, q_lens, ctxs, 5000, s)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("bs", [16, 32])
def test_first_window_starts_mid_page(bs):
    """ctx0 - W + 1 = 1000 - 100 - 50 + 1 = 851: inside a page and inside a 32-token tile."""
    _run([100], [1000], 8, 1, 64, bs, seed=bs + 1, window=50, sinks=_sinks(8, 5))


def test_q_len_longer_than_the_window():
    """Rows near the end of a 500-token chunk never see its start (W = 128)."""
    _run([500, 35], [600, 2000], 16, 2, 64, 16, seed=6, window=128, sinks=None)


def test_dominant_sink_over_the_split_key_range():
    """A small chunk over a long context (64 tokens at 8192 on one kv head: the key range is split and merged) with a
    sink that outweighs every key (e^12 against ~e^9.5 for the sum of the scores).  V has mean 1, so the output is
    ~0.08 of it: a sink counted once per split would shrink the output well past the tolerance."""
    _run([64], [8192], 8, 1, 64, 16, seed=7, window=0, sinks=_sinks(8, 7, shift=12.0), v_shift=1.0)


@pytest.mark.parametrize("window", [0, 128], ids=["full", "W128"])
def test_sinks_over_the_split_key_range_window(window):
    _run([64, 40], [8192, 3000], 8, 1, 64, 32, seed=8, window=window, sinks=_sinks(8, 8, shift=4.0), v_shift=1.0)


# ---- head size 128 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("window", [128, 33], ids=["W128", "W33"])
def test_head_size_128_with_window_and_sinks(fp8, window):
    _run([300, 64, 35], [1300, 64, 500], 32, 8, 128, 16, seed=9 + window, window=window, sinks=_sinks(32, 9), fp8=fp8)


# ---- mixed step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 64, 8), (128, 32, 8)], ids=["D64", "D128"])
def test_mixed_step_decodes_drafts_and_a_chunk(D, Hq, Hkv):
    """Decodes, long drafts and a chunk on a W = 128 + sinks layer: the chunk against the oracle, and the decode rows
    bit-identical to the decode part served alone by verify_attention (the compact layout the step hands it: only the
    decode rows, the prefill requests as empty ranges, the same request lists)."""
    ops = _ops()
    W = 128
    q_lens, ctxs = [1, 4, 300, 33, 2, 17], [900, 1300, 1500, 2000, 64, 333]
    c = _case(q_lens, ctxs, Hq, Hkv, D, 16, seed=12)
    q, kc, vc, bt, qsl, _, _ = c
    s = _sinks(Hq, 12)
    got = _call(c, q_lens, ctxs, W, s).float().cpu()
    want = _want(c, ctxs, W, s, heads=[0, 3])
    G = Hq // Hkv
    pf = slice(int(qsl[2]), int(qsl[3]))
    for h, w in want:
        _check(got[pf, h * G:(h + 1) * G], w[pf], ("chunk", h))
        dec_rows = np.concatenate([np.arange(qsl[i], qsl[i + 1]) for i in range(len(q_lens)) if q_lens[i] <= 33])
        _check(got[dec_rows, h * G:(h + 1) * G], w[dec_rows], ("decodes vs oracle", h))
    sp = ops.StepSplit(q_lens, G, DEV)
    rows = sp.decode_index.long()
    n_first = sp.n_short + sp.n_prefill
    split = (sp.req_lists[:n_first], n_first, sp.req_lists[n_first:], sp.n_long)
    alone = ops.verify_attention(q.to(DEV)[rows].contiguous(), kc.to(DEV), vc.to(DEV), bt.to(DEV),
                                 torch.tensor(ctxs, dtype=torch.int32, device=DEV), sp.decode_qsl, sp.max_decode_q_len,
                                 max(ctxs), D ** -0.5, req_split=split, sliding_window=W, sinks=s.to(DEV))
    got_bf = _call(c, q_lens, ctxs, W, s)
    assert torch.equal(got_bf[rows].view(torch.int16), alone.view(torch.int16))


# ---- invariants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Hq,Hkv,bs", [(64, 8, 1, 16), (64, 64, 8, 32), (128, 16, 4, 16)])
def test_pages_below_every_window_do_not_matter(D, Hq, Hkv, bs):
    """Every page that lies wholly below all rows' windows is replaced by NaN (K) and inf (V): bit-identical output."""
    W = 128
    q_lens, ctxs = [100, 300, 50], [3000, 1300, 4100]
    c = _case(q_lens, ctxs, Hq, Hkv, D, bs, seed=13)
    q, kc, vc, bt, qsl, _, _ = c
    s = _sinks(Hq, 13)
    clean = _call(c, q_lens, ctxs, W, s)
    kp, vp = kc.clone(), vc.clone()
    n = 0
    for i, (ql, ctx) in enumerate(zip(q_lens, ctxs)):
        first_seen = ctx - ql - W + 1                   # the first row's first key: no row sees anything below it
        for blk in range(first_seen // bs):
            kp[int(bt[i, blk])] = float("nan")
            vp[int(bt[i, blk])] = float("inf")
            n += 1
    assert n > 0
    poisoned = _call(c, q_lens, ctxs, W, s, kv=(kp, vp))
    assert not torch.isnan(clean.float()).any()
    assert torch.equal(clean.view(torch.int16), poisoned.view(torch.int16))


def test_defaults_and_repeat_calls_are_bit_identical():
    """sliding_window=0, sinks=None is the call without them; two identical calls agree bit for bit (D 64 and 128)."""
    for D, Hq, Hkv in [(64, 16, 2), (128, 32, 8)]:
        q_lens, ctxs = [3, 600, 1, 33, 100], [500, 1600, 2, 900, 4000]
        c = _case(q_lens, ctxs, Hq, Hkv, D, 16, seed=14)
        a = _call(c, q_lens, ctxs, None, None)
        b = _call(c, q_lens, ctxs, 0, None)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), D
        s = _sinks(Hq, 14)
        x = _call(c, q_lens, ctxs, 128, s)
        y = _call(c, q_lens, ctxs, 128, s)
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), D


def test_poisoned_output_is_fully_overwritten():
    q_lens, ctxs = [3, 600, 1, 33, 100], [500, 1600, 2, 900, 4000]
    c = _case(q_lens, ctxs, 16, 2, 64, 16, seed=15)
    out = torch.full((sum(q_lens), 16, 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    _call(c, q_lens, ctxs, 128, _sinks(16, 15), out=out)
    assert not torch.isnan(out.float()).any()


def test_fp8_cache_with_head_size_64_is_unsupported():
    from arcticinference_amd import _native as N
    c = _case([100], [200], 8, 1, 64, 16, seed=16, fp8=True)
    with pytest.raises(N.NativeError) as e:
        _call(c, [100], [200], 128, None)
    assert e.value.code == N.AIC_ERR_UNSUPPORTED
