"""GPU: the mask edges of both attention kernels (csrc/verify_attn.hip, csrc/prefill_attn.hip) on planted-key fixtures
(tests/attention_fixtures.py): every query row aims at ONE key, at its causal edge, one past it, at the window's lower
edge, one below it, or somewhere in the middle, and that key carries the row's whole weight.  A mask, a skipped tile, a
split border or a seq_len clamp that is off by one key on any row moves that row's output by order 1 (the host test
tests/test_attention_fixtures_host.py proves >= 0.1 on every concerned row); with random data the same fault sits on the
tolerance.  Against the fp32 oracle (oracle.spec_oracle.verify_attention) at the project's bar, atol 1e-3, rtol 2^-8, the
output buffer pre-filled with NaN.  Every request whose context ends inside a page carries the planted key of position
seq_len in the stale slot behind it; a context that ends on a page border finds it on the spare page the padded
block-table columns name.  Also here: the lazy running maximum of the prefill body on structured scores."""
import numpy as np
import pytest
import torch

import attention_fixtures as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = 1e-3, 2 ** -8


def _ops():
    from arcticinference_amd import ops
    return ops


def _sinks(Hq, seed):
    return (torch.randn(Hq, generator=torch.Generator().manual_seed(seed)) * 2).float()


def _dev(c):
    kw = {}
    if c.ks is not None:
        kw.update(k_scale=torch.tensor([c.ks], device=DEV), v_scale=torch.tensor([c.vs], device=DEV))
    if c.window:
        kw["sliding_window"] = c.window
    if c.sinks is not None:
        kw["sinks"] = c.sinks.to(DEV)
    args = (c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), torch.tensor(c.ctxs, dtype=torch.int32, device=DEV),
            torch.tensor(c.qsl, device=DEV))
    return args, kw


def _step(c):
    args, kw = _dev(c)
    out = torch.full(c.q.shape, float("nan"), dtype=torch.bfloat16, device=DEV)
    _ops().step_attention(*args, max(c.ctxs), c.scale, q_lens_host=c.q_lens, out=out, **kw)
    return out.float().cpu()


def _verify(c, host_lens):
    args, kw = _dev(c)
    out = torch.full(c.q.shape, float("nan"), dtype=torch.bfloat16, device=DEV)
    _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out,
                            q_lens_host=c.q_lens if host_lens else None, **kw)
    return out.float().cpu()


def _wants(c, heads=None):
    """[(sub-case, head slice, oracle)]: the whole case, or one entry per sampled kv head."""
    if heads is None:
        return [(c, slice(0, c.Hq), F.oracle(c))]
    G = c.Hq // c.Hkv
    return [(s, slice(h * G, (h + 1) * G), F.oracle(s)) for h in heads for s in [F.take_heads(c, h)]]


def _check(got, wants, what):
    for sub, sl, want in wants:
        g = got[:, sl]
        assert torch.isfinite(g).all(), f"{what}: non-finite output"
        assert torch.allclose(g, want, atol=ATOL, rtol=RTOL), f"{what} heads {sl}:\n" + F.describe(sub, g, want, ATOL, RTOL)


def _run_step(q_lens, ctxs, Hq, Hkv, D, bs, seed, window=0, fp8=False, sinks=False, heads=None, plant_below=False):
    c = F.planted_case(q_lens, ctxs, Hq, Hkv, D, bs, seed, window=window, fp8=fp8,
                       sinks=_sinks(Hq, seed) if sinks else None, plant_below=plant_below)
    _check(_step(c), _wants(c, heads), (q_lens, ctxs, Hq, Hkv, D, bs, window, fp8, sinks))
    return c


# ---- prefill body: q_len x context (first chunk, a later chunk, context 4096, a context that is not a multiple of 32) --
_QLENS = [34, 127, 128, 129, 500, 2048]
_KV = [(128, False), (128, True), (64, False)]      # (head size, fp8 cache)
_GROUPS = [(4, 1), (16, 4), (8, 1), (2, 2)]         # (Hq, Hkv): G = 4, 4, 8, 1
_SINGLE = []
for _i, _ql in enumerate(_QLENS):
    for _j, _ctx in enumerate([_ql, _ql + 1000, max(4096, _ql), _ql + 77]):
        _k = 4 * _i + _j
        _D, _fp8 = _KV[_k % 3]
        _Hq, _Hkv = _GROUPS[(_k + _k // 4) % 4]
        _SINGLE.append(dict(q_len=_ql, ctx=_ctx, D=_D, fp8=_fp8, Hq=_Hq, Hkv=_Hkv, bs=[16, 32, 48][(_k // 3 + _j) % 3],
                            window=[0, 33, 128][(_k + _k // 3) % 3], sinks=(_k // 2) % 2 == 0))


def _single_id(c):
    return (f"q{c['q_len']}-c{c['ctx']}-D{c['D']}{'fp8' if c['fp8'] else 'bf16'}-bs{c['bs']}-G{c['Hq'] // c['Hkv']}"
            f"-W{c['window']}-{'sinks' if c['sinks'] else 'nosinks'}")


def test_the_single_request_grid_covers_what_it_claims():
    for key, vals in (("bs", {16, 32, 48}), ("window", {0, 33, 128}), ("sinks", {True, False})):
        assert {c[key] for c in _SINGLE} == vals
    assert {c["Hq"] // c["Hkv"] for c in _SINGLE} == {1, 4, 8}
    assert {(c["D"], c["fp8"]) for c in _SINGLE} == set(_KV)
    for kv in _KV:           # every cache kind with every window, with and without a stale slot inside the last page
        assert {c["window"] for c in _SINGLE if (c["D"], c["fp8"]) == kv} == {0, 33, 128}
        assert {c["ctx"] % c["bs"] != 0 for c in _SINGLE if (c["D"], c["fp8"]) == kv} == {True, False}


@pytest.mark.parametrize("cfg", _SINGLE, ids=_single_id)
def test_single_prefill_request(cfg):
    _run_step([cfg["q_len"]], [cfg["ctx"]], cfg["Hq"], cfg["Hkv"], cfg["D"], cfg["bs"], seed=cfg["q_len"] + cfg["ctx"],
              window=cfg["window"], fp8=cfg["fp8"], sinks=cfg["sinks"])


@pytest.mark.parametrize("bs", [16, 32, 48])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("kv", _KV, ids=["D128bf16", "D128fp8", "D64bf16"])
@pytest.mark.parametrize("window", [0, 33, 128])
def test_block_size_group_size_cache_dtype_and_window(bs, G, kv, window):
    """Two kv heads (a mix-up of kv heads shows: their frequencies and V differ); contexts end inside a page."""
    _run_step([100, 37], [300, 37], 2 * G, 2, kv[0], bs, seed=bs + G + window, window=window, fp8=kv[1], sinks=window == 33)


def test_unsplit_path_full_grid():
    """1024 tokens of 32 query heads over 8 kv heads: 256 workgroups, no split."""
    _run_step([1024], [1024], 32, 8, 128, 16, seed=9)


@pytest.mark.parametrize("kv,window", [((128, False), 0), ((128, True), 0), ((64, False), 128), ((128, False), 33)],
                         ids=["D128bf16", "D128fp8", "D64bf16-W128", "D128bf16-W33"])
def test_split_key_range_small_chunk_long_context(kv, window):
    """64 query tokens at an 8192-token context on one kv head: the key range is split and merged; `far` rows aim into
    every split, `edge` / `past` rows at the last one's end, `win_lo` / `below` rows at the first tile of a windowed range."""
    _run_step([64], [8192], 8, 1, kv[0], 16, seed=8, window=window, fp8=kv[1], sinks=bool(window))
    _run_step([64, 40], [8189, 3000], 8, 1, kv[0], 32, seed=18, window=window, fp8=kv[1], sinks=bool(window))


@pytest.mark.parametrize("kv,window", [((128, False), 0), ((128, True), 128), ((64, False), 128), ((64, False), 0)],
                         ids=["D128bf16", "D128fp8-W128", "D64bf16-W128", "D64bf16"])
def test_several_prefill_requests_of_different_lengths(kv, window):
    q_lens, ctxs = [300, 34, 1000, 64, 129], [300, 1500, 2100, 64, 700]
    Hq = 32 if kv[0] == 128 else 64
    _run_step(q_lens, ctxs, Hq, 8, kv[0], 16, seed=5, window=window, fp8=kv[1], sinks=bool(window), heads=[0, 3, 7])


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_llama8b_chunk_2048_at_4096_sampled_heads(fp8):
    """Llama-3.1-8B (Hq 32, Hkv 8, D 128): a 2048-token chunk ending a 4096-token prompt, checked on two kv heads."""
    _run_step([2048], [4096], 32, 8, 128, 16, seed=10, fp8=fp8, heads=[0, 5])


@pytest.mark.parametrize("bs", [16, 32])
def test_gpt_oss_chunk_2048_at_4096_sampled_heads(bs):
    """gpt-oss-120b (Hq 64, Hkv 8, D 64) on a W = 128 layer with sinks, checked on two kv heads."""
    _run_step([2048], [4096], 64, 8, 64, bs, seed=bs, window=128, sinks=True, heads=[1, 6])


@pytest.mark.parametrize("D,Hq,Hkv,bs", [(64, 8, 1, 16), (64, 64, 8, 32), (128, 16, 4, 16)])
def test_lure_keys_on_every_page_below_the_window(D, Hq, Hkv, bs):
    """Every page wholly below the first row's window holds keys the first token's rows aim at (and the stale slots
    theirs): a tile taken below key_lo, or V not zeroed there, takes half of those rows' weight."""
    _run_step([100, 300, 50], [3000, 1300, 4100], Hq, Hkv, D, bs, seed=13, window=128, sinks=True,
              heads=[0, Hkv - 1] if Hkv > 1 else None, plant_below=True)


# ---- mixed step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["front", "middle", "end"])
@pytest.mark.parametrize("kv,window", [((128, False), 0), ((128, True), 0), ((64, False), 128)],
                         ids=["D128bf16", "D128fp8", "D64bf16-W128"])
def test_mixed_step_decodes_long_drafts_and_chunks(where, kv, window):
    dec_q, dec_c = [1, 4, 33, 2, 9, 1, 17], [900, 1300, 2000, 64, 700, 5, 333]
    chunks_q, chunks_c = [256, 48], [1256, 48]
    if where == "front":
        q_lens, ctxs = chunks_q + dec_q, chunks_c + dec_c
    elif where == "middle":
        q_lens, ctxs = dec_q[:3] + chunks_q[:1] + dec_q[3:] + chunks_q[1:], dec_c[:3] + chunks_c[:1] + dec_c[3:] + chunks_c[1:]
    else:
        q_lens, ctxs = dec_q + chunks_q, dec_c + chunks_c
    Hq = 32 if kv[0] == 128 else 64
    _run_step(q_lens, ctxs, Hq, 8, kv[0], 16, seed=11, window=window, fp8=kv[1], sinks=bool(window), heads=[0, 2, 7])


# ---- verify bodies ---------------------------------------------------------------------------------------------------
_VERIFY = [
    dict(Hq=32, Hkv=8, D=128, bs=16, fp8=False, window=0, sinks=False),
    dict(Hq=4, Hkv=1, D=128, bs=16, fp8=True, window=0, sinks=False),      # the SP = 8 slice: token-split waves
    dict(Hq=64, Hkv=8, D=64, bs=16, fp8=False, window=128, sinks=True),    # gpt-oss heads
    dict(Hq=16, Hkv=2, D=128, bs=32, fp8=True, window=128, sinks=True),    # G = 8
    dict(Hq=8, Hkv=8, D=64, bs=48, fp8=False, window=0, sinks=True),       # G = 1, pages of 48
]


@pytest.mark.parametrize("at_start", [False, True], ids=["ctx4096", "ctx=q_len"])
@pytest.mark.parametrize("cfg", _VERIFY, ids=lambda c: f"Hq{c['Hq']}-Hkv{c['Hkv']}-D{c['D']}{'fp8' if c['fp8'] else 'bf16'}"
                         f"-bs{c['bs']}-W{c['window']}")
def test_verify_q_len_1_to_33(cfg, at_start):
    """Requests of 1 .. 33 query tokens (shuffled) at contexts around 4096 (ending inside and on page and tile borders), or
    with no earlier context at all; with the host's query lengths (short and long bodies) and without (generic form),
    at the library's split count and at forced counts of 1 and 3."""
    from arcticinference_amd import _native as N
    rng = np.random.RandomState(cfg["Hq"] + cfg["D"])
    q_lens = [int(x) for x in rng.permutation(33) + 1]
    ctxs = list(q_lens) if at_start else [4096, 4097, 4095, 4112, 4128] + [4064 + 3 * i for i in range(28)]
    heads = None if cfg["Hkv"] <= 2 else [0, cfg["Hkv"] - 1]
    c = F.planted_case(q_lens, ctxs, cfg["Hq"], cfg["Hkv"], cfg["D"], cfg["bs"], seed=21, window=cfg["window"], fp8=cfg["fp8"],
                       sinks=_sinks(cfg["Hq"], 21) if cfg["sinks"] else None)
    wants = _wants(c, heads)
    try:
        for splits in (0, 1, 3):
            N.lib().aic_debug_attn_layout(0, splits)
            for host_lens in (True, False):
                _check(_verify(c, host_lens), wants, (cfg, at_start, "splits", splits, "host lens", host_lens))
    finally:
        N.lib().aic_debug_attn_layout(0, 0)
    _check(_step(c), wants, (cfg, at_start, "step_attention"))


# ---- lazy running maximum of the prefill body -------------------------------------------------------------------------
@pytest.mark.parametrize("profile", F.PROFILES)
@pytest.mark.parametrize("kv,window", [((128, False), 0), ((128, True), 0), ((64, False), 128)],
                         ids=["D128bf16", "D128fp8", "D64bf16-W128"])
def test_prefill_lazy_maximum_on_structured_scores(profile, kv, window):
    """The prefill body keeps a row's adopted maximum while no score exceeds it by more than 2^6 (kPfSlack) and hands
    (max, sum) per split to the combine kernel: scores that rise tile after tile, fall (the first tile's maximum stays),
    spike at isolated keys or sit on plateaus of 0.41 of the slack must give the oracle's attention, on the split path
    (64 tokens at 8192) and the unsplit one (600 tokens at 2100), alone and in one call."""
    D, fp8 = kv
    for q_lens, ctxs in (([64], [8192]), ([600], [2100]), ([600, 64, 4], [2100, 8192, 900])):
        c = F.structured_case(profile, q_lens, ctxs, 8, 2, D, 16, seed=23, fp8=fp8, window=window,
                              sinks=_sinks(8, 23) if window else None)
        got, want = _step(c), F.oracle(c)
        assert torch.isfinite(got).all(), (profile, q_lens)
        assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), (profile, kv, q_lens, float((got - want).abs().max()))
