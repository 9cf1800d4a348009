"""GPU: the shared-prefix (cascade) attention call, aic_verify_attention_prefix (csrc/prefix_attn.hip + the verify
bodies started at the prefix + the combine launch), against the fp32 oracle (oracle.spec_oracle.verify_attention) at
the project's bar, atol 1e-3, rtol 2^-8, every output buffer pre-filled with NaN.

  1. identity     shared_prefix_len = 0 through the new entry is aic_verify_attention_dt, bit for bit;
  2. the seam     the single-marked-key probe (tests/shared_prefix_fixtures.py; tests/test_shared_prefix_host.py proves
                  that a key dropped or counted twice moves every concerned row by ten times the bar at these shapes):
                  keys just below, at and just above P, one and two prefix splits, a prefix length that is no multiple of
                  the tile, pages of 48 tokens;
  3. one table    below P only prefix_block_table is read: the requests' own rows name poisoned pages there;
  4. attribution  planted-key cases (tests/attention_fixtures.py) with shared pages through every body the call can
                  launch, every cache kind, sinks, and row counts around the prefix body's 128-row block;
  5. the plugin   the patched Attention layer of the stand-in with metadata that says use_cascade."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attention_fixtures as F
import shared_prefix_fixtures as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = S.ATOL, S.RTOL


def _ops():
    from arcticinference_amd import ops
    return ops


def _native():
    from arcticinference_amd import _native as N
    return N


@pytest.fixture
def prefix_splits():
    """Forces the split count of the prefix launch; back to automatic afterwards."""
    L = _native().lib()
    try:
        yield L.aic_debug_attn_prefix_splits
    finally:
        L.aic_debug_attn_prefix_splits(0)
        L.aic_debug_attn_sequential(-1)


def _dev_args(c, bt=None):
    kw = {}
    if c.ks is not None:
        kw.update(k_scale=torch.tensor([c.ks], device=DEV), v_scale=torch.tensor([c.vs], device=DEV))
    if c.sinks is not None:
        kw["sinks"] = c.sinks.to(DEV)
    args = (c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), (c.bt if bt is None else bt).to(DEV),
            torch.tensor(c.ctxs, dtype=torch.int32, device=DEV), torch.tensor(c.qsl, device=DEV))
    return args, kw


def _run(c, shared_len, host_lens=True, bt=None, table=None):
    """ops.verify_attention with the case's shared prefix (shared_len = 0: the plain call)."""
    args, kw = _dev_args(c, bt)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    if shared_len:
        kw.update(shared_prefix_len=shared_len, prefix_block_table=(c.prefix_table if table is None else table).to(DEV),
                  seq_lens_host=c.ctxs)
    _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out,
                            q_lens_host=c.q_lens if host_lens else None, **kw)
    return out.float().cpu()


def _check(got, want, c, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), f"{what}: max abs err {float((got - want).abs().max()):.4g}\n" + (
        F.describe(c, got, want, ATOL, RTOL) if hasattr(c, "kind") else "")


# ---- 1. identity ----------------------------------------------------------------------------------------------------
def _raw(entry, c, tail):
    """The C entry itself (ops.verify_attention never calls the prefix entry for a length of 0)."""
    N, ops = _native(), _ops()
    q, kc, vc, bt = c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV)
    sl = torch.tensor(c.ctxs, dtype=torch.int32, device=DEV)
    qsl = torch.tensor(c.qsl, device=DEV)
    T, Hq, D = q.shape
    out = torch.full(q.shape, float("nan"), dtype=q.dtype, device=DEV)
    ws = torch.empty(N.lib().aic_verify_attention_workspace_bytes(T, Hq, D, 64), dtype=torch.uint8, device=DEV)
    short, n_short, long_, n_long = ops.split_requests(c.q_lens, Hq // c.Hkv, q.device)
    N.check(getattr(N.lib(), entry)(
        q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), N.torch_dtype_code(kc.dtype), None, None,
        bt.data_ptr(), bt.size(1), sl.data_ptr(), qsl.data_ptr(), len(c.ctxs), T, max(c.q_lens), Hq, c.Hkv, D, c.bs,
        float(c.scale), out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), max(c.ctxs),
        short.data_ptr() if n_short else None, n_short, long_.data_ptr() if n_long else None, n_long, 0, None,
        N.DT_BF16, *tail, N.current_stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("q_lens,ctxs", [([1, 2, 4, 3], [70, 129, 300, 33]), ([1, 4, 33, 2], [200, 90, 310, 64])],
                         ids=["short-only", "with-a-long-draft"])
def test_zero_prefix_is_the_plain_call(q_lens, ctxs):
    c = F.planted_case(q_lens, ctxs, 16, 4, 128, 16, seed=11)
    a = _raw("aic_verify_attention_dt", c, ())
    b = _raw("aic_verify_attention_prefix", c, (0, None))
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


# ---- 2. the seam ----------------------------------------------------------------------------------------------------
# (shared_prefix_len, block size, q_lens, contexts, marked keys).  Requests 1 and 3 of the first two: ctx - q_len equals
# the shared length exactly.  The first is the shape the host test proves the ten-times margin for.
_SEAMS = {
    "P64-bs16": (64, 16, [1, 2, 5, 28], [70, 66, 90, 92], [0, 31, 32, 63, 64, 95]),
    "len48-served-as-32": (48, 16, [1, 2, 5, 28], [70, 50, 90, 76], [0, 31, 32, 47, 48, 63]),
    "P96-bs48": (96, 48, [1, 2, 5, 28], [100, 98, 130, 124], [0, 31, 32, 95, 96, 127]),
}


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("seam", list(_SEAMS))
def test_marked_key_at_the_seam(seam, splits, prefix_splits):
    shared_len, bs, q_lens, ctxs, keys = _SEAMS[seam]
    assert any(c - q == shared_len for q, c in zip(q_lens, ctxs))
    prefix_splits(splits)
    for t in keys:
        c = S.marked_key_case(t, q_lens, ctxs, Hq=8, Hkv=2, D=128, bs=bs, shared_len=shared_len, seed=t)
        got = _run(c, shared_len)
        err = (got - c.expected).abs()
        bad = (err > S.bar(c.expected)).any(-1).any(-1)
        assert torch.isfinite(got).all() and not bad.any(), (
            f"marked key {t}, {splits} prefix split(s): rows at positions {c.pos[bad].tolist()} are off by up to "
            f"{float(err.max()):.4g} (expected 1 / (p + 1))")
        assert torch.allclose(got, F.oracle(c), atol=ATOL, rtol=RTOL)


# ---- 3. one table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["bf16", "f16"])
def test_below_the_prefix_only_the_prefix_table_is_read(fp16):
    P, bs = 64, 16
    c = S.share_prefix(F.planted_case([1, 3, 12, 2], [80, 67, 130, 97], 16, 4, 128, bs, seed=21), P)
    if fp16:
        c.q, c.kc, c.vc = c.q.to(torch.float16), c.kc.to(torch.float16), c.vc.to(torch.float16)
    want = F.oracle(c)                                   # on the clean shared table
    n = P // bs
    first = c.kc.shape[0]
    poison = torch.full((n,) + tuple(c.kc.shape[1:]), 3e4, dtype=c.kc.dtype)
    c.kc, c.vc = torch.cat([c.kc, poison]), torch.cat([c.vc, poison])
    bt = c.bt.clone()
    bt[1:, :n] = torch.arange(first, first + n, dtype=torch.int32)
    _check(_run(c, P, bt=bt), want, c, "poisoned own pages below P")
    # the poison is live: the plain call on the same rows reads it
    plain = _run(c, 0, bt=bt)
    assert not torch.allclose(torch.nan_to_num(plain[1:], nan=1e9), want[1:], atol=0.1, rtol=0.1)


# ---- 4. attribution -------------------------------------------------------------------------------------------------
def _cfg(name, q_lens, extra, Hq, Hkv, P, D=128, bs=16, fp8=False, f16=False, sinks=False, host_lens=True, sequential=None):
    return pytest.param(dict(q_lens=q_lens, extra=extra, Hq=Hq, Hkv=Hkv, P=P, D=D, bs=bs, fp8=fp8, f16=f16, sinks=sinks,
                             host_lens=host_lens, sequential=sequential), id=name)


# `extra`: context tokens between the prefix and the request's first query token (0: ctx - q_len == P exactly)
_CONFIGS = [
    # short body, one row tile (<= 16 rows per request); T G = 40
    _cfg("short-one-tile-16x4-bf16-P32", [1, 2, 3, 4], [0, 5, 40, 70], 16, 4, 32),
    # short body, two row tiles (32 rows per request); T G = 128 exactly, fp8 cache, two prefix splits
    _cfg("short-two-tile-16x4-fp8-P256-TG128", [8, 8, 8, 8], [0, 1, 33, 90], 16, 4, 256, fp8=True, bs=32),
    # waves as token ranges: one kv head (G = 4 and G = 8), two kv heads (G = 1)
    _cfg("ranges-4x1-bf16-P256", [1, 4, 8, 3], [3, 0, 64, 31], 4, 1, 256),
    _cfg("ranges-8x1-fp8-P32-TG128", [4, 4, 4, 4], [0, 17, 32, 100], 8, 1, 32, fp8=True),
    _cfg("ranges-2x2-D64-P256-TG129", [32, 32, 32, 32, 1], [0, 2, 40, 77, 5], 2, 2, 256, D=64, bs=32),
    # long-draft launch alone (every request over 32 rows)
    _cfg("long-only-32x8-bf16-P32", [9, 20], [0, 50], 32, 8, 32),
    _cfg("long-only-2x2-D64-P32-TG132", [33, 33, 33, 33], [0, 1, 30, 64], 2, 2, 32, D=64),
    # short requests + long drafts in one call, bf16, fp8 and f16 (with a prefix such a call goes out as two launches: the
    # one-grid kernel has no prefix-carrying copy); T G = 160
    _cfg("mixed-32x8-bf16-P256-TG160", [1, 4, 2, 33], [7, 0, 90, 12], 32, 8, 256),
    _cfg("mixed-16x4-fp8-P32", [1, 9, 3], [0, 20, 66], 16, 4, 32, fp8=True),
    _cfg("mixed-16x4-f16-P256", [1, 3, 9], [0, 20, 66], 16, 4, 256, f16=True, bs=32),
    # the same mix with the two-launch form forced, as tools do
    _cfg("two-launches-32x8-fp8-P256", [1, 4, 2, 33], [7, 0, 90, 12], 32, 8, 256, fp8=True, sequential=1),
    # head size 64 mixed: the long part beside the short one on the side stream
    _cfg("side-stream-8x1-D64-P32", [1, 10, 2], [0, 9, 70], 8, 1, 32, D=64),
    # sinks: the start of the first SUFFIX partial, counted once
    _cfg("sinks-16x4-bf16-P256", [2, 5, 12], [0, 3, 60], 16, 4, 256, sinks=True),
    _cfg("sinks-16x4-D64-P32", [1, 2, 3], [0, 3, 60], 16, 4, 32, D=64, sinks=True),
    # query lengths unknown on the host: the generic launch
    _cfg("generic-16x4-bf16-P32", [1, 3, 2], [0, 40, 3], 16, 4, 32, host_lens=False),
    _cfg("generic-4x1-f16-P256", [2, 7], [0, 40], 4, 1, 256, f16=True, host_lens=False),
]


def test_the_configurations_cover_what_they_claim():
    cs = [p.values[0] for p in _CONFIGS]
    assert {(c["Hq"], c["Hkv"]) for c in cs} == {(4, 1), (16, 4), (8, 1), (2, 2), (32, 8)}
    assert {(c["D"], c["fp8"], c["f16"]) for c in cs} >= {(128, False, False), (128, True, False), (64, False, False),
                                                          (128, False, True)}
    assert {c["P"] for c in cs} == {32, 256} and any(c["sinks"] for c in cs)
    tg = [sum(c["q_lens"]) * c["Hq"] // c["Hkv"] for c in cs]
    assert any(x < 128 for x in tg) and 128 in tg and any(x > 128 and x % 128 <= 4 for x in tg)
    for c in cs:
        assert 0 in c["extra"] and c["P"] % c["bs"] == 0        # a request whose first query token sits right at P


@pytest.mark.parametrize("cfg", _CONFIGS)
def test_shared_planted_case_meets_the_oracle(cfg, prefix_splits):
    ctxs = [cfg["P"] + e + q for q, e in zip(cfg["q_lens"], cfg["extra"])]
    seed = sum(ctxs) + cfg["Hq"]
    sinks = (torch.randn(cfg["Hq"], generator=torch.Generator().manual_seed(seed)) * 2).float() if cfg["sinks"] else None
    c = F.planted_case(cfg["q_lens"], ctxs, cfg["Hq"], cfg["Hkv"], cfg["D"], cfg["bs"], seed, fp8=cfg["fp8"], sinks=sinks)
    c = S.share_prefix(c, cfg["P"])
    if cfg["f16"]:
        c.q, c.kc, c.vc = c.q.to(torch.float16), c.kc.to(torch.float16), c.vc.to(torch.float16)
    if cfg["sequential"] is not None:
        _native().lib().aic_debug_attn_sequential(cfg["sequential"])
    want = F.oracle(c)
    _check(_run(c, cfg["P"], host_lens=cfg["host_lens"]), want, c, "automatic prefix splits")
    if cfg["P"] >= 256:
        prefix_splits(3)             # 8 tiles in 3 + 3 + 2
        _check(_run(c, cfg["P"], host_lens=cfg["host_lens"]), want, c, "three prefix splits")


# ---- 5. the plugin --------------------------------------------------------------------------------------------------
ENV = "ARCTIC_INFERENCE_HIP_SHARED_PREFIX"
_layer_no = [0]


def _plugin_layers():
    """Loads the plugin over the stand-in once and returns call(case, window=None, cascade=True): the patched Attention
    layer on metadata of the test's own (the stand-in's carries no cascade fields), K/V already in the cache — what
    _arctic_verify returns."""
    import vllm_harness as H
    from test_vllm_plugin_gpu import _vllm_config
    H.load_plugin()
    from vllm.attention.layer import Attention
    from vllm.config import set_current_vllm_config
    from vllm.forward_context import set_forward_context
    from arcticinference_amd.vllm_plugin import step_context
    cfg = _vllm_config()
    H.init_single_process_groups(cfg)
    set_current_vllm_config(cfg)

    def call(c, window=None, cascade=True):
        _layer_no[0] += 1
        layer = Attention(c.Hq, c.D, c.scale, num_kv_heads=c.Hkv, prefix=f"probe.{_layer_no[0]}.attn",
                          per_layer_sliding_window=window)
        layer.kv_cache = [torch.stack([c.kc, c.vc]).to(DEV)]
        T = int(c.qsl[-1])
        meta = SimpleNamespace(num_actual_tokens=T, max_query_len=max(c.q_lens), max_seq_len=max(c.ctxs),
                               query_start_loc=torch.tensor(c.qsl, device=DEV),
                               seq_lens=torch.tensor(c.ctxs, dtype=torch.int32, device=DEV), block_table=c.bt.to(DEV),
                               slot_mapping=None)
        if cascade:
            meta.use_cascade, meta.common_prefix_len = True, c.shared_len
        step_context.publish(np.asarray(c.q_lens), False)          # reads the switch, as the runner does once per step
        try:
            with set_forward_context(meta, cfg):
                out = layer._arctic_verify(c.q.to(DEV).view(T, c.Hq * c.D), None, None)
        finally:
            step_context.clear()
        torch.cuda.synchronize()
        assert out is not None, "the layer left the call to the backend"
        return out[:T].view(T, c.Hq, c.D).float().cpu()

    return call


def test_plugin_takes_the_prefix_path_only_when_told(stub_vllm, monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic, step_context
    # the shipped thresholds are measured break-evens (2048 tokens, 256 requests x kv heads); the route itself is tested
    # at the floor
    monkeypatch.setattr(runner_logic, "SHARED_PREFIX_MIN_LEN", 32)
    monkeypatch.setattr(runner_logic, "SHARED_PREFIX_MIN_ITEMS", 1)
    c = S.share_prefix(F.planted_case([1, 3, 4, 2], [80, 67, 130, 97], 8, 4, 128, 16, seed=31), 64)
    want = F.oracle(c)
    calls = step_context.calls
    _layer_call = _plugin_layers()
    # switch off: the plain call
    monkeypatch.delenv(ENV, raising=False)
    n0, v0 = calls["shared_prefix"], calls["verify"]
    off = _layer_call(c)
    assert calls["shared_prefix"] == n0 and calls["verify"] == v0 + 1
    _check(off, want, c, "switch off")
    assert torch.equal(off, _run(c, 0))
    # switch on: the prefix path, same answer
    monkeypatch.setenv(ENV, "1")
    on = _layer_call(c)
    assert calls["shared_prefix"] == n0 + 1 and calls["verify"] == v0 + 2
    _check(on, want, c, "switch on")
    # metadata that does not say so (the stand-in's own), and a windowed layer: the counter stays, the output is the plain call's
    plain = _layer_call(c, cascade=False)
    assert calls["shared_prefix"] == n0 + 1 and torch.equal(plain, off)
    c.window = 48
    windowed = _layer_call(c, window=48)
    assert calls["shared_prefix"] == n0 + 1 and calls["verify"] == v0 + 4
    _check(windowed, F.oracle(c), c, "windowed layer")
    c.window = 0
    assert torch.equal(windowed, _run_window(c, 48))


def _run_window(c, window):
    args, kw = _dev_args(c)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out, q_lens_host=c.q_lens,
                            sliding_window=window, **kw)
    return out.float().cpu()
