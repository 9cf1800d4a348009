"""GPU: the attention kernels' float16 instantiations (csrc/verify_attn.hip, csrc/prefill_attn.hip through
aic_verify_attention_dt / aic_step_attention_dt) against the fp32 oracle (oracle.spec_oracle.verify_attention, fed the
fp16 / e4m3 tensors themselves) at the project's bar, atol 1e-3, rtol 2^-8, the output buffer pre-filled with NaN.

Every case is the smallest shape that reaches one instantiation: the one- and two-row-tile short body with 4, 2 and 1 kv
heads per workgroup, the long-draft body, the one-grid short + long launch, the generic (device-geometry) kernel, head size
64 with a window and sinks, the prefill body split and unsplit, and q as a column slice of a wider buffer; each with an
fp16 cache and, at head size 128, with an e4m3 cache.  The split count is forced to 1 (the attention launch writes the
finished row: the direct epilogue) and to 3 (the combine launch writes it).

"The arithmetic is f16": V values that fp16 holds exactly and that lie 2^-8 from every bf16 value, under a single key of
weight 1, must come back within one fp16 step; e4m3 codes must come back exactly — from the verify bodies, and under equal
weights from the prefill body.  Weights below f16's normal range (2^-14 of the row maximum) must not be lost.  And the
dtype rules: a call that breaks one raises before anything is launched and leaves the NaN-filled output alone."""
import numpy as np
import pytest
import torch

import attention_fixtures as F
from oracle import spec_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = 1e-3, 2 ** -8


def _ops():
    from arcticinference_amd import ops
    return ops


def _native():
    from arcticinference_amd import _native as N
    return N


def _sinks(Hq, seed):
    return (torch.randn(Hq, generator=torch.Generator().manual_seed(seed)) * 2).float()


def _case(q_lens, ctxs, Hq, Hkv, D, bs, seed, fp8):
    """Random q / K / V in fp16 (or K / V as e4m3 codes of x / scale) behind a shuffled block table."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(c + bs - 1) // bs for c in ctxs]
    nb = sum(nblk) + 3
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(ctxs), max(nblk), dtype=torch.int32)
    p = 0
    for i, k in enumerate(nblk):
        bt[i, :k] = perm[p:p + k].to(torch.int32)
        p += k
    kc = torch.randn(nb, bs, Hkv, D, generator=g)
    vc = torch.randn(nb, bs, Hkv, D, generator=g)
    q = torch.randn(int(sum(q_lens)), Hq, D, generator=g).to(torch.float16)
    if fp8:
        kc, vc = O.fp8_sat(kc / F.K_SCALE, "e4m3"), O.fp8_sat(vc / F.V_SCALE, "e4m3")
    else:
        kc, vc = kc.to(torch.float16), vc.to(torch.float16)
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    return q, kc, vc, bt, qsl


def _want(q, kc, vc, bt, ctxs, qsl, D, fp8, window=0, sinks=None):
    sc = dict(k_scale=F.K_SCALE, v_scale=F.V_SCALE) if fp8 else {}
    return O.verify_attention(q, kc, vc, bt, ctxs, qsl, D ** -0.5, sliding_window=window, sinks=sinks, **sc)


def _kw(fp8, window, sinks):
    kw = {}
    if fp8:
        kw.update(k_scale=torch.tensor([F.K_SCALE], device=DEV), v_scale=torch.tensor([F.V_SCALE], device=DEV))
    if window:
        kw["sliding_window"] = window
    if sinks is not None:
        kw["sinks"] = sinks.to(DEV)
    return kw


def _assert_close(got, want, what):
    err = (got - want).abs()
    print(what, "max abs err", float(err.max()), "worst err / bound", float((err / (ATOL + RTOL * want.abs())).max()))
    assert torch.isfinite(got).all(), f"{what}: non-finite output (a row was not written)"
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), (what, float(err.max()))


class _forced_splits:
    """Force the split count of the short / generic launch and of the long part of a mixed call (0 = the library's
    choice); the hooks are reset whatever happens."""

    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        L = _native().lib()
        L.aic_debug_attn_layout(0, self.splits)
        L.aic_debug_attn_long_splits(self.splits)

    def __exit__(self, *exc):
        L = _native().lib()
        L.aic_debug_attn_layout(0, 0)
        L.aic_debug_attn_long_splits(0)
        return False


# ---- verify bodies ---------------------------------------------------------------------------------------------------
_VERIFY = {
    # the 40-token context is where a coarse P shows: few terms, nothing averages the weights' rounding out
    "short-1tile-hpw2": dict(Hq=8, Hkv=2, D=128, q_lens=[1, 4, 2], ctxs=[40, 200, 333], host=True),
    "short-1tile-hpw4": dict(Hq=16, Hkv=4, D=128, q_lens=[1, 4, 2], ctxs=[40, 200, 333], host=True),
    "short-2tile": dict(Hq=8, Hkv=2, D=128, q_lens=[5, 8, 1], ctxs=[300, 289, 304], host=True),
    "waves-as-ranges": dict(Hq=4, Hkv=1, D=128, q_lens=[4, 7, 1], ctxs=[200, 600, 417], host=True),
    "long-draft": dict(Hq=8, Hkv=2, D=128, q_lens=[20, 33], ctxs=[300, 700], host=True),
    "pair-launch": dict(Hq=8, Hkv=2, D=128, q_lens=[1, 33, 2, 12], ctxs=[40, 650, 333, 512], host=True),
    "generic": dict(Hq=8, Hkv=2, D=128, q_lens=[1, 4, 2], ctxs=[40, 200, 333], host=False),
    "generic-2tile-hpw4": dict(Hq=16, Hkv=4, D=128, q_lens=[8, 33, 7], ctxs=[300, 650, 40], host=False),
    "gpt-oss-window": dict(Hq=16, Hkv=2, D=64, q_lens=[1, 4, 2, 33], ctxs=[40, 200, 333, 500], host=True, window=128,
                           sinks=True),
    "gpt-oss-full": dict(Hq=16, Hkv=2, D=64, q_lens=[1, 4, 2, 33], ctxs=[40, 200, 333, 500], host=True, sinks=True),
    "gpt-oss-generic": dict(Hq=16, Hkv=2, D=64, q_lens=[1, 3, 2], ctxs=[40, 200, 333], host=False, window=128, sinks=True),
}
_VERIFY_PARAMS = [(name, fp8) for name, c in _VERIFY.items() for fp8 in (False, True) if not (fp8 and c["D"] == 64)]


@pytest.mark.parametrize("name,fp8", _VERIFY_PARAMS, ids=[f"{n}-{'e4m3' if f else 'fp16'}" for n, f in _VERIFY_PARAMS])
def test_verify_attention_fp16_matches_the_oracle(name, fp8):
    c = _VERIFY[name]
    Hq, D, q_lens, ctxs = c["Hq"], c["D"], c["q_lens"], c["ctxs"]
    window = c.get("window", 0)
    sinks = _sinks(Hq, 3) if c.get("sinks") else None
    q, kc, vc, bt, qsl = _case(q_lens, ctxs, Hq, c["Hkv"], D, 16, seed=len(name), fp8=fp8)
    want = _want(q, kc, vc, bt, ctxs, qsl, D, fp8, window, sinks)
    args = (q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV),
            torch.tensor(qsl, device=DEV), max(q_lens), max(ctxs), D ** -0.5)
    for splits in (1, 3, 0):
        with _forced_splits(splits):
            out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
            got = _ops().verify_attention(*args, out=out, q_lens_host=q_lens if c["host"] else None,
                                          **_kw(fp8, window, sinks))
            assert got.dtype == torch.float16 and got.data_ptr() == out.data_ptr()
            _assert_close(out.float().cpu(), want, (name, "e4m3" if fp8 else "fp16", "splits", splits))


@pytest.mark.parametrize("fp8", [False, True], ids=["fp16", "e4m3"])
def test_q_as_a_column_slice_of_a_wider_buffer(fp8):
    """The all-to-all receive form: q rows sit q_stride > Hq * D elements apart, what lies between them is NaN."""
    Hq, Hkv, D, q_lens, ctxs = 8, 2, 128, [1, 33, 2, 12], [40, 650, 333, 512]
    q, kc, vc, bt, qsl = _case(q_lens, ctxs, Hq, Hkv, D, 16, seed=31, fp8=fp8)
    want = _want(q, kc, vc, bt, ctxs, qsl, D, fp8)
    T = q.shape[0]
    wide = torch.full((T, Hq * D + 2 * Hkv * D), float("nan"), dtype=torch.float16, device=DEV)
    wide[:, :Hq * D] = q.to(DEV).view(T, Hq * D)
    qv = wide[:, :Hq * D].unflatten(-1, (Hq, D))
    assert qv.stride(0) == Hq * D + 2 * Hkv * D and qv.data_ptr() == wide.data_ptr()
    for host in (True, False):
        out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
        _ops().verify_attention(qv, kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV),
                                torch.tensor(qsl, device=DEV), max(q_lens), max(ctxs), D ** -0.5, out=out,
                                q_lens_host=q_lens if host else None, **_kw(fp8, 0, None))
        _assert_close(out.float().cpu(), want, ("column slice", fp8, host))


# ---- prefill chunks through step_attention ---------------------------------------------------------------------------
_STEP = {
    # contexts from q_len to q_len + 500; 333 tokens at most keep the first call's key ranges unsplit (the finished rows
    # come from the prefill launch), 629 splits them (they come from the prefill combine launch)
    "chunk-unsplit": dict(q_lens=[70, 1, 3], ctxs=[70, 200, 333]),
    "chunk-split": dict(q_lens=[70, 1, 3], ctxs=[570, 40, 333]),
    "chunk-129-and-long-draft": dict(q_lens=[129, 33], ctxs=[629, 533]),
}
_STEP_KV = {"D128-fp16": (8, 2, 128, False, 0, False), "D128-e4m3": (8, 2, 128, True, 0, False),
            "D64-W33-sinks": (16, 2, 64, False, 33, True)}


@pytest.mark.parametrize("kv", list(_STEP_KV))
@pytest.mark.parametrize("name", list(_STEP))
def test_step_attention_fp16_prefill_chunks_match_the_oracle(name, kv):
    Hq, Hkv, D, fp8, window, with_sinks = _STEP_KV[kv]
    q_lens, ctxs = _STEP[name]["q_lens"], _STEP[name]["ctxs"]
    sinks = _sinks(Hq, 5) if with_sinks else None
    q, kc, vc, bt, qsl = _case(q_lens, ctxs, Hq, Hkv, D, 16, seed=len(name) + D, fp8=fp8)
    want = _want(q, kc, vc, bt, ctxs, qsl, D, fp8, window, sinks)
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
    _ops().step_attention(q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV),
                          torch.tensor(qsl, device=DEV), max(ctxs), D ** -0.5, q_lens_host=q_lens, out=out,
                          **_kw(fp8, window, sinks))
    _assert_close(out.float().cpu(), want, (name, kv))


# ---- the arithmetic is f16, not a bf16 detour ------------------------------------------------------------------------
def _one_key(D, v_row, kc_dtype, fp8):
    """One request, q_len 1, context 1: the single key has weight 1, so the output is V's row."""
    g = torch.Generator().manual_seed(D)
    q = torch.randn(1, 1, D, generator=g).to(torch.float16)
    kc = torch.randn(1, 16, 1, D, generator=g)
    kc = O.fp8_sat(kc, "e4m3") if fp8 else kc.to(kc_dtype)
    vc = torch.zeros(1, 16, 1, D, dtype=torch.float32)
    vc[0, 0, 0] = v_row
    vc = vc.to(torch.float8_e4m3fn) if fp8 else vc.to(kc_dtype)
    assert torch.equal(vc[0, 0, 0].float(), v_row), "the planted row must be exact in the cache's type"
    bt = torch.zeros(1, 1, dtype=torch.int32)
    return q, kc, vc, bt


def _both_calls(q, kc, vc, bt, D, **kw):
    """The output row of the verify call (with and without the host's lengths) and of the step call."""
    dev = (q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor([1], dtype=torch.int32, device=DEV),
           torch.tensor([0, 1], dtype=torch.int32, device=DEV))
    rows = []
    for host in (True, False):
        out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
        _ops().verify_attention(*dev, 1, 1, D ** -0.5, out=out, q_lens_host=[1] if host else None, **kw)
        rows.append(("verify host lens" if host else "verify generic", out.float().cpu()[0, 0]))
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
    _ops().step_attention(*dev, 1, D ** -0.5, q_lens_host=[1], out=out, **kw)
    rows.append(("step", out.float().cpu()[0, 0]))
    return rows


@pytest.mark.parametrize("D", [128, 64])
def test_values_between_bf16_neighbours_survive(D):
    """V = 1 + (2 k + 1) 2^-8: odd multiples of 2^-8 in [1, 2), exact in fp16 and 2^-8 from every bf16 value (bf16 steps by
    2^-7 there).  A bf16 MFMA, tile image or output rounding anywhere on the way moves every element by 2^-8."""
    v_row = 1.0 + (2.0 * torch.arange(D, dtype=torch.float32) + 1.0) * 2.0 ** -8
    assert ((v_row.to(torch.bfloat16).float() - v_row).abs() == 2.0 ** -8).all()
    q, kc, vc, bt = _one_key(D, v_row, torch.float16, fp8=False)
    for what, row in _both_calls(q, kc, vc, bt, D):
        err = float((row - v_row).abs().max())
        print(what, "D", D, "max abs err", err)
        assert err <= 2.0 ** -10, (what, err)


def test_e4m3_codes_come_back_exactly():
    """An e4m3 cache with v_scale = 1: every finite e4m3 value of either sign, subnormals included, is an fp16 value, and
    the single key has weight 1 — the output equals the codes' values bit for bit."""
    D = 128
    codes = torch.arange(D, dtype=torch.int64)
    codes = torch.where(codes < 127, codes, torch.full_like(codes, 0x5a))      # 0x7f is NaN
    codes = codes | ((torch.arange(D) % 2) << 7)                               # alternate the sign
    v_row = codes.to(torch.uint8).view(torch.float8_e4m3fn).float()
    assert torch.isfinite(v_row).all() and torch.equal(v_row.to(torch.float16).float(), v_row)
    q, kc, vc, bt = _one_key(D, v_row, None, fp8=True)
    one = torch.ones(1, device=DEV)
    for what, row in _both_calls(q, kc, vc, bt, D, k_scale=one, v_scale=one):
        assert torch.equal(row, v_row), (what, float((row - v_row).abs().max()))


def _flat_chunk(D, v_row, fp8, q_len, ctx):
    """One prefill chunk (q_len > 33) whose keys all weigh the same: q = 0, so every score is 0 and every weight exactly 1
    whatever K holds, and every V row is `v_row` — the output of every query row is n v / n with n v exact in f32."""
    g = torch.Generator().manual_seed(D + ctx)
    nblk = (ctx + 15) // 16
    q = torch.zeros(q_len, 1, D, dtype=torch.float16)
    kc = torch.randn(nblk, 16, 1, D, generator=g)
    kc = O.fp8_sat(kc, "e4m3") if fp8 else kc.to(torch.float16)
    vc = v_row.expand(nblk, 16, 1, D).contiguous()
    vc = vc.to(torch.float8_e4m3fn) if fp8 else vc.to(torch.float16)
    assert torch.equal(vc[0, 0, 0].float(), v_row), "the planted row must be exact in the cache's type"
    bt = torch.randperm(nblk, generator=g).to(torch.int32).view(1, nblk)
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
    kw = dict(k_scale=torch.ones(1, device=DEV), v_scale=torch.ones(1, device=DEV)) if fp8 else {}
    _ops().step_attention(q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor([ctx], dtype=torch.int32, device=DEV),
                          torch.tensor([0, q_len], dtype=torch.int32, device=DEV), ctx, D ** -0.5, q_lens_host=[q_len],
                          out=out, **kw)
    return out.float().cpu()[:, 0]


# q_len 34 over its own 34 tokens: one key range, the prefill launch writes the finished rows; 129 over 629: split ranges,
# the prefill combine launch writes them
_FLAT = [(34, 34), (129, 629)]


@pytest.mark.parametrize("q_len,ctx", _FLAT)
@pytest.mark.parametrize("D", [128, 64])
def test_values_between_bf16_neighbours_survive_the_prefill_body(D, q_len, ctx):
    """The q_len 1 step call above is served by the verify bodies.  This one reaches the prefill body's MFMAs and both of
    its f16 epilogues with the same V row under equal weights (n v <= 629 * 2 in steps of 2^-8: exact in f32)."""
    v_row = 1.0 + (2.0 * torch.arange(D, dtype=torch.float32) + 1.0) * 2.0 ** -8
    rows = _flat_chunk(D, v_row, False, q_len, ctx)
    err = float((rows - v_row).abs().max())
    print("prefill D", D, "q_len", q_len, "ctx", ctx, "max abs err", err)
    assert err <= 2.0 ** -10, err


@pytest.mark.parametrize("q_len,ctx", _FLAT)
def test_e4m3_codes_come_back_exactly_from_the_prefill_body(q_len, ctx):
    """The prefill body's e4m3 -> f16 tile conversion: every finite code under equal weights, v_scale = 1 (n v has at most
    4 + 10 significant bits: exact in f32, and n v / n rounds to the f16 value v itself)."""
    D = 128
    codes = torch.arange(D, dtype=torch.int64)
    codes = torch.where(codes < 127, codes, torch.full_like(codes, 0x5a))      # 0x7f is NaN
    codes = codes | ((torch.arange(D) % 2) << 7)                               # alternate the sign
    v_row = codes.to(torch.uint8).view(torch.float8_e4m3fn).float()
    rows = _flat_chunk(D, v_row, True, q_len, ctx)
    assert torch.equal(rows, v_row.expand_as(rows)), float((rows - v_row).abs().max())


# ---- weights below f16's normal range ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form,q_len", [("verify", 1), ("verify", 33), ("step", 70)], ids=["short", "long-draft", "prefill"])
@pytest.mark.parametrize("T", [15, 20])
def test_weights_below_the_f16_normal_range_are_not_lost(form, q_len, T):
    """Key 0 scores high and has V = 0; the other keys score 0 and have V = 1, so each weighs w = 2^-T of the row's maximum:
    as an f16 P operand that is a SUBNORMAL (below 2^-14; bf16 has f32's range and no such edge).  Row i sees n_i such keys
    and the exact output is n_i w / (1 + n_i w): 0.11 at T = 15, 0.004 at T = 20 over 4096 keys — and 0 if the matrix unit
    flushed subnormal operands.  Kept, a weight is off by at most 2^-25 (half an f16 subnormal step; equal weights round the
    same way, so the errors add): 4096 * 2^-25 = 1.2e-4 on a row sum above 1, inside the project's bar, which is what is
    asserted, against the closed form in float64.  One split, so that key 0 and the light keys meet in one soft-max."""
    H, D, ctx = 4, 128, 4097
    nblk = (ctx + 15) // 16
    a = (T * np.log(2.0) * D ** 0.5) ** 0.5
    q = torch.zeros(q_len, H, D, dtype=torch.float16)
    q[:, :, 0] = a
    kc = torch.zeros(nblk, 16, H, D, dtype=torch.float16)
    kc[0, 0, :, 0] = a
    vc = torch.ones(nblk, 16, H, D, dtype=torch.float16)
    vc[0, 0] = 0
    bt = torch.arange(nblk, dtype=torch.int32).view(1, nblk)
    w = np.exp(-float(q[0, 0, 0].double() * kc[0, 0, 0, 0].double()) * D ** -0.5)
    assert 2.0 ** -(T + 0.1) < w < 2.0 ** -(T - 0.1)
    n = (np.arange(q_len) + (ctx - q_len)).astype(np.float64)
    want = torch.tensor(n * w / (1 + n * w), dtype=torch.float32).view(q_len, 1, 1).expand(q_len, H, D)
    args = (q.to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor([ctx], dtype=torch.int32, device=DEV),
            torch.tensor([0, q_len], dtype=torch.int32, device=DEV))
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device=DEV)
    with _forced_splits(1):
        if form == "step":
            _ops().step_attention(*args, ctx, D ** -0.5, q_lens_host=[q_len], out=out, num_splits_max=1)
        else:
            _ops().verify_attention(*args, q_len, ctx, D ** -0.5, out=out, q_lens_host=[q_len])
    _assert_close(out.float().cpu(), want, ("weights 2^-%d" % T, form, q_len))


# ---- argument errors: refused before any launch ----------------------------------------------------------------------
def _error_case(D, q_dtype, kv, fp8=False):
    q, kc, vc, bt, qsl = _case([2, 1], [40, 17], 8, 2, D, 16, seed=41, fp8=fp8)
    if not fp8:
        kc, vc = kc.to(kv), vc.to(kv)
    args = (q.to(q_dtype).to(DEV), kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor([40, 17], dtype=torch.int32, device=DEV),
            torch.tensor(qsl, device=DEV))
    out = torch.full(q.shape, float("nan"), dtype=q_dtype, device=DEV)
    return args, out


def _refused(args, out, exc, **kw):
    ops = _ops()
    for call in (lambda: ops.verify_attention(*args, 2, 40, 0.1, out=out, **kw),
                 lambda: ops.verify_attention(*args, 2, 40, 0.1, out=out, q_lens_host=[2, 1], **kw),
                 lambda: ops.step_attention(*args, 40, 0.1, q_lens_host=[2, 1], out=out, **kw)):
        with pytest.raises(exc) as e:
            call()
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused call wrote to the output"
    return e


def test_fp16_query_with_a_bf16_cache_is_refused():
    _refused(*_error_case(128, torch.float16, torch.bfloat16), ValueError)
    _refused(*_error_case(128, torch.bfloat16, torch.float16), ValueError)


def test_float32_query_is_refused():
    _refused(*_error_case(128, torch.float32, torch.float16), ValueError)


def test_out_of_another_dtype_is_refused():
    args, _ = _error_case(128, torch.float16, torch.float16)
    _refused(args, torch.full(args[0].shape, float("nan"), dtype=torch.bfloat16, device=DEV), ValueError)


def test_fp16_head_size_64_with_an_fp8_cache_is_unsupported_like_bf16():
    N = _native()
    one = torch.ones(1, device=DEV)
    for q_dtype in (torch.float16, torch.bfloat16):
        e = _refused(*_error_case(64, q_dtype, None, fp8=True), N.NativeError, k_scale=one, v_scale=one)
        assert e.value.code == N.AIC_ERR_UNSUPPORTED


def test_the_c_entry_points_apply_the_dtype_rules_themselves():
    """Past the Python checks: q_dtype f32, or an fp16 query with a bf16 cache (and the reverse), is AIC_ERR_UNSUPPORTED
    from both entry points, with nothing written."""
    N = _native()
    L = N.lib()
    (q, kc, vc, bt, sl, qsl), out = _error_case(128, torch.float16, torch.float16)
    ws = torch.empty(L.aic_step_attention_workspace_bytes(3, 0, 0, 8, 2, 128, 64), dtype=torch.uint8, device=DEV)
    lists = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    s = N.current_stream_ptr()
    for q_dtype, kv_dtype in ((N.DT_F32, N.DT_F16), (N.DT_F16, N.DT_BF16), (N.DT_BF16, N.DT_F16), (N.DT_F16, N.DT_FP8_E5M2),
                              (N.DT_FP8_E4M3, N.DT_FP8_E4M3)):
        rc = L.aic_verify_attention_dt(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), kv_dtype, None,
                                       None, bt.data_ptr(), bt.size(1), sl.data_ptr(), qsl.data_ptr(), 2, 3, 2, 8, 2, 128,
                                       16, 0.1, out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), 40, None, 0, None,
                                       0, 0, None, q_dtype, s)
        assert rc == N.AIC_ERR_UNSUPPORTED, (q_dtype, kv_dtype, rc)
        rc = L.aic_step_attention_dt(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), kv_dtype, None,
                                     None, bt.data_ptr(), bt.size(1), sl.data_ptr(), qsl.data_ptr(), 2, 3, 8, 2, 128, 16,
                                     0.1, out.data_ptr(), out.stride(0), ws.data_ptr(), ws.numel(), 40, lists.data_ptr(), 2,
                                     0, 0, qsl.data_ptr(), None, 0, 2, 0, 0, None, q_dtype, s)
        assert rc == N.AIC_ERR_UNSUPPORTED, (q_dtype, kv_dtype, rc)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
