"""GPU: the mask edges of the float16 attention bodies on planted-key fixtures (tests/attention_fixtures.py), once per
body.  The mask code is shared with the bf16 instantiations, but every f16 instantiation is a kernel of its own: the
short body, the long-draft body, the one-grid mixed call, the prefill body at q_len 34 and 129, a windowed head-size-64
layer with sinks, and one e4m3 cache.  The fixture's q / K / V are converted to fp16 (e4m3 caches: q only) and the fp32
oracle is put on the converted tensors; atol 1e-3, rtol 2^-8, the output pre-filled with NaN.  Every case has contexts
that end inside a page (the planted key of position seq_len sits in the stale slot behind them) and on a page border
(it sits on the spare page the padded block-table columns name)."""
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


def _fp16_case(q_lens, ctxs, Hq, Hkv, D, bs, seed, window=0, fp8=False, sinks=False):
    c = F.planted_case(q_lens, ctxs, Hq, Hkv, D, bs, seed, window=window, fp8=fp8, sinks=_sinks(Hq, seed) if sinks else None)
    c.q = c.q.to(torch.float16)
    if not fp8:
        c.kc, c.vc = c.kc.to(torch.float16), c.vc.to(torch.float16)
    assert any(x % bs == 0 for x in ctxs) and any(x % bs != 0 for x in ctxs)
    return c


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


def _check(c, got, want, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), f"{what}:\n" + F.describe(c, got, want, ATOL, RTOL)


def _verify_and_step(c, what):
    """The verify call with the host's lengths (short / long bodies) and without (generic kernel), and the step call."""
    want = F.oracle(c)
    args, kw = _dev(c)
    for host_lens in (True, False):
        out = torch.full(c.q.shape, float("nan"), dtype=torch.float16, device=DEV)
        _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out,
                                q_lens_host=c.q_lens if host_lens else None, **kw)
        _check(c, out.float().cpu(), want, (what, "host lens", host_lens))
    _step(c, what, want)


def _step(c, what, want=None):
    want = F.oracle(c) if want is None else want
    args, kw = _dev(c)
    out = torch.full(c.q.shape, float("nan"), dtype=torch.float16, device=DEV)
    _ops().step_attention(*args, max(c.ctxs), c.scale, q_lens_host=c.q_lens, out=out, **kw)
    _check(c, out.float().cpu(), want, (what, "step_attention"))


def test_short_body():
    """1 .. 8 query tokens at G = 4 (one and two row tiles), two kv heads."""
    _verify_and_step(_fp16_case([1, 4, 8, 5, 2], [333, 320, 47, 8, 2], 8, 2, 128, 16, seed=51), "short")


def test_long_draft_body():
    _verify_and_step(_fp16_case([33, 20, 9], [700, 512, 9], 8, 2, 128, 16, seed=52), "long")


def test_mixed_call():
    """Short requests and long drafts in one call: the one-grid launch."""
    _verify_and_step(_fp16_case([1, 33, 2, 12, 4], [40, 650, 336, 512, 4], 8, 2, 128, 16, seed=53), "mixed")


@pytest.mark.parametrize("q_len", [34, 129])
def test_prefill_body(q_len):
    """A first chunk (context = q_len), a later chunk ending on a page border, and a decode beside them."""
    _step(_fp16_case([q_len, q_len, 3], [q_len, q_len + 512 - q_len % 16, 77], 8, 2, 128, 16, seed=54 + q_len),
          ("prefill", q_len))


def test_windowed_head_size_64_layer_with_sinks():
    c = _fp16_case([1, 4, 33, 2, 70], [333, 320, 500, 48, 270], 16, 2, 64, 16, seed=55, window=128, sinks=True)
    _step(c, "D64 W128 sinks")
    d = _fp16_case([1, 4, 33, 2], [333, 320, 500, 48], 16, 2, 64, 16, seed=56, window=128, sinks=True)
    _verify_and_step(d, "D64 W128 sinks, decode only")


def test_e4m3_cache():
    """fp16 queries over an e4m3 cache: the tile conversion feeds every body (short, long, prefill)."""
    _verify_and_step(_fp16_case([1, 33, 2, 12, 4], [40, 650, 336, 512, 4], 8, 2, 128, 16, seed=57, fp8=True), "e4m3 decode")
    _step(_fp16_case([34, 129, 3], [34, 640, 77], 8, 2, 128, 16, seed=58, fp8=True), "e4m3 prefill")
