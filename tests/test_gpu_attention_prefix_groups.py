"""GPU: the grouped shared-prefix attention call, aic_verify_attention_prefix_groups (the grouped prefix body of
csrc/prefix_attn.hip + the verify bodies started at each request's own prefix + the combine launch), against the fp32
oracle (oracle.spec_oracle.verify_attention) at the project's bar, atol 1e-3, rtol 2^-8, every output buffer pre-filled
with NaN.

  1. identity     n_groups = 0 through the new entry is aic_verify_attention_dt, bit for bit; one group that holds every
                  request meets the oracle and agrees with aic_verify_attention_prefix;
  2. attribution  planted-key cases (tests/attention_fixtures.py) with pages shared per group: interleaved members, a
                  request in no group that is shorter than every prefix, a second row block, a length that is no multiple
                  of the tile, every cache kind, sinks, long drafts — automatic and three forced prefix splits;
  3. the seam     the marked-key probe (tests/prefix_group_fixtures.py; tests/test_prefix_groups_host.py proves that a key
                  dropped or counted twice moves every concerned row by ten times the bar at these shapes) at P_g - 1 and
                  P_g of every group, one and two suffix splits, one and three prefix splits;
  4. one table    below a group's prefix only its leader's block-table row is read: the members' own name poison there;
  5. stale slots  a call whose rows are all grouped, then one on the same workspace with requests in no group and a short
                  group: what the first call left in the prefix slots is not merged;
  6. the plugin   the patched Attention layer of the stand-in on a step published with its host block table."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attention_fixtures as F
import prefix_group_fixtures as PG
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
def knobs():
    """The library's debug knobs (prefix splits, suffix layout, launch form); back to automatic afterwards."""
    L = _native().lib()
    try:
        yield L
    finally:
        L.aic_debug_attn_prefix_splits(0)
        L.aic_debug_attn_layout(0, 0)
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


def _run(c, req_group=None, group_len=None, host_lens=True, bt=None, dev=None):
    """ops.verify_attention with the given groups (None: the plain call).  `dev`: (args, kw) already on the device."""
    args, kw = dev if dev is not None else _dev_args(c, bt)
    kw = dict(kw)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    if req_group is not None:
        kw.update(prefix_groups=_ops().PrefixGroups(req_group, group_len, c.q_lens, torch.device(DEV)), seq_lens_host=c.ctxs)
    _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out,
                            q_lens_host=c.q_lens if host_lens else None, **kw)
    return out.float().cpu()


def _check(got, want, c, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), f"{what}: max abs err {float((got - want).abs().max()):.4g}\n" + (
        F.describe(c, got, want, ATOL, RTOL) if hasattr(c, "kind") else "")


# ---- 1. identity ----------------------------------------------------------------------------------------------------
def _raw(entry, c, tail):
    """The C entry itself."""
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
def test_no_groups_is_the_plain_call(q_lens, ctxs):
    c = F.planted_case(q_lens, ctxs, 16, 4, 128, 16, seed=11)
    a = _raw("aic_verify_attention_dt", c, ())
    b = _raw("aic_verify_attention_prefix_groups", c, (0, None, None, None, None, None))
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_one_group_of_everybody_is_the_single_prefix_call():
    c = S.share_prefix(F.planted_case([1, 3, 9, 2], [80, 67, 130, 97], 16, 4, 128, 16, seed=21), 64)
    want = F.oracle(c)
    grouped = _run(c, [0, 0, 0, 0], [64])
    _check(grouped, want, c, "one group")
    args, kw = _dev_args(c)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out, q_lens_host=c.q_lens, shared_prefix_len=64,
                            prefix_block_table=c.prefix_table.to(DEV), seq_lens_host=c.ctxs, **kw)
    single = out.float().cpu()
    assert torch.allclose(grouped, single, atol=ATOL, rtol=RTOL)


# ---- 2. attribution -------------------------------------------------------------------------------------------------
def _cfg(name, q_lens, req_group, group_len, extra, Hq=16, Hkv=4, D=128, bs=16, fp8=False, f16=False, sinks=False,
         host_lens=True):
    return pytest.param(dict(q_lens=q_lens, req_group=req_group, group_len=group_len, extra=extra, Hq=Hq, Hkv=Hkv, D=D, bs=bs,
                             fp8=fp8, f16=f16, sinks=sinks, host_lens=host_lens), id=name)


# `extra`: for a member, context tokens between its group's length and its first query token (0: ctx - q_len equals the
# length exactly); for a request in no group, its context before the query tokens
_CONFIGS = [
    # groups A (32) and B (96) interleaved A B - A B A, the loner's context is 20: shorter than either prefix; the 9-token
    # draft is 36 rows, so the call takes the two-launch long form
    _cfg("two-groups-and-a-loner", [1, 4, 2, 3, 9, 1], [0, 1, -1, 0, 1, 0], [32, 96], [0, 5, 18, 40, 0, 70]),
    # 5 requests x 7 tokens x G 4 = 140 rows: two row blocks, the second nearly empty; beside a group of 8 rows
    _cfg("140-rows-beside-8", [7, 1, 7, 7, 1, 7, 7], [0, 1, 0, 0, 1, 0, 0], [64, 32], [0, 3, 9, 33, 0, 2, 60]),
    # a length of 70 is served as 64; request 0's first query token sits exactly at 70
    _cfg("length-70-served-as-64", [2, 3, 1, 2], [0, 0, -1, 0], [70], [0, 30, 49, 7]),
    _cfg("fp8-pages-of-32", [1, 4, 2, 3, 9, 1], [0, 1, -1, 0, 1, 0], [64, 96], [0, 5, 18, 40, 0, 70], fp8=True, bs=32),
    _cfg("D64-8x1", [1, 4, 2, 3, 5, 1], [0, 1, -1, 0, 1, 0], [32, 96], [0, 5, 18, 40, 0, 70], Hq=8, Hkv=1, D=64),
    _cfg("f16", [1, 4, 2, 3, 9, 1], [0, 1, -1, 0, 1, 0], [32, 96], [0, 5, 18, 40, 0, 70], f16=True),
    _cfg("sinks", [1, 4, 2, 3, 9, 1], [0, 1, -1, 0, 1, 0], [32, 96], [0, 5, 18, 40, 0, 70], sinks=True),
    # query lengths given to PrefixGroups but not to verify_attention: the generic launch
    _cfg("generic-launch", [1, 4, 2, 3, 2, 1], [0, 1, -1, 0, 1, 0], [32, 96], [0, 5, 18, 40, 0, 70], host_lens=False),
    _cfg("32x8-with-a-33-token-draft", [1, 33, 2, 3], [0, 0, -1, 1], [96, 32], [0, 4, 18, 0], Hq=32, Hkv=8),
]


@pytest.mark.parametrize("cfg", _CONFIGS)
def test_grouped_planted_case_meets_the_oracle(cfg, knobs):
    ctxs = [(cfg["group_len"][g] if g >= 0 else 0) + e + q for q, e, g in zip(cfg["q_lens"], cfg["extra"], cfg["req_group"])]
    seed = sum(ctxs) + cfg["Hq"]
    sinks = (torch.randn(cfg["Hq"], generator=torch.Generator().manual_seed(seed)) * 2).float() if cfg["sinks"] else None
    c = F.planted_case(cfg["q_lens"], ctxs, cfg["Hq"], cfg["Hkv"], cfg["D"], cfg["bs"], seed, fp8=cfg["fp8"], sinks=sinks)
    c = PG.share_in_groups(c, cfg["req_group"], cfg["group_len"])
    if cfg["f16"]:
        c.q, c.kc, c.vc = c.q.to(torch.float16), c.kc.to(torch.float16), c.vc.to(torch.float16)
    want = F.oracle(c)
    dev = _dev_args(c)
    _check(_run(c, c.req_group, c.group_len, host_lens=cfg["host_lens"], dev=dev), want, c, "automatic prefix splits")
    knobs.aic_debug_attn_prefix_splits(3)
    _check(_run(c, c.req_group, c.group_len, host_lens=cfg["host_lens"], dev=dev), want, c, "three prefix splits")


# ---- 3. the seam ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix_splits", [1, 3])
@pytest.mark.parametrize("suffix_splits", [1, 2])
def test_marked_key_at_every_groups_seam(suffix_splits, prefix_splits, knobs):
    knobs.aic_debug_attn_prefix_splits(prefix_splits)
    knobs.aic_debug_attn_layout(0, suffix_splits)
    for t in PG.SEAM_KEYS:
        c = PG.grouped_marked_case(t, PG.SEAM_Q_LENS, PG.SEAM_CTXS, Hq=8, Hkv=2, D=128, bs=16, req_group=PG.SEAM_REQ_GROUP,
                                   group_len=PG.SEAM_GROUP_LEN, seed=t)
        got = _run(c, c.req_group, c.group_len)
        err = (got - c.expected).abs()
        bad = (err > S.bar(c.expected)).any(-1).any(-1)
        assert torch.isfinite(got).all() and not bad.any(), (
            f"marked key {t}, {prefix_splits} prefix / {suffix_splits} suffix split(s): rows at positions "
            f"{c.pos[bad].tolist()} are off by up to {float(err.max()):.4g} (expected 1 / (p + 1))")
        assert torch.allclose(got, F.oracle(c), atol=ATOL, rtol=RTOL)


# ---- 4. one table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "f16", "fp8"])
def test_below_a_groups_prefix_only_the_leaders_row_is_read(kind):
    bs = 32 if kind == "fp8" else 16
    req_group, group_len = [0, 1, -1, 0, 1, 0], [64, 96]
    q_lens, ctxs = [1, 3, 2, 12, 2, 4], [80, 110, 20, 130, 99, 97]
    c = PG.share_in_groups(F.planted_case(q_lens, ctxs, 16, 4, 128, bs, seed=21, fp8=kind == "fp8"), req_group, group_len)
    if kind == "f16":
        c.q, c.kc, c.vc = c.q.to(torch.float16), c.kc.to(torch.float16), c.vc.to(torch.float16)
    want = F.oracle(c)                                   # on the clean shared table
    first = c.kc.shape[0]
    n_max = max(group_len) // bs
    if kind == "fp8":
        poison = torch.full((n_max,) + tuple(c.kc.shape[1:]), 0x7f, dtype=torch.uint8).view(c.kc.dtype)
    else:
        poison = torch.full((n_max,) + tuple(c.kc.shape[1:]), float("nan"), dtype=c.kc.dtype)
    c.kc, c.vc = torch.cat([c.kc, poison]), torch.cat([c.vc, poison])
    bt = c.bt.clone()
    for i, g in enumerate(req_group):
        if g >= 0 and c.leader[g] != i:
            n = group_len[g] // bs
            bt[i, :n] = torch.arange(first, first + n, dtype=torch.int32)
    _check(_run(c, req_group, group_len, bt=bt), want, c, "poisoned own pages below the group's prefix")
    # the poison is live: the plain call on the same rows reads it
    plain = _run(c, bt=bt)
    members = torch.cat([torch.full((q,), float(g >= 0 and c.leader[g] != i)) for i, (q, g) in enumerate(zip(q_lens, req_group))]) > 0
    assert not torch.allclose(torch.nan_to_num(plain[members], nan=1e9), want[members], atol=0.1, rtol=0.1)


# ---- 5. stale slots -------------------------------------------------------------------------------------------------
def test_prefix_slots_of_an_earlier_call_are_not_merged(knobs):
    q_lens, ctxs = [1, 4, 2, 3, 2, 1], [300, 290, 280, 310, 270, 300]
    c = PG.share_in_groups(F.planted_case(q_lens, ctxs, 16, 4, 128, 16, seed=41), [0, 0, 0, 1, 1, 1], [256, 256])
    want = F.oracle(c)
    dev = _dev_args(c)
    knobs.aic_debug_attn_prefix_splits(8)
    # every request grouped, eight live prefix partials per row
    _check(_run(c, [0, 0, 0, 1, 1, 1], [256, 256], dev=dev), want, c, "every request grouped")
    # the same tensors and workspace: half the requests in no group, one group of one tile — seven of its eight prefix
    # slots and all eight of the ungrouped rows must read as empty, not as what the call above left there
    second = _run(c, [0, 0, -1, 1, -1, -1], [256, 32], dev=dev)
    _check(second, want, c, "half ungrouped, one short group")
    assert torch.equal(second, _run(c, [0, 0, -1, 1, -1, -1], [256, 32], dev=dev))
    # and back
    _check(_run(c, [0, 0, 0, 1, 1, 1], [256, 256], dev=dev), want, c, "every request grouped again")


# ---- 6. the plugin --------------------------------------------------------------------------------------------------
ENV, ENV_SINGLE = "ARCTIC_INFERENCE_HIP_PREFIX_GROUPS", "ARCTIC_INFERENCE_HIP_SHARED_PREFIX"
_layer_no = [0]


def _plugin_layers():
    """Loads the plugin over the stand-in once and returns call(case, window=None, cascade=False): the patched Attention
    layer on metadata of the test's own, the step published as the runner does with the groups switch on (host block
    table, computed tokens, block size), K/V already in the cache — what _arctic_verify returns."""
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

    def call(c, window=None, cascade=False):
        _layer_no[0] += 1
        layer = Attention(c.Hq, c.D, c.scale, num_kv_heads=c.Hkv, prefix=f"groups.{_layer_no[0]}.attn",
                          per_layer_sliding_window=window)
        layer.kv_cache = [torch.stack([c.kc, c.vc]).to(DEV)]
        T = int(c.qsl[-1])
        meta = SimpleNamespace(num_actual_tokens=T, max_query_len=max(c.q_lens), max_seq_len=max(c.ctxs),
                               query_start_loc=torch.tensor(c.qsl, device=DEV),
                               seq_lens=torch.tensor(c.ctxs, dtype=torch.int32, device=DEV), block_table=c.bt.to(DEV),
                               slot_mapping=None)
        if cascade:
            meta.use_cascade, meta.common_prefix_len = True, c.shared_len
        computed = np.asarray(c.ctxs) - np.asarray(c.q_lens)
        step_context.publish(np.asarray(c.q_lens), False, block_table=c.bt.numpy(), num_computed=computed, block_size=c.bs)
        try:
            with set_forward_context(meta, cfg):
                out = layer._arctic_verify(c.q.to(DEV).view(T, c.Hq * c.D), None, None)
        finally:
            step_context.clear()
        torch.cuda.synchronize()
        assert out is not None, "the layer left the call to the backend"
        return out[:T].view(T, c.Hq, c.D).float().cpu()

    return call


def test_plugin_takes_the_grouped_path_only_when_told(stub_vllm, monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic, step_context
    # the shipped thresholds are measured break-evens; the route itself is tested at the floor
    for name, value in (("SHARED_PREFIX_MIN_LEN", 32), ("SHARED_PREFIX_MIN_ITEMS", 1), ("PREFIX_GROUPS_MIN_MEMBERS", 2)):
        monkeypatch.setattr(runner_logic, name, value)
    req_group, group_len = [0, 1, -1, 0, 1, 0], [64, 96]
    c = PG.share_in_groups(F.planted_case([1, 3, 2, 4, 2, 1], [80, 110, 20, 130, 99, 97], 8, 4, 128, 16, seed=31), req_group,
                           group_len)
    want = F.oracle(c)
    found = runner_logic.prefix_groups(c.bt.numpy(), np.asarray(c.ctxs) - np.asarray(c.q_lens), c.q_lens, 16, 4, False)
    assert found is not None and found[0].tolist() == req_group and found[1] == group_len
    calls = step_context.calls
    _layer_call = _plugin_layers()
    monkeypatch.delenv(ENV_SINGLE, raising=False)
    # switch off: the plain call
    monkeypatch.delenv(ENV, raising=False)
    n0, s0, v0 = calls["prefix_groups"], calls["shared_prefix"], calls["verify"]
    off = _layer_call(c)
    assert calls["prefix_groups"] == n0 and calls["verify"] == v0 + 1
    _check(off, want, c, "switch off")
    assert torch.equal(off, _run(c))
    # switch on: the grouped path, same answer
    monkeypatch.setenv(ENV, "1")
    on = _layer_call(c)
    assert calls["prefix_groups"] == n0 + 1 and calls["verify"] == v0 + 2 and calls["shared_prefix"] == s0
    _check(on, want, c, "switch on")
    # a windowed layer: the plain call
    c.window = 48
    windowed = _layer_call(c, window=48)
    assert calls["prefix_groups"] == n0 + 1 and calls["verify"] == v0 + 3
    _check(windowed, F.oracle(c), c, "windowed layer")
    c.window = 0
    # metadata that says use_cascade, with that switch on: the single-prefix path keeps precedence
    monkeypatch.setenv(ENV_SINGLE, "1")
    every = S.share_prefix(F.planted_case([1, 3, 4, 2], [80, 67, 130, 97], 8, 4, 128, 16, seed=31), 64)
    got = _layer_call(every, cascade=True)
    assert calls["shared_prefix"] == s0 + 1 and calls["prefix_groups"] == n0 + 1 and calls["verify"] == v0 + 4
    _check(got, F.oracle(every), every, "use_cascade")
    # ... and without it the same step is one group
    got = _layer_call(every, cascade=False)
    assert calls["shared_prefix"] == s0 + 1 and calls["prefix_groups"] == n0 + 2
    _check(got, F.oracle(every), every, "one group found on the host")
