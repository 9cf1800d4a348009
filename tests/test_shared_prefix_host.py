"""CPU: the host half of the shared-prefix (cascade) attention call.

  * the marked-key probe of tests/shared_prefix_fixtures.py: the oracle returns its closed form, and a reference that
    drops the marked key, or counts it twice, moves every concerned row by at least ten times the bar — so the GPU test
    that uses the probe at the seam cannot pass with either fault;
  * runner_logic.shared_prefix_len, the plugin's decision;
  * ops.verify_attention's argument rules, which are answered before the device check;
  * the header declares the entry points and the built library exports them."""
import os
from types import SimpleNamespace

import pytest
import torch

import attention_fixtures as F
import shared_prefix_fixtures as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Requests 1 and 3: ctx - q_len == 64 exactly.  Every context <= 92: a row at position p that counts key t twice moves by
# p / ((p + 1) (p + 2)), which is ten times the bar up to p = 92 (and no further), one that drops it by 1 / (p + 1).
Q_LENS, CTXS = [1, 2, 5, 28], [70, 66, 90, 92]


@pytest.mark.parametrize("t", [0, 31, 32, 63, 64, 95])
def test_marked_key_probe_closed_form_and_mutants(t):
    c = S.marked_key_case(t, Q_LENS, CTXS, Hq=4, Hkv=2, D=64, bs=16, shared_len=64)
    assert min(q for q in Q_LENS) >= 1 and any(cx - ql == 64 for ql, cx in zip(Q_LENS, CTXS)) and max(CTXS) <= 92
    want = F.oracle(c)
    assert torch.allclose(want, c.expected, atol=1e-6, rtol=1e-5)
    assert torch.allclose(S.marked_reference(c).float(), c.expected, atol=1e-6, rtol=1e-5)
    concerned = c.pos >= t
    if t >= max(CTXS):               # the marker sits behind every context: nobody sees it, everything is zero
        assert not concerned.any() and float(c.expected.abs().max()) == 0.0
        return
    assert concerned.any()
    for w in (0.0, 2.0):             # key t dropped / counted twice
        moved = (S.marked_reference(c, w) - c.expected.double()).abs()
        floor = 10.0 * S.bar(c.expected.double())
        assert bool((moved[concerned] >= floor[concerned]).all()), (t, w, float(moved[concerned].min()))
        assert float(moved[~concerned].max()) == 0.0 if (~concerned).any() else True


def test_share_prefix_shares_pages_and_keeps_the_keys():
    c0 = F.planted_case([1, 3], [300, 290], 4, 1, 128, 16, seed=5)
    k_before = [c0.kc[c0.bt[i, :16].long()].clone() for i in range(2)]
    c = S.share_prefix(c0, 256)
    assert torch.equal(c.bt[1, :16], c.bt[0, :16]) and not torch.equal(c.bt[1, 16:18], c.bt[0, 16:18])
    assert torch.equal(c.prefix_table, c.bt[0, :16])
    assert torch.equal(c.kc[c.bt[1, :16].long()], k_before[1])         # position-coded keys: K is what it was
    with pytest.raises(AssertionError):
        S.share_prefix(F.planted_case([40], [290], 4, 1, 128, 16, seed=5), 256)   # a query token inside the prefix


# ---- the plugin's decision ------------------------------------------------------------------------------------------
def _meta(**kw):
    return SimpleNamespace(**kw)


def test_shared_prefix_len_rule(monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic
    from arcticinference_amd.vllm_plugin.runner_logic import shared_prefix_len
    # the rule itself, with the thresholds at the kernel's floor (the shipped ones are measured break-evens: below)
    monkeypatch.setattr(runner_logic, "SHARED_PREFIX_MIN_LEN", 32)
    monkeypatch.setattr(runner_logic, "SHARED_PREFIX_MIN_ITEMS", 1)
    monkeypatch.setattr(runner_logic, "SHARED_PREFIX_MIN_ITEMS_FP8", 1)
    cascade = _meta(use_cascade=True, common_prefix_len=2048)
    assert shared_prefix_len(cascade, 0, False, True) == 2048
    assert shared_prefix_len(cascade, None, False, True) == 2048
    assert shared_prefix_len(cascade, 0, False, False) == 0                       # switch off
    assert shared_prefix_len(_meta(), 0, False, True) == 0                        # no attributes (the stand-in's metadata)
    assert shared_prefix_len(_meta(common_prefix_len=2048), 0, False, True) == 0
    assert shared_prefix_len(_meta(use_cascade=False, common_prefix_len=2048), 0, False, True) == 0
    assert shared_prefix_len(cascade, 128, False, True) == 0                      # a windowed layer
    assert shared_prefix_len(cascade, 0, True, True) == 0                         # capturing
    for n, want in ((0, 0), (16, 0), (31, 0), (32, 32), (2048, 2048)):
        assert shared_prefix_len(_meta(use_cascade=True, common_prefix_len=n), 0, False, True) == want
    assert shared_prefix_len(_meta(use_cascade=True), 0, False, True) == 0
    assert shared_prefix_len(None, 0, False, True) == 0
    monkeypatch.setattr(runner_logic, "SHARED_PREFIX_MIN_LEN", 0)        # never below one tile, whatever the constant
    assert shared_prefix_len(_meta(use_cascade=True, common_prefix_len=31), 0, False, True) == 0


def test_shipped_thresholds_are_the_measured_break_evens():
    from arcticinference_amd.vllm_plugin import runner_logic as R
    assert (R.SHARED_PREFIX_MIN_LEN, R.SHARED_PREFIX_MIN_ITEMS, R.SHARED_PREFIX_MIN_ITEMS_FP8) == (2048, 256, 512)

    def ask(n, requests, kv_heads=None, fp8=False, **kw):
        meta = _meta(use_cascade=True, common_prefix_len=n, seq_lens=torch.zeros(requests, dtype=torch.int32), **kw)
        return R.shared_prefix_len(meta, 0, False, True, kv_heads, fp8)
    # the measured shapes, 8 kv heads: wins are taken, losses refused
    assert ask(2048, 64, 8) == 2048 and ask(2048, 32, 8) == 2048 and ask(2048, 31, 8) == 0 and ask(2048, 8, 8) == 0
    assert ask(2048, 64, 8, fp8=True) == 2048 and ask(2048, 32, 8, fp8=True) == 0 and ask(2048, 63, 8, fp8=True) == 0
    assert ask(1024, 64, 8) == 0 and ask(2047, 64, 8) == 0 and ask(4096, 64, 8) == 4096
    # a rank of Ulysses SP = 8 (one kv head): the measured 64 requests lose, and are refused
    assert ask(2048, 64, 1) == 0 and ask(2048, 255, 1) == 0 and ask(2048, 256, 1) == 2048
    assert ask(2048, 256, 1, fp8=True) == 0 and ask(2048, 512, 1, fp8=True) == 2048
    assert ask(2048, 32) == 2048 and ask(2048, 31) == 0                    # kv heads not named: the measured 8
    # no query token behind the prefix: the plain call, not an argument error inside the step
    assert ask(2048, 64, 8, max_seq_len=2048) == 0 and ask(2048, 64, 8, max_seq_len=2049) == 2048
    assert R.shared_prefix_len(_meta(use_cascade=True, common_prefix_len=2048), 0, False, True) == 2048   # no seq_lens: length only


def test_switch_is_read_when_the_step_is_published(monkeypatch):
    import numpy as np
    from arcticinference_amd.vllm_plugin import step_context
    from arcticinference_amd.vllm_plugin.runner_logic import SHARED_PREFIX_ENV
    assert SHARED_PREFIX_ENV == "ARCTIC_INFERENCE_HIP_SHARED_PREFIX" and "shared_prefix" in step_context.calls
    try:
        monkeypatch.delenv(SHARED_PREFIX_ENV, raising=False)
        step_context.publish(np.array([1, 1]), False)
        assert not step_context.shared_prefix_on()
        monkeypatch.setenv(SHARED_PREFIX_ENV, "1")
        assert not step_context.shared_prefix_on()           # not before the next step
        step_context.publish(np.array([1, 1]), False)
        assert step_context.shared_prefix_on()
    finally:
        monkeypatch.delenv(SHARED_PREFIX_ENV, raising=False)
        step_context.publish(np.array([1]), False)
        step_context.clear()


# ---- ops.verify_attention: answered before the device check ----------------------------------------------------------
def _call(shared_prefix_len, table, q_lens=(1, 2), seq_lens=(100, 80), **kw):
    from arcticinference_amd import ops
    Hq, Hkv, D, bs = 4, 1, 128, 16
    T = sum(q_lens)
    q = torch.zeros(T, Hq, D, dtype=torch.bfloat16)
    kc = torch.zeros(16, bs, Hkv, D, dtype=torch.bfloat16)
    bt = torch.zeros(len(q_lens), 8, dtype=torch.int32)
    qsl = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32)
    return ops.verify_attention(q, kc, kc.clone(), bt, torch.tensor(seq_lens, dtype=torch.int32), qsl, max(q_lens),
                                max(seq_lens), D ** -0.5, q_lens_host=list(q_lens), shared_prefix_len=shared_prefix_len,
                                prefix_block_table=table, **kw)


def test_ops_refuses_bad_prefix_arguments_without_a_device():
    good = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="sliding window"):
        _call(64, good, sliding_window=128)
    with pytest.raises(ValueError, match="pages"):
        _call(64, torch.zeros(3, dtype=torch.int32))                   # 64 tokens in pages of 16 need 4
    with pytest.raises(ValueError, match="int32"):
        _call(64, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="prefix_block_table"):
        _call(64, None)
    with pytest.raises(ValueError, match="int32"):
        _call(64, torch.zeros(8, dtype=torch.int32)[::2])              # not contiguous
    with pytest.raises(ValueError, match="request 1"):
        _call(64, good, q_lens=(1, 2), seq_lens=(100, 65))             # 65 - 2 < 64
    with pytest.raises(ValueError, match="request 0"):
        _call(64, good, q_lens=(1, 2), seq_lens=(100, 80), seq_lens_host=[64, 80])    # the host lengths decide
    with pytest.raises(ValueError, match=">= 0"):
        _call(-32, good)
    # a good call gets as far as the device check (CPU tensors): nothing above is what stops it
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(64, good)
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(0, None)


# ---- header and library ---------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from arcticinference_amd import _native as N
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    for name in ("aic_verify_attention_prefix", "aic_debug_attn_prefix_splits"):
        assert f"int {name}(" in text, name
        assert name in N._SIGNATURES and name in N.EXPORTED_SYMBOLS
        assert hasattr(N.lib(), name), f"libarctic_hip.so lacks {name}"
    dt, px = N._SIGNATURES["aic_verify_attention_dt"][1], N._SIGNATURES["aic_verify_attention_prefix"][1]
    assert px[:len(dt) - 1] == dt[:-1] and len(px) == len(dt) + 2       # dt's arguments before `stream`, then two, then stream
    assert "ulysses.py:510" in text[text.index("aic_verify_attention_dt for a step whose requests begin"):
                                    text.index("int aic_verify_attention_prefix(")]


def test_entry_answers_argument_errors_before_any_launch():
    """A call that breaks the argument rules is answered before the device is looked for; without a device, one that keeps
    them ends at AIC_ERR_NO_DEVICE."""
    from arcticinference_amd import _native as N
    L = N.lib()

    def call(shared, table, window=0, max_seq_len=200):
        return L.aic_verify_attention_prefix(1, 512, 1, 1, 16 * 128, N.DT_BF16, None, None, 1, 8, 1, 1, 2, 3, 2, 4, 1, 128, 16,
                                             0.088, 1, 512, 1, 1 << 20, max_seq_len, None, 0, None, 0, window, None,
                                             N.DT_BF16, shared, table, None)
    assert call(-1, 1) == N.AIC_ERR_INVALID
    assert call(64, None) == N.AIC_ERR_INVALID
    assert call(64, 1, window=128) == N.AIC_ERR_UNSUPPORTED
    assert call(64, 1, max_seq_len=64) == N.AIC_ERR_INVALID
    if not torch.cuda.is_available():                    # (with a device these two would launch on the dummy pointers)
        assert call(64, 1) == N.AIC_ERR_NO_DEVICE
        assert call(0, None) == N.AIC_ERR_NO_DEVICE      # the plain call
    assert L.aic_debug_attn_prefix_splits(2) == N.AIC_OK and L.aic_debug_attn_prefix_splits(0) == N.AIC_OK
