"""CPU: the plugin's gates with the logprobs switch, the two logprobs oracles against each other on every fixture of the
GPU tests, and the argument checks of ops.token_logprobs / aic_token_logprobs without a device."""
import types

import numpy as np
import pytest
import torch

import logprobs_oracle as LO
from arcticinference_amd import _native


def _sm(**kw):
    base = dict(max_num_logprobs=None, no_penalties=True, allowed_token_ids_mask=None, bad_words_token_ids={},
                logit_bias=[None, None, None], min_tokens={}, min_p=None, all_greedy=False,
                temperature=torch.tensor([-1.0, 0.7, 1.0]), top_k=None, top_p=None, generators={})
    base.update(kw)
    return types.SimpleNamespace(**base)


_TK, _TP = torch.tensor([0, 40, 0]), torch.tensor([1.0, 0.9, 1.0])
_METADATA = {"greedy": dict(all_greedy=True, temperature=None), "random": dict(),
             "filtered": dict(top_k=_TK, top_p=_TP)}
_KIND = {"greedy": "greedy", "random": "random", "filtered": "random_topk_topp"}
_EXCLUSIONS = (dict(no_penalties=False), dict(allowed_token_ids_mask=torch.zeros(3, 8, dtype=torch.bool)),
               dict(bad_words_token_ids={1: [[5]]}), dict(logit_bias=[None, {3: 1.0}, None]),
               dict(min_tokens={0: (2, {1})}), dict(min_p=torch.zeros(3)))


def test_the_cap_is_the_librarys():
    assert _native.lib().aic_logprobs_max() == LO.CAP == 32
    from arcticinference_amd.vllm_plugin import runner_logic as R
    assert R.logprobs_cap() == LO.CAP


@pytest.mark.parametrize("which", list(_METADATA))
def test_gates_admit_logprobs_up_to_the_cap_with_the_switch(which):
    from arcticinference_amd.vllm_plugin import runner_logic as R
    kw = _METADATA[which]
    for n in (0, 5, LO.CAP):
        assert R.hip_acceptance_kind(_sm(max_num_logprobs=n, **kw), True, logprobs=True) == _KIND[which]
        assert R.hip_sampler_ok(_sm(max_num_logprobs=n, **kw), logprobs=True)
    assert R.hip_acceptance_kind(_sm(max_num_logprobs=LO.CAP + 1, **kw), True, logprobs=True) is None
    assert not R.hip_sampler_ok(_sm(max_num_logprobs=LO.CAP + 1, **kw), logprobs=True)
    assert R.hip_acceptance_kind(_sm(max_num_logprobs=-1, **kw), True, logprobs=True) is None
    # every other exclusion still excludes, with and without logprobs beside it
    for ex in _EXCLUSIONS:
        for lp in (dict(), dict(max_num_logprobs=3)):
            assert R.hip_acceptance_kind(_sm(**ex, **lp, **kw), True, logprobs=True) is None
            assert not R.hip_sampler_ok(_sm(**ex, **lp, **kw), logprobs=True)
    # top-k / top-p still need their own switch
    if which == "filtered":
        assert R.hip_acceptance_kind(_sm(max_num_logprobs=3, **kw), False, logprobs=True) is None


@pytest.mark.parametrize("which", list(_METADATA))
def test_gates_give_todays_answers_by_default(which):
    from arcticinference_amd.vllm_plugin import runner_logic as R
    kw = _METADATA[which]
    assert R.hip_acceptance_kind(_sm(**kw), True) == R.hip_acceptance_kind(_sm(**kw), True, logprobs=True) == _KIND[which]
    assert R.hip_sampler_ok(_sm(**kw)) and R.hip_sampler_ok(_sm(**kw), logprobs=True)
    for n in (0, 2, LO.CAP):
        assert R.hip_acceptance_kind(_sm(max_num_logprobs=n, **kw), True) is None
        assert R.hip_acceptance_kind(_sm(max_num_logprobs=n, **kw), True, False) is None
        assert not R.hip_sampler_ok(_sm(max_num_logprobs=n, **kw))
        assert not R.hip_sampler_ok(_sm(max_num_logprobs=n, **kw), False)


def test_logprobs_switch_parses_like_its_siblings(monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic as R
    assert R.LOGPROBS_ENV == "ARCTIC_INFERENCE_HIP_LOGPROBS"
    monkeypatch.delenv(R.LOGPROBS_ENV, raising=False)
    assert not R.logprobs_switch()
    for v in ("1", "true", " On ", "YES"):
        monkeypatch.setenv(R.LOGPROBS_ENV, v)
        assert R.logprobs_switch()
    for v in ("0", "", "off", "2"):
        monkeypatch.setenv(R.LOGPROBS_ENV, v)
        assert not R.logprobs_switch()
    monkeypatch.setenv(R.LOGPROBS_ENV, "1")
    monkeypatch.delenv(R.HIP_SAMPLER_ENV, raising=False)
    monkeypatch.delenv(R.TOP_K_TOP_P_ENV, raising=False)
    assert not R.hip_sampler_switch() and not R.top_k_top_p_switch()      # the switches are independent


# ---------------------------------------------------------------------------------------------------------------------
# the oracles on the GPU tests' fixtures
# ---------------------------------------------------------------------------------------------------------------------
CASES = LO.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_literal_restatement_meets_the_f64_oracle_on_the_gpu_fixtures(case):
    lg = case.served()
    ids64, lp64, rank64 = LO.f64_oracle(lg, case.token_ids, case.n)
    ids, lp, ranks = LO.vllm_literal(lg, torch.tensor(case.token_ids), case.n)
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32 and ranks.dtype == torch.int64
    assert ids.shape == lp.shape == (lg.shape[0], 1 + case.n)
    # the f64 oracle returns the planted indices in the planted order
    assert ids64[:, 1:].tolist() == case.planted
    assert ids64[:, 0].tolist() == case.token_ids
    tied = "ties" in case.name or "masked" in case.name
    if not tied:        # torch.topk leaves the order of equal values open: only untied rows pin the literal's ids
        assert ids[:, 1:].tolist() == case.planted
        assert ranks.tolist() == rank64.tolist()
    assert ids[:, 0].tolist() == case.token_ids
    assert LO.within_bar(lp.numpy(), lp64).all(), LO.max_excess(lp.numpy(), lp64)


def test_rank_kinds_of_the_planted_rows():
    c = LO.planted_case(1000, torch.bfloat16, 5, 5)
    _, _, ranks = LO.f64_oracle(c.served(), c.token_ids, c.n)
    assert ranks.tolist() == [1, 5 // 2 + 1, 5 + 1, 1000, 5 + 2 + 7]      # top, mid, outside, min, tied7
    t = LO.tie_case(1000, torch.float16)
    _, _, ranks = LO.f64_oracle(t.served(), t.token_ids, t.n)
    assert ranks.tolist() == [t.n + 2, 3, 2]
    m = LO.masked_case(1000, torch.float32)
    ids, lps, ranks = LO.f64_oracle(m.served(), m.token_ids, m.n)
    assert np.isneginf(lps[:, 6:]).all() and np.isfinite(lps[:, 1:6]).all() and ranks.tolist() == [3, 1000]
    assert np.allclose(np.exp(lps[:, 1:6]).sum(-1), 1.0)                  # the 5-way log-softmax


def test_arg_max_form_of_the_oracle_takes_the_lowest_tied_index():
    t = LO.tie_case(1000, torch.bfloat16)
    ids, _, ranks = LO.f64_oracle(t.served(), None, t.n)
    assert ids[2, 0] == min(t.planted[2][:2]) and ranks[2] == 2 and ranks[0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# ops.token_logprobs and the entry point without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_token_logprobs_has_no_cpu_fallback_and_checks_its_arguments():
    from arcticinference_amd import ops
    lg = torch.zeros(3, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_logprobs(lg, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.token_logprobs(lg, 0, token_ids=torch.tensor([1, 2]), row_index=torch.tensor([2, 0]))
    with pytest.raises(ValueError, match="logits"):
        ops.token_logprobs(torch.zeros(8), 1)
    with pytest.raises(ValueError, match="row_index"):
        ops.token_logprobs(lg, 1, row_index=torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="one token per row"):
        ops.token_logprobs(lg, 1, token_ids=torch.tensor([1, 2]))
    for n in (-1, LO.CAP + 1):
        with pytest.raises(ValueError, match="num_logprobs"):
            ops.token_logprobs(lg, n)
    with pytest.raises(ValueError, match="num_logprobs"):
        ops.token_logprobs(torch.zeros(3, 4), 5)


def test_the_entry_point_checks_before_it_needs_a_device():
    """Return codes that do not depend on a device being present (the calls that would launch pass no rows)."""
    L = _native.lib()
    assert L.aic_logprobs_workspace_bytes(64, 201088, _native.DT_BF16, 20) > 0
    lg = torch.zeros(2, 64)
    ids = torch.zeros(2, 40, dtype=torch.int32)
    lp = torch.zeros(2, 40)
    rk = torch.zeros(2, dtype=torch.int64)
    ws = torch.zeros(L.aic_logprobs_workspace_bytes(2, 64, _native.DT_F32, 3), dtype=torch.uint8)
    args = lambda dt, rows, n: (lg.data_ptr(), dt, 64, 64, None, None, rows, n, ids.data_ptr(), lp.data_ptr(),
                                rk.data_ptr(), ws.data_ptr(), None)
    assert L.aic_token_logprobs(*args(_native.DT_F32, 2, LO.CAP + 1)) == _native.AIC_ERR_INVALID
    assert L.aic_token_logprobs(*args(_native.DT_F32, 2, -1)) == _native.AIC_ERR_INVALID
    assert L.aic_token_logprobs(*args(_native.DT_FP8_E4M3, 2, 3)) == _native.AIC_ERR_UNSUPPORTED
    assert L.aic_token_logprobs(*args(_native.DT_F32, 0, 3)) == 0                         # rows == 0: a no-op
    assert L.aic_token_logprobs(None, _native.DT_F32, 64, 64, None, None, 2, 3, ids.data_ptr(), lp.data_ptr(),
                                rk.data_ptr(), ws.data_ptr(), None) == _native.AIC_ERR_INVALID
    if not torch.cuda.is_available():
        assert L.aic_token_logprobs(*args(_native.DT_F32, 2, 3)) == _native.AIC_ERR_NO_DEVICE
