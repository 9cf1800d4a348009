"""CPU: the top-k / top-p restatement (tests/sampling_oracle.py), its fixture builder, and the plugin's routing switch
for aic_rejection_random_topk_topp."""
import types

import numpy as np
import pytest
import torch

import sampling_oracle as S


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", ["k", "p", "kp"])
@pytest.mark.parametrize("V", [1000, 32007])
def test_builder_rows_have_the_same_kept_set_in_f64_and_in_the_literal_restatement(dtype, mode, V):
    rng = np.random.default_rng(V + len(mode))
    for i in range(6):
        T = (1.0, 0.8)[i % 2]
        row, k, p = S.build_row(V, dtype, rng, T, mode, tie_cut=(i % 3 == 2 and "p" in mode))
        want = S.kept_f64(S.scaled(row, T), k, p)
        assert (S.literal_kept(row, T, k, p) == want).all(), (mode, i, k, p)
        assert 1 <= want.sum() < V


def test_top_p_ties_at_the_boundary_are_dropped_from_the_lowest_index_up():
    x = torch.tensor([0.0, 2.0, 1.0, 2.0, 2.0, 1.0, 2.0], dtype=torch.bfloat16)
    xf = S.scaled(x, 1.0)
    e = np.exp(xf - xf.max())
    pr = e / e.sum()                                    # four ties at 2.0 carry ~0.22 each
    one_minus_p = pr[0] + 2 * pr[2] + 2.5 * pr[1]       # midway through the ties: the first two tied indices go
    keep = S.kept_f64(xf, 7, 1.0 - one_minus_p)
    assert keep.tolist() == [False, False, False, False, True, False, True]
    assert S.literal_kept(x, 1.0, 7, 1.0 - one_minus_p).tolist() == keep.tolist()


def test_top_k_keeps_every_tie_of_the_kth_value():
    x = torch.tensor([5.0, 3.0, 4.0, 3.0, 1.0, 3.0], dtype=torch.bfloat16)
    for k in (3, 4, 5):
        keep = S.kept_f64(S.scaled(x, 1.0), k, 1.0)
        assert keep.tolist() == [True, True, True, True, False, True]
        assert S.literal_kept(x, 1.0, k, 1.0).tolist() == keep.tolist()
    assert S.kept_f64(S.scaled(x, 1.0), 2, 1.0).tolist() == [True, False, True, False, False, False]


def test_disabled_filters_leave_rows_unfiltered():
    rng = np.random.default_rng(0)
    row = torch.from_numpy(rng.standard_normal(300).astype(np.float32)).to(torch.bfloat16)
    for k, p in ((300, 1.0), (0, 1.0), (-3, 1.0), (300, 1.5)):
        assert S.kept_f64(S.scaled(row, 0.9), k, p).all()
        assert S.literal_kept(row, 0.9, k, min(p, 1.0)).all()
    probs = S.compute_probs(row[None], torch.tensor([0.9]), torch.tensor([0]), torch.tensor([1.0]))
    plain = torch.softmax((row.float() / 0.9).to(torch.bfloat16).float(), dim=-1)
    assert torch.equal(probs[0], plain)


def test_tiny_p_keeps_only_the_largest_survivor():
    x = torch.tensor([1.0, 3.0, 2.0, 3.0, 0.5], dtype=torch.bfloat16)
    keep = S.kept_f64(S.scaled(x, 1.0), 5, 1e-6)
    assert keep.tolist() == [False, False, False, True, False]   # ties of the maximum: the largest index stays
    assert S.literal_kept(x, 1.0, 5, 1e-6).tolist() == keep.tolist()


def _sm(**kw):
    base = dict(max_num_logprobs=None, no_penalties=True, allowed_token_ids_mask=None, bad_words_token_ids={},
                logit_bias=[None, None, None], min_tokens={}, min_p=None, all_greedy=False,
                temperature=torch.tensor([-1.0, 0.7, 1.0]), top_k=None, top_p=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_hip_acceptance_kind_sends_top_k_top_p_batches_to_the_new_kernel_only_with_the_switch(monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic as R
    tk, tp = torch.tensor([0, 40, 0]), torch.tensor([1.0, 0.9, 1.0])
    for kw in (dict(top_k=tk), dict(top_p=tp), dict(top_k=tk, top_p=tp)):
        assert R.hip_acceptance_kind(_sm(**kw)) is None
        assert R.hip_acceptance_kind(_sm(**kw), False) is None
        assert R.hip_acceptance_kind(_sm(**kw), True) == R.KIND_TOP_K_TOP_P
        # the other exclusions stay
        assert R.hip_acceptance_kind(_sm(min_p=torch.zeros(3), **kw), True) is None
        assert R.hip_acceptance_kind(_sm(max_num_logprobs=2, **kw), True) is None
        assert R.hip_acceptance_kind(_sm(no_penalties=False, **kw), True) is None
        assert R.hip_acceptance_kind(_sm(logit_bias=[None, {3: 1.0}, None], **kw), True) is None
        assert R.hip_acceptance_kind(_sm(min_tokens={0: (2, {1})}, **kw), True) is None
        assert R.hip_acceptance_kind(_sm(temperature=None, **kw), True) is None
    assert R.hip_acceptance_kind(_sm(), True) == "random"
    assert R.hip_acceptance_kind(_sm(all_greedy=True, temperature=None, top_p=tp), True) == "greedy"
    monkeypatch.delenv(R.TOP_K_TOP_P_ENV, raising=False)
    assert not R.top_k_top_p_switch()
    monkeypatch.setenv(R.TOP_K_TOP_P_ENV, "1")
    assert R.top_k_top_p_switch()
    monkeypatch.setenv(R.TOP_K_TOP_P_ENV, "0")
    assert not R.top_k_top_p_switch()


def test_rejection_sample_rejects_top_k_top_p_without_temperature():
    from arcticinference_amd import ops
    lg = torch.zeros(2, 8)
    d = torch.zeros(2, dtype=torch.int32)
    cu = torch.tensor([2], dtype=torch.int32)
    b = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="temperature"):
        ops.rejection_sample(lg, d, cu, b, 2, top_k=torch.tensor([3]))
    with pytest.raises(ValueError, match="temperature"):
        ops.rejection_sample(lg, d, cu, b, 2, top_p=torch.tensor([0.5]))
