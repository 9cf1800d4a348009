"""CPU: the sampler restatement (tests/sampler_oracle.py) and its fixture builder, the plugin's gate and noise draw for
aic_sample_topk_topp, and the argument checks of ops.sample_tokens."""
import types

import numpy as np
import pytest
import torch

import sampler_oracle as O
import sampling_oracle as S
from arcticinference_amd import _native

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _check_batch(b):
    """Builder properties on the sampler's f32 x, the 2 % cap, and the literal restatement against f64."""
    B, V = b.logits.shape
    assert b.rebuilt <= 0.02 * B and b.redrawn <= 0.02 * B, (b.rebuilt, b.redrawn, B)
    for r in range(B):
        if b.temps[r] <= 0:
            continue
        x = O.scaled_f32(b.logits[r], b.temps[r])
        assert O.cumsums_clear(x, b.ks[r], b.ps[r])
        # the literal f32 restatement keeps the contract's set
        k = S._norm_k(torch.tensor([b.ks[r]]), V)
        m = S.apply_top_k_top_p(torch.from_numpy(x).float()[None], k, torch.tensor([b.ps[r]]) if b.ps[r] < 1.0 else None)
        assert ((m[0] != -float("inf")).numpy() == S.kept_f64(x, b.ks[r], b.ps[r])).all(), r
    want, worst = O.sample_f64(b.logits, b.temps, b.ks, b.ps, b.q)
    assert worst >= O.WINNER_MARGIN
    assert torch.equal(O.sample_literal(b.logits, b.temps, b.ks, b.ps, b.q), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [1000, 32007])
def test_small_batches_of_the_gpu_tests(dtype, V):
    for modes in O.SMALL_MODES:
        _check_batch(O.small_case(dtype, V, modes))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_cut_batches_of_the_gpu_tests(dtype):
    _check_batch(O.tie_case(dtype))


@pytest.mark.parametrize("V", [128256, 201088])
def test_full_vocab_batches_of_the_gpu_tests(V):
    b = O.full_case(V)
    _check_batch(b)
    assert sum(t <= 0 for t in b.temps) > 0 and sum(p < 1.0 for p in b.ps) > 10


def test_filters_may_be_absent_and_greedy_rows_ignore_theirs():
    b = O.small_case(torch.bfloat16, 1000, ("kp", "g", "p", "t", "k"))
    plain = O.sample_literal(b.logits, b.temps, None, None, b.q)
    t = torch.tensor(b.temps)
    x = b.logits.float() / torch.where(t > 0, t, torch.ones_like(t))[:, None]
    want = torch.where(t > 0, (torch.softmax(x, dim=-1) / b.q).argmax(dim=-1), b.logits.float().argmax(dim=-1))
    assert torch.equal(plain, want.to(torch.int32))
    got = O.sample_literal(b.logits, b.temps, b.ks, b.ps, b.q)
    g = [i for i, T in enumerate(b.temps) if T <= 0]
    assert g and all(int(got[i]) == int(b.logits[i].float().argmax()) for i in g)


def test_f32_scaling_and_rounded_scaling_keep_different_sets():
    lg, T, ks, ps = O.rounding_split_rows()
    x32 = [O.scaled_f32(lg[r], T[r]) for r in range(2)]
    x16 = [S.scaled(lg[r], T[r]) for r in range(2)]
    assert x32[0][100] != x32[0][200] and x16[0][100] == x16[0][200]        # the pair differs in f32, ties in bf16
    assert np.nonzero(S.kept_f64(x32[0], ks[0], ps[0]))[0].tolist() == [7, 200]
    assert np.nonzero(S.kept_f64(x16[0], ks[0], ps[0]))[0].tolist() == [7, 100, 200]
    assert np.nonzero(S.kept_f64(x32[1], ks[1], ps[1]))[0].tolist() == [9, 50]
    assert np.nonzero(S.kept_f64(x16[1], ks[1], ps[1]))[0].tolist() == [9, 300]
    for r in range(2):
        assert O.cumsums_clear(x32[r], ks[r], ps[r])


# ---------------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------------
def _sm(**kw):
    base = dict(max_num_logprobs=None, no_penalties=True, allowed_token_ids_mask=None, bad_words_token_ids={},
                logit_bias=[None, None, None], min_tokens={}, min_p=None, all_greedy=False,
                temperature=torch.tensor([-1.0, 0.7, 1.0]), top_k=None, top_p=None, generators={})
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_hip_sampler_ok_field_by_field(monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic as R
    tk, tp = torch.tensor([0, 40, 0]), torch.tensor([1.0, 0.9, 1.0])
    for kw in (dict(), dict(top_k=tk), dict(top_p=tp), dict(top_k=tk, top_p=tp)):
        assert R.hip_sampler_ok(_sm(**kw))
        assert not R.hip_sampler_ok(_sm(max_num_logprobs=2, **kw))
        assert not R.hip_sampler_ok(_sm(max_num_logprobs=0, **kw))
        assert not R.hip_sampler_ok(_sm(no_penalties=False, **kw))
        assert not R.hip_sampler_ok(_sm(allowed_token_ids_mask=torch.zeros(3, 8, dtype=torch.bool), **kw))
        assert not R.hip_sampler_ok(_sm(bad_words_token_ids={1: [[5]]}, **kw))
        assert not R.hip_sampler_ok(_sm(logit_bias=[None, {3: 1.0}, None], **kw))
        assert not R.hip_sampler_ok(_sm(min_tokens={0: (2, {1})}, **kw))
        assert not R.hip_sampler_ok(_sm(min_p=torch.zeros(3), **kw))
        assert not R.hip_sampler_ok(_sm(temperature=None, **kw))
        assert R.hip_sampler_ok(_sm(all_greedy=True, temperature=None, **kw))
        assert R.hip_sampler_ok(_sm(logit_bias=[None, {}, None], **kw))
    monkeypatch.delenv(R.HIP_SAMPLER_ENV, raising=False)
    assert R.HIP_SAMPLER_ENV == "ARCTIC_INFERENCE_HIP_SAMPLER" and not R.hip_sampler_switch()
    monkeypatch.setenv(R.HIP_SAMPLER_ENV, "1")
    monkeypatch.delenv(R.TOP_K_TOP_P_ENV, raising=False)
    assert R.hip_sampler_switch() and not R.top_k_top_p_switch()      # the two switches are independent
    monkeypatch.setenv(R.HIP_SAMPLER_ENV, "0")
    assert not R.hip_sampler_switch()


# ---------------------------------------------------------------------------------------------------------------------
# the noise draw
# ---------------------------------------------------------------------------------------------------------------------
def test_draw_sampler_noise_consumes_generators_like_the_stand_in_sampler(stub_vllm):
    from vllm.v1.worker.gpu_model_runner import Sampler
    from arcticinference_amd.vllm_plugin.model_runner import draw_sampler_noise
    B, V = 4, 300
    mk = lambda: {1: torch.Generator().manual_seed(11), 3: torch.Generator().manual_seed(12)}
    gens, twins = mk(), mk()
    q = draw_sampler_noise(B, V, gens, torch.device("cpu"))
    assert q.dtype == torch.float32 and q.shape == (B, V) and bool((q > 0).all())
    for i, g in twins.items():
        assert torch.equal(q[i], torch.empty(V).exponential_(generator=g))
    # a second draw continues the generators' streams, as a second sampler call does
    q2 = draw_sampler_noise(B, V, gens, torch.device("cpu"))
    for i, g in twins.items():
        assert torch.equal(q2[i], torch.empty(V).exponential_(generator=g))
    # the stand-in Sampler, fed twin generators, picks the tokens this noise picks
    logits = torch.randn(B, V, generator=torch.Generator().manual_seed(0))
    temp = torch.tensor([0.9, 0.7, 1.1, 1.3])
    sm = types.SimpleNamespace(all_greedy=False, temperature=temp, generators=mk())
    torch.manual_seed(5)
    out = Sampler()(logits, sm).sampled_token_ids.view(-1)
    torch.manual_seed(5)
    q3 = draw_sampler_noise(B, V, mk(), torch.device("cpu"))
    assert torch.equal(out, (torch.softmax(logits / temp[:, None], dim=-1) / q3).argmax(dim=-1).to(torch.int32))


def test_draw_sampler_noise_leaves_the_default_generator_alone_when_every_row_is_seeded():
    from arcticinference_amd.vllm_plugin.model_runner import draw_sampler_noise
    gens = {i: torch.Generator().manual_seed(20 + i) for i in range(3)}
    torch.manual_seed(9)
    before = torch.get_rng_state()
    q = draw_sampler_noise(3, 64, gens, torch.device("cpu"))
    assert torch.equal(torch.get_rng_state(), before)
    for i in range(3):
        assert torch.equal(q[i], torch.empty(64).exponential_(generator=torch.Generator().manual_seed(20 + i)))
    draw_sampler_noise(3, 64, {0: gens[0]}, torch.device("cpu"))
    assert not torch.equal(torch.get_rng_state(), before)


# ---------------------------------------------------------------------------------------------------------------------
# ops.sample_tokens and the entry point without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_tokens_has_no_cpu_fallback_and_checks_its_arguments():
    from arcticinference_amd import ops
    lg = torch.zeros(3, 8)
    t = torch.ones(3)
    q = torch.ones(3, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t, q)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_tokens(lg, t[:2], q[:2], top_k=torch.tensor([1, 2]), top_p=torch.tensor([0.5, 0.5]),
                          row_index=torch.tensor([2, 0]))
    with pytest.raises(ValueError, match="logits"):
        ops.sample_tokens(torch.zeros(8), t, q)
    with pytest.raises(ValueError, match="row_index"):
        ops.sample_tokens(lg, t, q, row_index=torch.tensor([0, 1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="one value per row"):
        ops.sample_tokens(lg, t[:2], q)
    with pytest.raises(ValueError, match="one value per row"):
        ops.sample_tokens(lg, t, q, top_k=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="one value per row"):
        ops.sample_tokens(lg, t, q, top_p=torch.tensor([0.5]))
    with pytest.raises(ValueError, match="exp_noise"):
        ops.sample_tokens(lg, t, q[:2])
    with pytest.raises(ValueError, match="exp_noise"):
        ops.sample_tokens(lg, t, q.double())


def test_the_entry_point_fails_loudly_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    L = _native.lib()
    assert L.aic_sample_workspace_bytes(64, 128256, _native.DT_BF16) > 0
    lg = torch.zeros(2, 16)
    t = torch.ones(2)
    q = torch.ones(2, 16)
    out = torch.zeros(2, dtype=torch.int32)
    ws = torch.zeros(L.aic_sample_workspace_bytes(2, 16, _native.DT_F32), dtype=torch.uint8)
    rc = L.aic_sample_topk_topp(lg.data_ptr(), _native.DT_F32, 16, 16, None, t.data_ptr(), q.data_ptr(), None, None, 2,
                                out.data_ptr(), ws.data_ptr(), None)
    assert rc == _native.AIC_ERR_NO_DEVICE
    assert L.aic_sample_topk_topp(None, _native.DT_F32, 16, 16, None, None, None, None, None, 0, None, None, None) == 0
    assert L.aic_sample_topk_topp(None, _native.DT_F32, 16, 16, None, t.data_ptr(), q.data_ptr(), None, None, 2,
                                  out.data_ptr(), ws.data_ptr(), None) == _native.AIC_ERR_INVALID
