"""CPU: the plugin's gates with the logits-edits switch, the packing of a SamplingMetadata into the arguments of
ops.edit_logits against literal per-request loops, the oracle of tests/logits_edit_oracle.py on a hand-computed case,
the min-p margin of every fixture the GPU tests use, and the argument checks of ops.edit_logits without a device."""
import types

import numpy as np
import pytest
import torch

import logits_edit_oracle as E

V = 8


def _sm(**kw):
    base = dict(max_num_logprobs=None, no_penalties=True, allowed_token_ids_mask=None, bad_words_token_ids={},
                logit_bias=[None, None, None], min_tokens={}, min_p=None, all_greedy=False,
                temperature=torch.tensor([-1.0, 0.7, 1.0]), top_k=None, top_p=None, generators={},
                prompt_token_ids=None, output_token_ids=[[], [], []], frequency_penalties=None, presence_penalties=None,
                repetition_penalties=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


_TK, _TP = torch.tensor([0, 40, 0]), torch.tensor([1.0, 0.9, 1.0])
_METADATA = {"greedy": dict(all_greedy=True, temperature=None), "random": dict(), "filtered": dict(top_k=_TK, top_p=_TP)}
_EDITS = {"penalties": dict(no_penalties=False), "mask": dict(allowed_token_ids_mask=torch.zeros(3, V, dtype=torch.bool)),
          "bad_words": dict(bad_words_token_ids={1: [[5]]}), "bias": dict(logit_bias=[None, {3: 1.0}, None]),
          "min_tokens": dict(min_tokens={0: (2, {1})}), "min_p": dict(min_p=torch.zeros(3))}


@pytest.mark.parametrize("field", list(_EDITS))
@pytest.mark.parametrize("which", list(_METADATA))
def test_gates_keep_todays_answers_without_the_keyword_and_ignore_the_field_with_it(which, field):
    from arcticinference_amd.vllm_plugin import logits_edits as L
    from arcticinference_amd.vllm_plugin import runner_logic as R
    kw, ex = _METADATA[which], _EDITS[field]
    assert L.has_edits(_sm(**ex, **kw)) and not L.has_edits(_sm(**kw))
    for filters in (False, True):
        for lp, n in ((False, None), (True, 3)):
            plain = _sm(max_num_logprobs=n, **kw)
            edited = _sm(max_num_logprobs=n, **ex, **kw)
            # without the keyword (and with it False): excluded, as on the parent commit
            assert R.hip_acceptance_kind(edited, filters, lp) is None
            assert R.hip_acceptance_kind(edited, filters, lp, logits_edits=False) is None
            assert not R.hip_sampler_ok(edited, lp) and not R.hip_sampler_ok(edited, lp, logits_edits=False)
            # with it: what the same metadata without the field gives
            assert R.hip_acceptance_kind(edited, filters, lp, logits_edits=True) == R.hip_acceptance_kind(plain, filters, lp)
            assert R.hip_sampler_ok(edited, lp, logits_edits=True) == R.hip_sampler_ok(plain, lp)
            # metadata without edits does not care about the keyword
            assert R.hip_acceptance_kind(plain, filters, lp, logits_edits=True) == R.hip_acceptance_kind(plain, filters, lp)
    # logprobs keep their own switch
    assert R.hip_acceptance_kind(_sm(max_num_logprobs=3, **ex, **kw), True, False, logits_edits=True) is None
    assert not R.hip_sampler_ok(_sm(max_num_logprobs=3, **ex, **kw), False, logits_edits=True)


def test_switch_parses_like_its_siblings(monkeypatch):
    from arcticinference_amd.vllm_plugin import logits_edits as L
    from arcticinference_amd.vllm_plugin import runner_logic as R
    assert R.LOGITS_EDITS_ENV == L.LOGITS_EDITS_ENV == "ARCTIC_INFERENCE_HIP_LOGITS_EDITS"
    monkeypatch.delenv(L.LOGITS_EDITS_ENV, raising=False)
    assert not L.logits_edits_switch()
    for value, want in (("1", True), ("true", True), (" ON ", True), ("0", False), ("", False), ("no", False)):
        monkeypatch.setenv(L.LOGITS_EDITS_ENV, value)
        assert L.logits_edits_switch() is want


class _Recorder:
    """Stands in for ops.rejection_sample: records the calls of one step."""

    def __init__(self):
        self.calls = []

    def rejection_sample(self, *a, **kw):
        self.calls.append(("accept", a, kw))
        n = a[2].numel()
        return types.SimpleNamespace(output_token_ids=torch.zeros(n, 3, dtype=torch.int32))


def test_an_all_greedy_verify_step_with_edits_passes_its_bonus_tokens_to_the_acceptance(stub_vllm, monkeypatch):
    """The routing alone, without a device: `logits.is_cuda` is what sends a step to the HIP routes, so the step runs on
    a CPU tensor that says it is on the GPU, with ops.rejection_sample recorded instead of launched."""
    import vllm_harness as H
    H.load_plugin()
    from arcticinference_amd.vllm_plugin import model_runner as MR
    from vllm.v1.outputs import SamplerOutput

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)

    rec = _Recorder()
    from arcticinference_amd import ops
    monkeypatch.setattr(ops, "rejection_sample", rec.rejection_sample)
    sampler_calls = []

    def sampler(logits, sampling_metadata):
        sampler_calls.append(tuple(logits.shape))
        return SamplerOutput(sampled_token_ids=torch.full((logits.shape[0], 1), 5, dtype=torch.int32), logprobs_tensors=None)

    runner = types.SimpleNamespace(sampler=sampler, _arctic_maybe_draft_early=lambda *a: None)
    md = types.SimpleNamespace(num_draft_tokens=[2, 1, 0], draft_token_ids=torch.tensor([1, 2, 3], dtype=torch.int32),
                               cu_num_draft_tokens=torch.tensor([2, 3, 3], dtype=torch.int32),
                               target_logits_indices=torch.tensor([0, 1, 3]), bonus_logits_indices=torch.tensor([2, 4, 5]))
    logits = torch.zeros(6, V).as_subclass(OnGpu)
    sample = MR.build_model_runner_patch()._arctic_sample
    greedy = dict(all_greedy=True, temperature=None)
    monkeypatch.delenv("ARCTIC_INFERENCE_HIP_SAMPLER", raising=False)
    monkeypatch.delenv("ARCTIC_INFERENCE_HIP_LOGPROBS", raising=False)
    # switch on, a request with a penalty: vLLM's sampler draws the bonus tokens, the greedy acceptance takes them
    monkeypatch.setenv("ARCTIC_INFERENCE_HIP_LOGITS_EDITS", "1")
    sample(runner, logits, _sm(no_penalties=False, **greedy), md, None)
    (_, a, kw), = rec.calls
    assert sampler_calls == [(3, V)]
    assert a[3] is not None and a[3].flatten().tolist() == [5, 5, 5] and kw.get("bonus_row_index") is None
    assert kw["target_row_index"].tolist() == [0, 1, 3] and "temperature" not in kw
    # switch on, no edits: the one-launch form with its own bonus arg-max, as on the parent commit
    rec.calls.clear(), sampler_calls.clear()
    sample(runner, logits, _sm(**greedy), md, None)
    (_, a, kw), = rec.calls
    assert not sampler_calls and a[3] is None and kw["bonus_row_index"].tolist() == [2, 4, 5]


# ---------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------
def _rows(pair):
    off, tok = pair[0].tolist(), pair[1].tolist()
    return [tok[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_packing_matches_literal_per_request_loops():
    from arcticinference_amd.vllm_plugin import logits_edits as L
    VV = 50
    outputs = [[4, 9, 7], [], [1, 2, 3, 4], [8]]
    sm = _sm(no_penalties=False, output_token_ids=outputs, all_greedy=False,
             temperature=torch.tensor([1.0, -1.0, 0.5, 0.9]), min_p=torch.tensor([0.1, 0.0, 0.0, 0.2]),
             prompt_token_ids=torch.tensor([[5, 6, 7], [1, VV, VV], [VV, VV, VV], [2, 2, VV]]),
             repetition_penalties=torch.tensor([1.1, 1.0, 1.2, 1.0]), frequency_penalties=torch.tensor([0.0, 0.5, 0.0, 0.0]),
             presence_penalties=torch.tensor([0.0, 0.0, -0.5, 0.0]),
             logit_bias=[{3: 1.5, 40: -2.0}, {}, None, {0: 0.25}],
             min_tokens={0: (3, {48, 49}), 2: (5, {49}), 3: (1, {47})},          # reached, not reached, reached
             bad_words_token_ids={0: [[9, 7, 30]],          # prefix 9 7 equals the output's tail: 30 banned
                                  1: [[6, 31]],             # longer than the (empty) output + 1: nothing
                                  2: [[3, 5, 32], [33]],    # prefix 3 5 differs from the tail 3 4: nothing; one token: banned
                                  3: [[8, 34], [7, 35]]},   # 8 matches, 7 does not
             allowed_token_ids_mask=torch.zeros(4, VV, dtype=torch.bool))
    kw = L.pack_edits(sm, 4, "cpu")
    # the literal loops
    want_bans = [[], [], [], []]
    for i, (n, stops) in sm.min_tokens.items():
        if len(outputs[i]) < n:
            want_bans[i] += sorted(stops)
    for i, words in sm.bad_words_token_ids.items():
        for w in words:
            if len(w) == 1 or (len(w) - 1 <= len(outputs[i]) and outputs[i][len(outputs[i]) - (len(w) - 1):] == w[:-1]):
                want_bans[i].append(w[-1])
    assert want_bans == [[30], [], [49, 33], [34]]
    assert [sorted(r) for r in _rows(kw["ban"])] == [sorted(r) for r in want_bans]
    assert L.banned_tokens(sm, 4) == want_bans
    assert _rows(kw["output"]) == outputs                                       # an empty output list stays an empty row
    bias_rows = _rows(kw["bias"])
    assert bias_rows == [[3, 40], [], [], [0]]                                  # an empty dict and None: empty rows
    assert kw["bias"][2].dtype == torch.float32 and kw["bias"][2].tolist() == [1.5, -2.0, 0.25]
    assert _rows(kw["prompt"]) == sm.prompt_token_ids.tolist()                  # the padding VV travels; the kernel ignores it
    for pair in (kw["ban"], kw["bias"], kw["prompt"], kw["output"]):
        assert pair[0].dtype == pair[1].dtype == torch.int32 and pair[0].numel() == 5
    assert torch.equal(kw["repetition"], sm.repetition_penalties) and torch.equal(kw["frequency"], sm.frequency_penalties)
    assert torch.equal(kw["presence"], sm.presence_penalties)
    assert torch.equal(kw["min_p"], sm.min_p) and torch.equal(kw["temperature"], sm.temperature)
    assert kw["allowed_mask"].shape == (4, VV)
    # the oracle ignores the padding and ids outside the row, as the kernel does
    x = torch.zeros(4, VV)
    a = E.edit(x + 1, prompts=_rows(kw["prompt"]), outputs=outputs, repetition=[2.0] * 4)
    assert a[1].tolist() == [1.0, 0.5] + [1.0] * (VV - 2) and a[2].tolist()[:5] == [1.0, 0.5, 0.5, 0.5, 0.5]


def test_packing_leaves_out_what_nobody_uses():
    from arcticinference_amd.vllm_plugin import logits_edits as L
    assert L.pack_edits(_sm(), 3, "cpu") == {}
    # min_tokens reached everywhere and an empty bias dict: no ban list, no bias list
    kw = L.pack_edits(_sm(min_tokens={0: (1, {4})}, output_token_ids=[[9], [], []], logit_bias=[{}, None, None]), 3, "cpu")
    assert kw == {}
    # min-p touches no greedy row: an all-greedy batch carries none
    kw = L.pack_edits(_sm(min_p=torch.tensor([0.1, 0.1, 0.1]), all_greedy=True, temperature=None), 3, "cpu")
    assert kw == {}
    kw = L.pack_edits(_sm(min_p=torch.tensor([0.1, 0.0, 0.1])), 3, "cpu")
    assert set(kw) == {"min_p", "temperature"}
    # penalties without a prompt matrix: outputs and the three tensors only
    kw = L.pack_edits(_sm(no_penalties=False, frequency_penalties=torch.tensor([0.5, 0.0, 0.0])), 3, "cpu")
    assert set(kw) == {"output", "frequency"} and kw["output"][0].tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------
# the oracle, by hand
# ---------------------------------------------------------------------------------------------------
def test_oracle_on_a_hand_computed_case():
    inf = float("inf")
    logits = torch.tensor([[2.0, -1.0, 0.0, 4.0, -inf, 1.0, -2.0, 3.0],
                           [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]], dtype=torch.bfloat16)
    mask = torch.zeros(2, 8, dtype=torch.bool)
    mask[0, 7] = True
    got = E.edit(logits, allowed_mask=mask, bans=[[5], []], bias=[{1: 0.5, 4: 1.0}, {}], prompts=[[3, 8], []],
                 outputs=[[0, 0, 6], [7]], repetition=[2.0, 0.5], frequency=[0.5, -1.0], presence=[0.25, 0.0])
    # row 0: 7 masked, 5 banned, 1 biased to -0.5 (-inf + 1 stays -inf); seen = {3 (prompt), 0, 6}: 2 / 2 = 1, 4 / 2 = 2,
    # -2 * 2 = -4; frequency 0.5: token 0 (twice) 1 - 1 = 0, token 6 (once) -4.5; presence 0.25: -0.25 and -4.75
    # row 1: token 7 seen: 8 / 0.5 = 16, minus -1 * 1: 17
    want = torch.tensor([[-0.25, -0.5, 0.0, 2.0, -inf, -inf, -4.75, -inf], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 17.0]])
    assert got.dtype == torch.float32 and torch.equal(got, want)
    # min-p: row 0 keeps x >= 2 + ln 0.5 = 1.307 (token 3 only); row 1, T = 2: x >= 17 + 2 ln 0.1 = 12.39 (token 7 only)
    kept = E.apply_min_p(got, [0.5, 0.1], [1.0, 2.0])
    assert kept[0].tolist() == [-inf, -inf, -inf, 2.0, -inf, -inf, -inf, -inf]
    assert kept[1].tolist() == [-inf] * 7 + [17.0]
    d = E.min_p_distance(got, [0.5, 0.1], [1.0, 2.0])
    assert ((d >= 0) == (kept != -inf).numpy()).all()
    assert abs(d[0, 3] - np.log(2.0)) < 1e-12 and abs(d[1, 6] - (-5.0 - np.log(float(np.float32(0.1))))) < 1e-12   # min_p is an f32
    # T <= 0 and min_p == 0: untouched
    assert torch.equal(E.apply_min_p(got, [0.5, 0.0], [-1.0, 2.0]), got)


@pytest.mark.parametrize("shape", E.shapes(E.segment_size()))
def test_min_p_fixtures_keep_every_token_clear_of_the_threshold(shape):
    """A condition on the fixtures, not a tolerance: the f32 evaluation of (x - m) / T is off by a few 1e-6 at these
    magnitudes, so with no token within 1e-3 of the threshold the kept set is unambiguous."""
    S = E.segment_size()
    fx = E.build_fixture(*shape, S)
    for case in ("min_p", "all"):
        x = E.edit(fx.logits, **fx.oracle_kwargs(case))
        d = E.min_p_distance(x, fx.min_p, fx.temperature)
        assert np.abs(d).min() >= E.MIN_P_MARGIN, (case, float(np.abs(d).min()))
        kept = E.apply_min_p(x, fx.min_p, fx.temperature)
        for r in range(fx.rows):
            if fx.temperature[r] > 0 and fx.min_p[r] > 0:
                assert ((kept[r] != float("-inf")).numpy() == (d[r] >= 0)).all()      # the f32 form agrees with the f64 one
                assert 1 <= int((d[r] >= 0).sum()) < fx.V                              # min-p keeps some, drops some
            else:
                assert torch.equal(kept[r], x[r])
    # the planted values survive the margin pass, and the logits are exact in the 16-bit types
    assert fx.moved < fx.rows * fx.V // 20
    assert torch.equal(fx.logits.to(torch.bfloat16).float(), fx.logits) and torch.equal(fx.logits.half().float(), fx.logits)
    assert fx.outputs[0].count(7) == E.REPEATS > 255
    assert float(fx.logits[0, 3]) == float("-inf") and float(fx.logits[0, 2]) == 0.0


# ---------------------------------------------------------------------------------------------------
# ops.edit_logits: refusals before any launch (no device needed: the checks come first)
# ---------------------------------------------------------------------------------------------------
def test_edit_logits_refuses_wrong_arguments_before_any_launch():
    from arcticinference_amd import ops
    lg = torch.zeros(3, V, dtype=torch.bfloat16)
    off = torch.zeros(4, dtype=torch.int32)
    tok = torch.zeros(0, dtype=torch.int32)
    f = torch.zeros(3)
    bad = [dict(logits=torch.zeros(3, V, dtype=torch.float64)), dict(logits=torch.zeros(V)),
           dict(row_index=torch.zeros(2, dtype=torch.int32)),
           dict(allowed_mask=torch.zeros(3, V, dtype=torch.int32)), dict(allowed_mask=torch.zeros(2, V, dtype=torch.bool)),
           dict(ban=(off.long(), tok)), dict(ban=(off[:3], tok)), dict(ban=(off, tok.long())), dict(ban=(off,)),
           dict(bias=(off, tok)), dict(bias=(off, tok, torch.zeros(0, dtype=torch.float64))),
           dict(bias=(off, tok, torch.zeros(2))), dict(prompt=(off, tok, tok)), dict(output=(off.float(), tok)),
           dict(repetition=f.double()), dict(frequency=torch.zeros(2)), dict(presence=torch.zeros(3, 1)),
           dict(min_p=f), dict(min_p=f, temperature=f.half())]
    for kw in bad:
        args = dict(kw)
        with pytest.raises(ValueError):
            ops.edit_logits(args.pop("logits", lg), **args)
    # well-formed arguments on the CPU: refused as every op is, there is no CPU fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.edit_logits(lg, ban=(off, tok), min_p=f, temperature=f)
