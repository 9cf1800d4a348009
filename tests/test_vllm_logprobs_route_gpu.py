"""GPU: steps that report logprobs on the plugin's HIP routes (ARCTIC_INFERENCE_HIP_LOGPROBS=1, aic_token_logprobs)
through the stand-in for vLLM 0.9.2.  The stand-in's vllm.v1.outputs has no LogprobsTensors: the tests plant the
three-field NamedTuple of tests/logprobs_oracle.py there.  The stand-in InputBatch does not fill max_num_logprobs (nor
top_k / top_p); the tests set them as vLLM's _make_sampling_metadata would."""
import numpy as np
import pytest
import torch

import logprobs_oracle as LO
import vllm_harness as H
from test_vllm_plugin_gpu import DEV, SoftSteered, _requests
from test_vllm_sampler_route_gpu import FILTER_ENV, SAMPLER_ENV, _drive
from test_vllm_topk_topp_route_gpu import TEMPS, _runner

pytestmark = pytest.mark.gpu
LOGPROBS_ENV = "ARCTIC_INFERENCE_HIP_LOGPROBS"
N_LOGPROBS = 3
GREEDY = {rid: None for rid in TEMPS}


def _plant(monkeypatch):
    import vllm.v1.outputs
    monkeypatch.setattr(vllm.v1.outputs, "LogprobsTensors", LO.LogprobsTensors, raising=False)


def _spy(monkeypatch):
    """Records every ops.token_logprobs and ops.rejection_sample call's keyword arguments."""
    from arcticinference_amd import ops
    calls = dict(logprobs=[], accept=[])
    orig_lp, orig_rej = ops.token_logprobs, ops.rejection_sample
    monkeypatch.setattr(ops, "token_logprobs", lambda *a, **kw: (calls["logprobs"].append(kw), orig_lp(*a, **kw))[1])
    monkeypatch.setattr(ops, "rejection_sample", lambda *a, **kw: (calls["accept"].append(kw), orig_rej(*a, **kw))[1])
    return calls


def _record_steps(runner, monkeypatch, num_logprobs, temps=TEMPS):
    """Wraps execute_model: sets max_num_logprobs for the step's metadata, and checks the step's logprobs lists against
    the f64 oracle on the sampler call's rows (the bonus rows of a verify step, every row of a draft-free step)."""
    seen = dict(verify=0, draft_free=0, with_lists=0, bonus_emitted=0, worst=0.0)
    orig = runner.execute_model

    def execute(so):
        runner.input_batch.extra_sampling["max_num_logprobs"] = num_logprobs
        out = orig(so)
        ids = list(out.req_ids)
        n = [len(so.scheduled_spec_decode_tokens.get(rid, ())) for rid in ids]
        seen["verify" if sum(n) else "draft_free"] += 1
        if out.logprobs is None:
            return out
        seen["with_lists"] += 1
        lists = out.logprobs
        lg = runner.model.logit_hook.logits
        bonus_rows = np.cumsum(np.asarray(n) + 1) - 1
        blg = lg[torch.from_numpy(bonus_rows).to(DEV)].cpu()
        col0 = [row[0] for row in lists.logprob_token_ids]
        for i, rid in enumerate(ids):
            if temps[rid] is None:                                  # greedy requests: the bonus token is the arg-max
                assert col0[i] == int(blg[i].float().argmax())
            if len(out.sampled_token_ids[i]) == n[i] + 1:           # the sampler's token was emitted
                assert col0[i] == out.sampled_token_ids[i][-1]
                seen["bonus_emitted"] += 1
        want_ids, want_lp, want_rank = LO.f64_oracle(blg, col0, num_logprobs)
        assert lists.logprob_token_ids == want_ids.tolist(), (lists.logprob_token_ids, want_ids.tolist())
        assert lists.sampled_token_ranks == want_rank.tolist()
        got = np.asarray(lists.logprobs, dtype=np.float64)
        seen["worst"] = max(seen["worst"], LO.max_excess(got, want_lp))
        assert LO.within_bar(got, want_lp).all(), LO.max_excess(got, want_lp)
        return out

    monkeypatch.setattr(runner, "execute_model", execute)
    return seen


def _drive_plain(runner, monkeypatch, steps, temps):
    """`steps` steps of the four requests with `temps`; returns (verify steps, early-draft calls, RejectionSampler calls,
    Sampler calls)."""
    from vllm.v1.sample.rejection_sampler import RejectionSampler
    from vllm.v1.worker.gpu_model_runner import Sampler
    B, PL = 4, 96
    streams = _requests(B, PL, seed=6)
    sched = H.MiniScheduler(16, 400)
    for rid, s in streams.items():
        sched.add(rid, [int(x) for x in s[:PL]], *(temps[rid] or ()))
    steer = SoftSteered(runner, sched, streams)
    early = []
    orig = runner._arctic_maybe_draft_early
    monkeypatch.setattr(runner, "_arctic_maybe_draft_early", lambda *a: (early.append(1), orig(*a))[1])
    RejectionSampler.calls = Sampler.calls = 0
    verify = 0
    outs = []
    for _ in range(steps):
        so = sched.schedule()
        steer.plan(so)
        out = runner.execute_model(so)
        verify += bool(so.scheduled_spec_decode_tokens)
        outs.append(out)
        sched.update(out)
    return verify, len(early), RejectionSampler.calls, Sampler.calls, outs


def test_all_switches_on_tokens_and_logprobs_come_from_hip(stub_vllm, monkeypatch):
    _plant(monkeypatch)
    for env in (LOGPROBS_ENV, SAMPLER_ENV, FILTER_ENV):
        monkeypatch.setenv(env, "1")
    runner = _runner()
    calls = _spy(monkeypatch)
    seen = _record_steps(runner, monkeypatch, N_LOGPROBS)
    steps = 24
    # the existing driver: emitted tokens equal the twin-generator replay, skipped steps counted
    stats, early, rs_calls, sampler_calls, hip_calls = _drive(runner, monkeypatch, steps, filters=True, check=True)
    print(f"largest logprob error / bar over {seen['with_lists']} steps: {seen['worst']:.3f}")
    assert sampler_calls == 0, "a step reached vLLM's Sampler"
    assert rs_calls == 0, "a step reached vLLM's RejectionSampler"
    assert stats["skipped"] <= 1, stats
    assert stats["verify"] > 5 and stats["draft_free"] >= 1, stats
    assert hip_calls == steps and early == stats["verify"]
    assert seen["with_lists"] == steps and seen["bonus_emitted"] > 4 * stats["draft_free"]
    assert len(calls["logprobs"]) == steps
    assert all(kw["token_ids"] is not None for kw in calls["logprobs"])
    # verify steps read the bonus rows in place; draft-free steps every row
    assert sum(kw.get("row_index") is not None for kw in calls["logprobs"]) == stats["verify"]


def test_logprobs_switch_alone_keeps_the_one_launch_greedy_acceptance(stub_vllm, monkeypatch):
    _plant(monkeypatch)
    monkeypatch.setenv(LOGPROBS_ENV, "1")
    monkeypatch.delenv(SAMPLER_ENV, raising=False)
    monkeypatch.delenv(FILTER_ENV, raising=False)
    runner = _runner()
    calls = _spy(monkeypatch)
    seen = _record_steps(runner, monkeypatch, N_LOGPROBS, temps=GREEDY)
    runner.input_batch.extra_sampling = {}
    steps = 14
    verify, early, rs_calls, sampler_calls, outs = _drive_plain(runner, monkeypatch, steps, GREEDY)
    assert verify > 5 and early == verify
    assert rs_calls == 0 and sampler_calls == steps - verify            # vLLM's classes: draft-free steps only
    assert len(calls["accept"]) == verify and all(kw.get("bonus_row_index") is not None for kw in calls["accept"])
    assert len(calls["logprobs"]) == verify
    assert all(kw["token_ids"] is None and kw["row_index"] is not None for kw in calls["logprobs"])
    assert seen["with_lists"] == verify                                 # the stand-in's sampler reports none


def test_logprobs_switch_alone_random_batches_pass_the_samplers_tensors_through(stub_vllm, monkeypatch):
    _plant(monkeypatch)
    monkeypatch.setenv(LOGPROBS_ENV, "1")
    monkeypatch.delenv(SAMPLER_ENV, raising=False)
    monkeypatch.delenv(FILTER_ENV, raising=False)
    runner = _runner()
    calls = _spy(monkeypatch)
    seen = _record_steps(runner, monkeypatch, N_LOGPROBS)
    runner.input_batch.extra_sampling = {}
    steps = 14
    verify, early, rs_calls, sampler_calls, outs = _drive_plain(runner, monkeypatch, steps, TEMPS)
    assert verify > 5 and early == verify
    assert rs_calls == 0 and len(calls["accept"]) == verify             # the acceptance stays on HIP
    assert sampler_calls == steps                                       # vLLM's sampler draws every bonus token
    assert not calls["logprobs"]
    assert seen["with_lists"] == 0 and all(o.logprobs is None for o in outs)    # the stand-in returns None: passed through


@pytest.mark.parametrize("switch,num_logprobs", [("0", N_LOGPROBS), ("1", LO.CAP + 1)])
def test_switch_off_or_above_the_cap_is_the_parent_behaviour(stub_vllm, monkeypatch, switch, num_logprobs):
    _plant(monkeypatch)
    monkeypatch.setenv(LOGPROBS_ENV, switch)
    monkeypatch.setenv(SAMPLER_ENV, "1")
    monkeypatch.setenv(FILTER_ENV, "1")
    runner = _runner()
    calls = _spy(monkeypatch)
    seen = _record_steps(runner, monkeypatch, num_logprobs)
    runner.input_batch.extra_sampling = {}
    steps = 12
    verify, early, rs_calls, sampler_calls, outs = _drive_plain(runner, monkeypatch, steps, TEMPS)
    assert verify > 3
    assert sampler_calls == steps and rs_calls == verify and early == 0     # both of vLLM's classes, every step
    assert not calls["logprobs"] and not calls["accept"]
    assert seen["with_lists"] == 0
