"""GPU: the plugin's HIP sampler route (ARCTIC_INFERENCE_HIP_SAMPLER=1, aic_sample_topk_topp) through the stand-in for
vLLM 0.9.2: bonus tokens of verify steps and whole steps without draft tokens, next to the top-k / top-p acceptance
switch (ARCTIC_INFERENCE_HIP_TOP_K_TOP_P).  The stand-in InputBatch does not fill top_k / top_p; the tests set them as
vLLM's _make_sampling_metadata would."""
import numpy as np
import pytest
import torch

import sampler_oracle as O
import sampling_oracle as S
import vllm_harness as H
from test_vllm_plugin_gpu import DEV, SoftSteered, _requests
from test_vllm_topk_topp_route_gpu import TEMPS, TOP_K, TOP_P, _runner

pytestmark = pytest.mark.gpu
SAMPLER_ENV = "ARCTIC_INFERENCE_HIP_SAMPLER"
FILTER_ENV = "ARCTIC_INFERENCE_HIP_TOP_K_TOP_P"


def _drive(runner, monkeypatch, steps, filters, check):
    """Drives `steps` steps of two seeded sampling requests beside two greedy ones.  With `check`, every step's tokens
    are compared with the oracle replay for the route with BOTH the sampler and the acceptance on HIP: twin generators
    consumed in vLLM's order (sampler noise, then uniforms, then recovery noise), the bonus tokens and the tokens of
    draft-free steps sampled with the filters."""
    from arcticinference_amd import ops
    from vllm.v1.sample.rejection_sampler import RejectionSampler
    from vllm.v1.worker.gpu_model_runner import Sampler
    B, PL, V = 4, 96, 2000
    streams = _requests(B, PL, seed=6)
    sched = H.MiniScheduler(16, 400)
    for rid, s in streams.items():
        sched.add(rid, [int(x) for x in s[:PL]], *(TEMPS[rid] or ()))
    steer = SoftSteered(runner, sched, streams)
    ids0 = list(streams)
    if filters:
        runner.input_batch.extra_sampling = dict(
            top_k=torch.tensor([TOP_K[r] for r in ids0], dtype=torch.int32, device=DEV),
            top_p=torch.tensor([TOP_P[r] for r in ids0], dtype=torch.float32, device=DEV))
    early, hip_calls = [], []
    orig = runner._arctic_maybe_draft_early
    monkeypatch.setattr(runner, "_arctic_maybe_draft_early", lambda *a: (early.append(1), orig(*a))[1])
    orig_sample = ops.sample_tokens
    monkeypatch.setattr(ops, "sample_tokens", lambda *a, **kw: (hip_calls.append(1), orig_sample(*a, **kw))[1])
    twins = {rid: torch.Generator(device=DEV).manual_seed(t[1]) for rid, t in TEMPS.items() if t}
    RejectionSampler.calls = Sampler.calls = 0
    stats = dict(verify=0, draft_free=0, skipped=0, bonus_emitted=0)
    for step in range(steps):
        so = sched.schedule()
        steer.plan(so)
        out = runner.execute_model(so)
        ids = list(out.req_ids)
        assert ids == ids0
        n = [len(so.scheduled_spec_decode_tokens.get(rid, ())) for rid in ids]
        stats["verify" if sum(n) else "draft_free"] += 1
        emitted = sched.update(out)
        if not check:
            continue
        lg = steer.logits
        temp = [TEMPS[rid][0] if TEMPS[rid] else -1.0 for rid in ids]
        ks = [TOP_K[r] for r in ids] if filters else None
        ps = [TOP_P[r] for r in ids] if filters else None
        bonus_rows = np.cumsum(np.asarray(n) + 1) - 1
        # the sampler: one Exp(1) row per request, seeded requests from their generator (the greedy rows' noise is unused)
        q = torch.ones(len(ids), V)
        for i, rid in enumerate(ids):
            if rid in twins:
                q[i] = torch.empty(V, dtype=torch.float32, device=DEV).exponential_(generator=twins[rid]).cpu()
        blg = lg[torch.from_numpy(bonus_rows).to(DEV)].cpu()
        bonus = O.sample_literal(blg, temp, ks, ps, q).tolist()
        _, lead = O.sample_f64(blg, temp, ks, ps, q)
        if sum(n) == 0:
            want = [[b] for b in bonus]
        else:
            u = np.zeros(sum(n))
            noise = torch.ones(len(ids), V)
            at = 0
            for i, rid in enumerate(ids):
                if n[i] and rid in twins:
                    u[at:at + n[i]] = torch.empty(n[i], dtype=torch.float64, device=DEV).uniform_(generator=twins[rid]).cpu().numpy()
                at += n[i]
            for i, rid in enumerate(ids):
                if n[i] and rid in twins:
                    noise[i] = torch.empty(V, dtype=torch.float32, device=DEV).exponential_(generator=twins[rid]).cpu()
            is_bonus = np.zeros(lg.shape[0], dtype=bool)
            is_bonus[bonus_rows] = True
            target = lg[torch.from_numpy(np.nonzero(~is_bonus)[0]).to(DEV)].cpu()
            drafts = [t for rid in ids for t in so.scheduled_spec_decode_tokens.get(rid, ())]
            mat = S.rejection_topk_topp(target, drafts, n, bonus, max(n), temp, u, noise, ks, ps)
            want = [[int(t) for t in row if t != -1] for row in mat]
            stats["bonus_emitted"] += sum(1 for i, rid in enumerate(ids) if rid in twins and len(want[i]) == n[i] + 1)
        if lead < O.WINNER_MARGIN:
            stats["skipped"] += 1
            continue
        assert [emitted[rid] for rid in ids] == want, (step, emitted, want)
    print(f"steps skipped for a winner margin under {O.WINNER_MARGIN}: {stats['skipped']} of {steps}")
    return stats, len(early), RejectionSampler.calls, Sampler.calls, len(hip_calls)


def test_both_switches_on_sampler_and_acceptance_run_on_hip(stub_vllm, monkeypatch):
    monkeypatch.setenv(SAMPLER_ENV, "1")
    monkeypatch.setenv(FILTER_ENV, "1")
    stats, early, rs_calls, sampler_calls, hip_calls = _drive(_runner(), monkeypatch, 40, filters=True, check=True)
    assert sampler_calls == 0, "a step reached vLLM's Sampler"
    assert rs_calls == 0, "a step reached vLLM's RejectionSampler"
    assert stats["draft_free"] >= 1 and stats["verify"] > 10, stats
    assert stats["bonus_emitted"] > 3, stats                  # sampled bonus tokens reached the output
    assert stats["skipped"] <= 1, stats
    assert hip_calls == 40                                    # one sampler call per step, none twice
    assert early == stats["verify"]                           # the early draft-model hook still fires on every verify step


def test_sampler_switch_alone_serves_temperature_only_batches(stub_vllm, monkeypatch):
    monkeypatch.setenv(SAMPLER_ENV, "1")
    monkeypatch.delenv(FILTER_ENV, raising=False)
    stats, early, rs_calls, sampler_calls, hip_calls = _drive(_runner(), monkeypatch, 24, filters=False, check=True)
    assert sampler_calls == 0 and rs_calls == 0
    assert stats["verify"] > 5 and stats["skipped"] <= 1 and hip_calls == 24 and early == stats["verify"], stats


def test_sampler_switch_alone_leaves_filtered_verify_steps_to_vllm(stub_vllm, monkeypatch):
    monkeypatch.setenv(SAMPLER_ENV, "1")
    monkeypatch.delenv(FILTER_ENV, raising=False)
    stats, early, rs_calls, sampler_calls, hip_calls = _drive(_runner(), monkeypatch, 12, filters=True, check=False)
    assert stats["verify"] > 0
    # verify steps: vLLM's sampler (bonus tokens, sampled once: no HIP sampler call beside it) + RejectionSampler
    assert sampler_calls == stats["verify"] and rs_calls == stats["verify"] and not early
    assert hip_calls == stats["draft_free"]                   # steps without draft tokens are still sampled in HIP


@pytest.mark.parametrize("filters", [False, True])
def test_both_switches_off_is_the_parent_behaviour(stub_vllm, monkeypatch, filters):
    monkeypatch.delenv(SAMPLER_ENV, raising=False)
    monkeypatch.delenv(FILTER_ENV, raising=False)
    steps = 12
    stats, early, rs_calls, sampler_calls, hip_calls = _drive(_runner(), monkeypatch, steps, filters=filters, check=False)
    assert hip_calls == 0
    assert sampler_calls == steps                             # the batch is never all-greedy
    # temperature-only batches take aic_rejection_random; filtered ones vLLM's RejectionSampler, as on the parent commit
    assert rs_calls == (stats["verify"] if filters else 0)
    assert early == (0 if filters else stats["verify"])
