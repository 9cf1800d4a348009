"""GPU: verify steps whose sampling carries top-k / top-p on the plugin's HIP acceptance route
(ARCTIC_INFERENCE_HIP_TOP_K_TOP_P=1, aic_rejection_random_topk_topp), driven through the stand-in for vLLM 0.9.2.
The stand-in InputBatch does not fill top_k / top_p; the test sets them as vLLM's _make_sampling_metadata would."""
import numpy as np
import pytest
import torch

import sampling_oracle as S
import vllm_harness as H
from test_vllm_plugin_gpu import DEV, SoftSteered, _requests, _vllm_config

pytestmark = pytest.mark.gpu
ENV = "ARCTIC_INFERENCE_HIP_TOP_K_TOP_P"
# r0 / r3 greedy (their filters are ignored, as vLLM's arg-max of the filtered row does with a unique maximum);
# r1 top-k 3 + top-p 0.95 at T = 1; r2 top-p 0.5 at T = 0.7 (only the stream's token survives)
TEMPS = {"r0": None, "r1": (1.0, 101), "r2": (0.7, 102), "r3": None}
TOP_K = {"r0": 5, "r1": 3, "r2": 0, "r3": 0}
TOP_P = {"r0": 0.8, "r1": 0.95, "r2": 0.5, "r3": 1.0}


def _runner():
    H.load_plugin()
    from vllm.config import SpeculativeConfig, set_current_vllm_config
    from vllm.v1.worker.gpu_model_runner import GPUModelRunner
    spec = SpeculativeConfig(method="suffix")
    spec.proposal_indexing = "single_advance"
    cfg = _vllm_config(spec)
    H.init_single_process_groups(cfg)
    runner = GPUModelRunner(cfg, torch.device(DEV))
    set_current_vllm_config(cfg)
    runner.load_model()
    runner.initialize_kv_cache((200, torch.bfloat16))
    return runner


def _drive(runner, monkeypatch, steps, check):
    from vllm.v1.sample.rejection_sampler import RejectionSampler
    from vllm.v1.worker.gpu_model_runner import Sampler
    B, PL, V = 4, 96, 2000
    streams = _requests(B, PL, seed=6)
    sched = H.MiniScheduler(16, 400)
    for rid, s in streams.items():
        sched.add(rid, [int(x) for x in s[:PL]], *(TEMPS[rid] or ()))
    steer = SoftSteered(runner, sched, streams)
    ids0 = list(streams)
    runner.input_batch.extra_sampling = dict(
        top_k=torch.tensor([TOP_K[r] for r in ids0], dtype=torch.int32, device=DEV),
        top_p=torch.tensor([TOP_P[r] for r in ids0], dtype=torch.float32, device=DEV))
    early = []
    orig = runner._arctic_maybe_draft_early
    monkeypatch.setattr(runner, "_arctic_maybe_draft_early", lambda *a: (early.append(1), orig(*a))[1])
    twins = {rid: torch.Generator(device=DEV).manual_seed(t[1]) for rid, t in TEMPS.items() if t}
    RejectionSampler.calls = Sampler.calls = 0
    stats = dict(verify=0, accepted=0, recovered=0)
    for step in range(steps):
        so = sched.schedule()
        steer.plan(so)
        out = runner.execute_model(so)
        ids = list(out.req_ids)
        assert ids == ids0
        n = [len(so.scheduled_spec_decode_tokens.get(rid, ())) for rid in ids]
        lg = steer.logits
        temp = [TEMPS[rid][0] if TEMPS[rid] else -1.0 for rid in ids]
        bonus_rows = np.cumsum(np.asarray(n) + 1) - 1
        bonus = []
        for i, rid in enumerate(ids):      # the stand-in sampler on the bonus rows (vLLM's sampler keeps them)
            row = lg[bonus_rows[i]].float()
            if TEMPS[rid] is None:
                bonus.append(int(row.argmax()))
            else:
                q = torch.empty(V, dtype=torch.float32, device=DEV).exponential_(generator=twins[rid])
                bonus.append(int((torch.softmax(row / temp[i], dim=-1) / q).argmax()))
        if sum(n) == 0:
            want = [[b] for b in bonus]
        else:
            stats["verify"] += 1
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
            mat = S.rejection_topk_topp(target, drafts, n, bonus, max(n), temp, u, noise,
                                        [TOP_K[r] for r in ids], [TOP_P[r] for r in ids])
            want = [[int(t) for t in row if t != -1] for row in mat]
            for i, rid in enumerate(ids):
                if rid in twins and n[i]:
                    acc = sum(1 for p in range(min(n[i], len(want[i]))) if want[i][p] == so.scheduled_spec_decode_tokens[rid][p])
                    stats["accepted"] += acc
                    stats["recovered"] += acc < n[i]
        emitted = sched.update(out)
        if check:
            assert [emitted[rid] for rid in ids] == want, (step, emitted, want)
    return stats, early, RejectionSampler.calls


def test_top_k_top_p_batches_are_accepted_by_the_hip_kernel_with_the_switch_on(stub_vllm, monkeypatch):
    monkeypatch.setenv(ENV, "1")
    stats, early, rs_calls = _drive(_runner(), monkeypatch, 40, check=True)
    assert stats["verify"] > 10 and stats["accepted"] > 5 and stats["recovered"] > 3, stats
    assert rs_calls == 0, "a top-k / top-p batch reached vLLM's RejectionSampler"
    assert len(early) == stats["verify"]          # every verify step took the early-draft path behind the kernel


def test_top_k_top_p_batches_keep_vllms_rejection_sampler_with_the_switch_off(stub_vllm, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    stats, early, rs_calls = _drive(_runner(), monkeypatch, 12, check=False)
    assert stats["verify"] > 0 and rs_calls == stats["verify"] and not early
