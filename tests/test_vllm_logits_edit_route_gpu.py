"""GPU: steps whose requests edit their logits (penalties, min_tokens, min-p, logit bias) on the plugin's HIP routes
(ARCTIC_INFERENCE_HIP_LOGITS_EDITS=1, aic_logits_edit) through the stand-in for vLLM 0.9.2.  The stand-in InputBatch
fills none of the edit fields and its Sampler applies no edits: the tests set the fields as vLLM's
_make_sampling_metadata would (output_token_ids before every step), and the expected tokens come from
tests/logits_edit_oracle.py + tests/sampler_oracle.py, never from the stand-in.

Of the four requests, r1 carries repetition / frequency / presence penalties and min_tokens (its stop id is the most
frequent token of its own stream, so the ban shows), r2 carries min-p and a logit bias that lifts one token between the
two planted logits; r0 and r3 carry nothing."""
import collections

import numpy as np
import pytest
import torch

import logits_edit_oracle as E
import logprobs_oracle as LO
import sampler_oracle as O
import sampling_oracle as S
import vllm_harness as H
from test_vllm_plugin_gpu import DEV, SoftSteered, _requests
from test_vllm_sampler_route_gpu import FILTER_ENV, SAMPLER_ENV
from test_vllm_sampler_route_gpu import _drive as _drive_without_edits
from test_vllm_topk_topp_route_gpu import TEMPS, TOP_K, TOP_P, _runner

pytestmark = pytest.mark.gpu
EDITS_ENV = "ARCTIC_INFERENCE_HIP_LOGITS_EDITS"
LOGPROBS_ENV = "ARCTIC_INFERENCE_HIP_LOGPROBS"
GREEDY = {rid: None for rid in TEMPS}
B, PL, V = 4, 96, 2000
REPETITION, FREQUENCY, PRESENCE = [1.0, 1.3, 1.0, 1.0], [0.0, 0.4, 0.0, 0.0], [0.0, 0.2, 0.0, 0.0]
MIN_P = [0.0, 0.0, 0.2, 0.0]
BIAS = [None, None, {1234: 8.5}, None]
MIN_TOKENS = 1000          # never reached in these runs: r1's stop id stays banned
N_LOGPROBS = 3
# Steps whose fixtures miss a margin (sampler winner 1e-4, top-p cumulative sum 5e-3, min-p threshold 1e-3) are not
# compared; the bound keeps the comparison on at least three quarters of the steps.
MAX_SKIPPED_FRACTION = 0.25


def _spy(monkeypatch):
    from arcticinference_amd import ops
    calls = collections.defaultdict(list)
    for name in ("edit_logits", "sample_tokens", "rejection_sample", "token_logprobs"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **kw: (calls[_n].append((a, kw)), _o(*a, **kw))[1])
    return calls


def _drive(runner, monkeypatch, steps, temps, filters, check, num_logprobs=None):
    """`steps` steps of the four requests with the edit fields set.  With `check`, every step's tokens are compared with
    the replay for the route with edits, sampler and acceptance on HIP: twin generators consumed in vLLM's order (sampler
    noise, uniforms, recovery noise), the sampler's rows (bonus rows, or every row of a draft-free step) edited by the
    oracle, the acceptance on the RAW target rows; and the step's logprobs, when asked for, with the f64 oracle on the
    RAW sampler rows."""
    from vllm.v1.sample.rejection_sampler import RejectionSampler
    from vllm.v1.worker.gpu_model_runner import Sampler
    streams = _requests(B, PL, seed=6)
    sched = H.MiniScheduler(16, 400)
    for rid, s in streams.items():
        sched.add(rid, [int(x) for x in s[:PL]], *(temps[rid] or ()))
    steer = SoftSteered(runner, sched, streams)
    ids0 = list(streams)
    stop = collections.Counter(int(x) for x in streams["r1"][PL:PL + 80]).most_common(1)[0][0]
    prompts = [[int(x) for x in streams[r][:PL]] + [V] * 3 for r in ids0]          # padded with the vocabulary size
    extra = dict(no_penalties=False, prompt_token_ids=torch.tensor(prompts, dtype=torch.int64, device=DEV),
                 repetition_penalties=torch.tensor(REPETITION, device=DEV),
                 frequency_penalties=torch.tensor(FREQUENCY, device=DEV),
                 presence_penalties=torch.tensor(PRESENCE, device=DEV), min_tokens={1: (MIN_TOKENS, {stop})},
                 min_p=torch.tensor(MIN_P, device=DEV), logit_bias=list(BIAS), max_num_logprobs=num_logprobs)
    if filters:
        extra.update(top_k=torch.tensor([TOP_K[r] for r in ids0], dtype=torch.int32, device=DEV),
                     top_p=torch.tensor([TOP_P[r] for r in ids0], dtype=torch.float32, device=DEV))
    runner.input_batch.extra_sampling = extra
    early = []
    orig = runner._arctic_maybe_draft_early
    monkeypatch.setattr(runner, "_arctic_maybe_draft_early", lambda *a: (early.append(1), orig(*a))[1])
    twins = {rid: torch.Generator(device=DEV).manual_seed(t[1]) for rid, t in temps.items() if t}
    all_greedy = not twins
    RejectionSampler.calls = Sampler.calls = 0
    stats = dict(verify=0, draft_free=0, skipped=0, bonus_emitted=0, edits_showed=0, logprob_steps=0, early=early)
    for step in range(steps):
        outputs = [list(sched.reqs[rid]["out"]) for rid in ids0]
        extra["output_token_ids"] = [list(o) for o in outputs]
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
        temp = [temps[rid][0] if temps[rid] else -1.0 for rid in ids]
        ks = [TOP_K[r] for r in ids] if filters else None
        ps = [TOP_P[r] for r in ids] if filters else None
        bonus_rows = np.cumsum(np.asarray(n) + 1) - 1
        q = torch.ones(B, V)
        for i, rid in enumerate(ids):
            if rid in twins:
                q[i] = torch.empty(V, dtype=torch.float32, device=DEV).exponential_(generator=twins[rid]).cpu()
        raw = lg[torch.from_numpy(bonus_rows).to(DEV)].cpu()
        bans = [[], [stop] if len(outputs[1]) < MIN_TOKENS else [], [], []]
        edited = E.edit(raw, bans=bans, bias=BIAS, prompts=prompts, outputs=outputs, repetition=REPETITION,
                        frequency=FREQUENCY, presence=PRESENCE)
        clear = True
        if not all_greedy:                                  # min-p touches no greedy row
            clear = float(np.abs(E.min_p_distance(edited, MIN_P, temp)).min()) >= E.MIN_P_MARGIN
            edited = E.apply_min_p(edited, MIN_P, temp)
        bonus = O.sample_literal(edited, temp, ks, ps, q).tolist()
        plain = O.sample_literal(raw, temp, ks, ps, q).tolist()
        _, lead = O.sample_f64(edited, temp, ks, ps, q)
        clear = clear and lead >= O.WINNER_MARGIN
        if filters:
            clear = clear and all(temp[i] <= 0 or O.cumsums_clear(O.scaled_f32(edited[i], temp[i]), ks[i] or V, ps[i])
                                  for i in range(B))
        if sum(n) == 0:
            want = [[b] for b in bonus]
        else:
            u = np.zeros(sum(n))
            noise = torch.ones(B, V)
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
            target = lg[torch.from_numpy(np.nonzero(~is_bonus)[0]).to(DEV)].cpu()       # the RAW target rows
            drafts = [t for rid in ids for t in so.scheduled_spec_decode_tokens.get(rid, ())]
            mat = S.rejection_topk_topp(target, drafts, n, bonus, max(n), temp, u, noise, ks, ps)
            want = [[int(t) for t in row if t != -1] for row in mat]
        if not clear:
            stats["skipped"] += 1
            continue
        assert [emitted[rid] for rid in ids] == want, (step, emitted, want)
        for i in range(B):
            if len(want[i]) == n[i] + 1:
                stats["bonus_emitted"] += 1
                stats["edits_showed"] += bonus[i] != plain[i]
        if num_logprobs is not None:
            lists = out.logprobs
            assert lists is not None
            stats["logprob_steps"] += 1
            col0 = [row[0] for row in lists.logprob_token_ids]
            assert col0 == bonus                                        # the sampler's tokens, from the EDITED rows
            want_ids, want_lp, want_rank = LO.f64_oracle(raw, col0, num_logprobs)     # logprobs of the RAW rows
            assert lists.logprob_token_ids == want_ids.tolist()
            assert lists.sampled_token_ranks == want_rank.tolist()
            got = np.asarray(lists.logprobs, dtype=np.float64)
            assert LO.within_bar(got, want_lp).all(), LO.max_excess(got, want_lp)
    print(f"steps skipped for a fixture margin: {stats['skipped']} of {steps}; sampled tokens the edits changed: "
          f"{stats['edits_showed']} of {stats['bonus_emitted']}")
    stats.update(rs_calls=RejectionSampler.calls, sampler_calls=Sampler.calls)
    return stats


FORMS = {"greedy": (GREEDY, False), "random": (TEMPS, False), "filtered": (TEMPS, True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_all_switches_on_edited_steps_run_on_hip_and_emit_the_oracles_tokens(stub_vllm, monkeypatch, form):
    import vllm.v1.outputs
    monkeypatch.setattr(vllm.v1.outputs, "LogprobsTensors", LO.LogprobsTensors, raising=False)
    for env in (EDITS_ENV, SAMPLER_ENV, FILTER_ENV, LOGPROBS_ENV):
        monkeypatch.setenv(env, "1")
    temps, filters = FORMS[form]
    runner = _runner()
    calls = _spy(monkeypatch)
    steps = 28
    st = _drive(runner, monkeypatch, steps, temps, filters, check=True, num_logprobs=N_LOGPROBS)
    assert st["sampler_calls"] == 0, "a step reached vLLM's Sampler"
    assert st["rs_calls"] == 0, "a step reached vLLM's RejectionSampler"
    assert st["verify"] > 5 and st["draft_free"] >= 1, st
    assert st["skipped"] <= MAX_SKIPPED_FRACTION * steps, st
    assert st["edits_showed"] >= 3, st                      # the edits changed sampled tokens that reached the output
    assert len(st["early"]) == st["verify"]
    # one edit and one sampler call per step, on f32 rows the size of the sampler call; the acceptance gets bonus tokens
    assert len(calls["edit_logits"]) == len(calls["sample_tokens"]) == steps
    assert all(a[0].dtype == torch.float32 and a[0].shape == (B, V) and kw.get("row_index") is None
               for a, kw in calls["sample_tokens"])
    assert sum(kw.get("row_index") is not None for _, kw in calls["edit_logits"]) == st["verify"]
    assert len(calls["rejection_sample"]) == st["verify"]
    assert all(a[3] is not None and kw.get("bonus_row_index") is None for a, kw in calls["rejection_sample"])
    # logprobs: of the raw rows (the model's logits, bf16), with the sampler's tokens
    assert st["logprob_steps"] >= steps - st["skipped"] and len(calls["token_logprobs"]) == steps
    assert all(a[0].dtype == torch.bfloat16 and kw["token_ids"] is not None for a, kw in calls["token_logprobs"])


@pytest.mark.parametrize("form", ["greedy", "filtered"])
def test_new_switch_off_the_step_is_vllms_as_today(stub_vllm, monkeypatch, form):
    monkeypatch.delenv(EDITS_ENV, raising=False)
    monkeypatch.setenv(SAMPLER_ENV, "1")
    monkeypatch.setenv(FILTER_ENV, "1")
    temps, filters = FORMS[form]
    runner = _runner()
    calls = _spy(monkeypatch)
    steps = 12
    st = _drive(runner, monkeypatch, steps, temps, filters, check=False)
    assert st["verify"] > 3
    assert st["sampler_calls"] == steps and st["rs_calls"] == st["verify"] and not st["early"]
    assert not calls["edit_logits"] and not calls["sample_tokens"] and not calls["rejection_sample"]


@pytest.mark.parametrize("form", ["greedy", "random"])
def test_new_switch_on_sampler_switch_off_vllm_draws_the_bonus_tokens_and_hip_accepts(stub_vllm, monkeypatch, form):
    monkeypatch.setenv(EDITS_ENV, "1")
    monkeypatch.delenv(SAMPLER_ENV, raising=False)
    monkeypatch.delenv(FILTER_ENV, raising=False)
    temps, filters = FORMS[form]
    runner = _runner()
    calls = _spy(monkeypatch)
    steps = 12
    st = _drive(runner, monkeypatch, steps, temps, filters, check=False)
    assert st["verify"] > 3
    assert st["sampler_calls"] == steps and st["rs_calls"] == 0            # vLLM's sampler every step, never its RejectionSampler
    assert not calls["edit_logits"] and not calls["sample_tokens"]         # vLLM's sampler edits its own copy
    assert len(calls["rejection_sample"]) == st["verify"] == len(st["early"])
    assert all(a[3] is not None and kw.get("bonus_row_index") is None for a, kw in calls["rejection_sample"])


def test_new_switch_on_steps_without_edit_fields_take_todays_path(stub_vllm, monkeypatch):
    for env in (EDITS_ENV, SAMPLER_ENV, FILTER_ENV):
        monkeypatch.setenv(env, "1")
    runner = _runner()
    calls = _spy(monkeypatch)
    steps = 16
    stats, early, rs_calls, sampler_calls, hip_calls = _drive_without_edits(runner, monkeypatch, steps, filters=True, check=True)
    assert sampler_calls == 0 and rs_calls == 0 and hip_calls == steps and stats["skipped"] <= 1
    assert not calls["edit_logits"]                                        # no extra launch
    assert all(a[0].dtype == torch.bfloat16 for a, _ in calls["sample_tokens"])      # the model's rows, in place
