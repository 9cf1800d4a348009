"""GPU: steps with prefill chunks on the plugin's HIP route (ARCTIC_INFERENCE_HIP_PREFILL=1, aic_step_attention),
through the stand-in for vLLM 0.9.2 (tests/stubs): hidden states match the stand-in backend's run, emitted tokens are
equal, and no attention call falls back.  With the switch off the same script keeps today's routing."""
import socket

import numpy as np
import pytest
import torch

import vllm_harness as H
from test_vllm_plugin_gpu import DEV, Steered, _requests, _sp_worker, _vllm_config

pytestmark = pytest.mark.gpu
ENV = "ARCTIC_INFERENCE_HIP_PREFILL"


def _drive(patched, streams, prompt_len, steps, chunk=None, late=None):
    """`late` = (step, request id, prompt length): a request added before that step (its chunks then share steps with
    the others' decodes and drafts)."""
    if patched:
        H.install()
        H.load_plugin()
    from vllm.config import SpeculativeConfig, set_current_vllm_config
    from vllm.v1.worker.gpu_model_runner import GPUModelRunner
    cfg = _vllm_config(SpeculativeConfig(method="ngram", num_speculative_tokens=2))
    H.init_single_process_groups(cfg)
    r = GPUModelRunner(cfg, torch.device(DEV))
    set_current_vllm_config(cfg)
    r.load_model()
    r.initialize_kv_cache((200, torch.bfloat16))
    sched = H.MiniScheduler(16, 400, chunk=chunk)
    for rid, s in streams.items():
        if late is None or rid != late[1]:
            sched.add(rid, [int(x) for x in s[:prompt_len]])
    steer = Steered(r, sched, streams)
    hs, toks, max_q = [], [], []
    for step in range(steps):
        if late is not None and step == late[0]:
            sched.add(late[1], [int(x) for x in streams[late[1]][:late[2]]])
        so = sched.schedule()
        max_q.append(max(so.num_scheduled_tokens.values()))
        steer.plan(so)
        toks.append(sched.update(r.execute_model(so)))
        hs.append(steer.hidden.float().cpu())
    return hs, toks, max_q


CASES = {
    "pure-prefill-first-step": dict(n=3, prompt_len=80, steps=6),
    "chunked-prefill": dict(n=2, prompt_len=200, steps=8, chunk=64),
    "request-added-mid-run": dict(n=3, prompt_len=80, steps=9, chunk=64, late=(3, "r2", 150)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_prefill_steps_on_the_hip_route_equal_the_stand_in_backend(stub_vllm, monkeypatch, case):
    c = dict(CASES[case])
    streams = _requests(c.pop("n"), 200, seed=9)
    monkeypatch.delenv(ENV, raising=False)
    a_hs, a_toks, max_q = _drive(False, streams, **c)
    n_prefill_steps = sum(m > 33 for m in max_q)
    assert n_prefill_steps >= 1
    from arcticinference_amd.vllm_plugin import step_context
    L = 2
    # switch off: today's routing (every step with a chunk falls back)
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    off_hs, off_toks, _ = _drive(True, streams, **c)
    assert step_context.calls["fallback"] == n_prefill_steps * L and step_context.calls["prefill"] == 0
    assert step_context.calls["verify"] == (len(max_q) - n_prefill_steps) * L
    # switch on: every attention call on the HIP route
    monkeypatch.setenv(ENV, "1")
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    b_hs, b_toks, _ = _drive(True, streams, **c)
    assert step_context.calls["fallback"] == 0, step_context.calls
    assert step_context.calls["verify"] == len(max_q) * L and step_context.calls["prefill"] == n_prefill_steps * L
    assert b_toks == a_toks
    for x, y in zip(a_hs, b_hs):
        assert x.shape == y.shape
        assert torch.allclose(x, y, atol=3e-2, rtol=3e-2), (x - y).abs().max()


def test_sp2_prefill_on_the_hip_route(monkeypatch):
    """Ulysses SP = 2 in two processes with the switch on: the SP-mode prefill step attends through aic_step_attention
    after the all-to-all; tokens equal the single-process run and nothing falls back."""
    import torch.multiprocessing as mp
    monkeypatch.setenv(ENV, "1")          # inherited by the spawned workers
    ctx = mp.get_context("spawn")
    q = ctx.Queue()

    def launch(world):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        ps = [ctx.Process(target=_sp_worker, args=(r, world, port, q)) for r in range(world)]
        for p in ps:
            p.start()
        res = [q.get(timeout=300) for _ in range(world)]
        for p in ps:
            p.join(60)
        for x in res:
            assert x[2] != "error", x[3]
        return res

    (_, _, ref_toks, ref_hs, _), = launch(1)
    for _, rank, toks, hs, calls in launch(2):
        assert toks == ref_toks, rank
        for a, b in zip(ref_hs, hs):
            assert np.allclose(a, b, atol=3e-2, rtol=3e-2), (rank, np.abs(a - b).max())
        assert calls["fallback"] == 0 and calls["prefill"] == 2 and calls["verify"] == 12, calls
