"""GPU: steps with prefill chunks of a gpt-oss-like model (head size 64, G = 8, a sliding window on every other layer,
per-head sinks on all of them) on the plugin's HIP route (ARCTIC_INFERENCE_HIP_PREFILL=1, aic_step_attention_win),
through the stand-in for vLLM 0.9.2 (tests/stubs): emitted tokens equal the stand-in backend's run, hidden states agree,
and no attention call falls back.  With the switch off the routing is unchanged: only the prefill steps fall back."""
import os
import socket

import numpy as np
import pytest
import torch

import vllm_harness as H
from test_vllm_plugin_gpu import DEV, GPT_OSS_LIKE, Steered, _requests, _vllm_config

pytestmark = pytest.mark.gpu
ENV = "ARCTIC_INFERENCE_HIP_PREFILL"
L = GPT_OSS_LIKE["num_hidden_layers"]


def _drive(patched, streams, prompt_len, steps, chunk=None):
    if patched:
        H.install()
        H.load_plugin()
    from vllm.config import SpeculativeConfig, set_current_vllm_config
    from vllm.v1.worker.gpu_model_runner import GPUModelRunner
    cfg = _vllm_config(SpeculativeConfig(method="ngram", num_speculative_tokens=2), hf=GPT_OSS_LIKE)
    H.init_single_process_groups(cfg)
    r = GPUModelRunner(cfg, torch.device(DEV))
    set_current_vllm_config(cfg)
    r.load_model()
    r.initialize_kv_cache((200, torch.bfloat16))
    sched = H.MiniScheduler(16, 400, chunk=chunk)
    for rid, s in streams.items():
        sched.add(rid, [int(x) for x in s[:prompt_len]])
    steer = Steered(r, sched, streams)
    hs, toks, max_q = [], [], []
    for _ in range(steps):
        so = sched.schedule()
        max_q.append(max(so.num_scheduled_tokens.values()))
        steer.plan(so)
        toks.append(sched.update(r.execute_model(so)))
        hs.append(steer.hidden.float().cpu())
    return hs, toks, max_q


CASES = {
    "pure-prefill-first-step": dict(n=3, prompt_len=80, steps=6),
    # 64-token chunks against the toy's 48-token window: windows cut across chunk boundaries
    "chunked-prefill": dict(n=2, prompt_len=200, steps=8, chunk=64),
}


@pytest.mark.parametrize("case", list(CASES))
def test_gpt_oss_prefill_steps_on_the_hip_route_equal_the_stand_in_backend(stub_vllm, monkeypatch, case):
    c = dict(CASES[case])
    streams = _requests(c.pop("n"), 200, seed=9)
    monkeypatch.delenv(ENV, raising=False)
    a_hs, a_toks, max_q = _drive(False, streams, **c)
    n_prefill_steps = sum(m > 33 for m in max_q)
    assert n_prefill_steps >= 1
    from arcticinference_amd.vllm_plugin import step_context
    # switch off: today's routing (every step with a chunk falls back, the decode steps take the verify route)
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    _drive(True, streams, **c)
    assert step_context.calls["fallback"] == n_prefill_steps * L and step_context.calls["prefill"] == 0
    assert step_context.calls["verify"] == (len(max_q) - n_prefill_steps) * L
    # switch on: every attention call on the HIP route, window and full layers alike
    monkeypatch.setenv(ENV, "1")
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    b_hs, b_toks, _ = _drive(True, streams, **c)
    assert step_context.calls["fallback"] == 0, step_context.calls
    assert step_context.calls["verify"] == len(max_q) * L and step_context.calls["prefill"] == n_prefill_steps * L
    assert b_toks == a_toks
    for x, y in zip(a_hs, b_hs):
        assert x.shape == y.shape
        assert torch.allclose(x, y, atol=3e-2, rtol=3e-2), (x - y).abs().max()


def _sp_worker_gpt_oss(rank, world, port, out_q):
    """One rank of the SP run on the gpt-oss-like model (1 kv head and 8 query heads per rank at SP = 2, sinks sliced
    per rank); world = 1 is the unpatched single-process reference."""
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        H.install()
        if world > 1:
            H.load_plugin()
        from vllm.config import ParallelConfig, set_current_vllm_config
        from vllm.distributed import parallel_state as ps
        from vllm.v1.worker.gpu_model_runner import GPUModelRunner
        kw = dict(ulysses_sequence_parallel_size=world, enable_shift_parallel=True, shift_parallel_threshold=16) if world > 1 else {}
        cfg = _vllm_config(parallel=ParallelConfig(**kw), hf=GPT_OSS_LIKE)
        cfg.parallel_config.rank = rank
        ps.reset_for_tests()
        ps.init_world_group(rank)
        set_current_vllm_config(cfg)
        ps.initialize_model_parallel(1, 1)
        r = GPUModelRunner(cfg, torch.device(DEV))
        r.load_model()
        r.initialize_kv_cache((200, torch.bfloat16))
        streams = _requests(3, 64, seed=4)
        sched = H.MiniScheduler(16, 400)
        for rid, s in streams.items():
            sched.add(rid, [int(x) for x in s[:64]])
        steer = Steered(r, sched, streams)
        hs, toks = [], []
        for _ in range(6):
            so = sched.schedule()
            steer.plan(so)
            toks.append(sched.update(r.execute_model(so)))
            hs.append(steer.hidden.float().cpu().numpy())
        calls = None
        if world > 1:
            from arcticinference_amd.vllm_plugin import step_context
            calls = dict(step_context.calls)
        out_q.put((world, rank, toks, hs, calls))
    except BaseException:
        import traceback
        out_q.put((world, rank, "error", traceback.format_exc(), None))
        raise
    finally:
        dist.destroy_process_group()


def test_sp2_gpt_oss_prefill_on_the_hip_route(monkeypatch):
    """Ulysses SP = 2 in two processes with the switch on: the SP-mode prefill step of the gpt-oss-like model attends
    through aic_step_attention_win after the all-to-all (window and sinks on each rank's heads); tokens equal the
    single-process run and nothing falls back."""
    import torch.multiprocessing as mp
    monkeypatch.setenv(ENV, "1")          # inherited by the spawned workers
    ctx = mp.get_context("spawn")
    q = ctx.Queue()

    def launch(world):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        ps = [ctx.Process(target=_sp_worker_gpt_oss, args=(r, world, port, q)) for r in range(world)]
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
        assert calls["fallback"] == 0 and calls["prefill"] == L and calls["verify"] == 6 * L, calls
