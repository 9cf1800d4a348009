"""GPU: a float16 model on the plugin's HIP attention route, through the stand-in for vLLM 0.9.2 (tests/stubs) with
n-gram drafts, after tests/test_vllm_prefill_route_gpu.py: fp16 parameters, fp16 hidden states and an fp16 KV cache.
Tokens equal the unpatched stand-in's and hidden states match it; with ARCTIC_INFERENCE_HIP_PREFILL on no attention call
falls back, with it off only the steps with prefill chunks do.  A float32 model is not the kernels' to serve: every
attention call falls back and the run equals the unpatched one."""
import pytest
import torch

import vllm_harness as H
from test_vllm_plugin_gpu import DEV, Steered, _requests, _vllm_config

pytestmark = pytest.mark.gpu
ENV = "ARCTIC_INFERENCE_HIP_PREFILL"
L = 2          # attention layers of the toy model


def _drive(patched, dtype, streams, prompt_len, steps, chunk=None):
    if patched:
        H.install()
        H.load_plugin()
    from vllm.config import SpeculativeConfig, set_current_vllm_config
    from vllm.v1.worker.gpu_model_runner import GPUModelRunner
    cfg = _vllm_config(SpeculativeConfig(method="ngram", num_speculative_tokens=2), dtype=dtype)
    H.init_single_process_groups(cfg)
    r = GPUModelRunner(cfg, torch.device(DEV))
    set_current_vllm_config(cfg)
    r.load_model()
    r.initialize_kv_cache((200, dtype))
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
        assert steer.hidden.dtype == dtype
        hs.append(steer.hidden.float().cpu())
    return hs, toks, max_q


def _same_run(a_hs, a_toks, b_hs, b_toks):
    assert b_toks == a_toks
    for x, y in zip(a_hs, b_hs):
        assert x.shape == y.shape
        assert torch.allclose(x, y, atol=3e-2, rtol=3e-2), (x - y).abs().max()


@pytest.mark.parametrize("case", [dict(n=3, prompt_len=80, steps=6), dict(n=2, prompt_len=200, steps=8, chunk=64)],
                         ids=["pure-prefill-first-step", "chunked-prefill"])
def test_fp16_model_takes_the_hip_route(stub_vllm, monkeypatch, case):
    c = dict(case)
    streams = _requests(c.pop("n"), 200, seed=9)
    monkeypatch.delenv(ENV, raising=False)
    a_hs, a_toks, max_q = _drive(False, torch.float16, streams, **c)
    n_prefill_steps = sum(m > 33 for m in max_q)
    assert 1 <= n_prefill_steps < len(max_q)
    from arcticinference_amd.vllm_plugin import step_context
    # switch off: decode / verify steps on the HIP route, only the steps with chunks fall back
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    off_hs, off_toks, _ = _drive(True, torch.float16, streams, **c)
    assert step_context.calls["fallback"] == n_prefill_steps * L and step_context.calls["prefill"] == 0, step_context.calls
    assert step_context.calls["verify"] == (len(max_q) - n_prefill_steps) * L, step_context.calls
    _same_run(a_hs, a_toks, off_hs, off_toks)
    # switch on: every attention call on the HIP route
    monkeypatch.setenv(ENV, "1")
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    on_hs, on_toks, _ = _drive(True, torch.float16, streams, **c)
    assert step_context.calls["fallback"] == 0, step_context.calls
    assert step_context.calls["verify"] == len(max_q) * L and step_context.calls["prefill"] == n_prefill_steps * L
    _same_run(a_hs, a_toks, on_hs, on_toks)


def test_float32_model_falls_back_on_every_attention_call(stub_vllm, monkeypatch):
    streams = _requests(2, 200, seed=9)
    monkeypatch.setenv(ENV, "1")
    a_hs, a_toks, max_q = _drive(False, torch.float32, streams, prompt_len=80, steps=5)
    from arcticinference_amd.vllm_plugin import step_context
    step_context.calls.update(verify=0, fallback=0, prefill=0)
    b_hs, b_toks, _ = _drive(True, torch.float32, streams, prompt_len=80, steps=5)
    assert step_context.calls["fallback"] == len(max_q) * L, step_context.calls
    assert step_context.calls["verify"] == 0 and step_context.calls["prefill"] == 0, step_context.calls
    _same_run(a_hs, a_toks, b_hs, b_toks)


def test_a_cache_of_the_other_16_bit_type_falls_back(stub_vllm, monkeypatch):
    """An fp16 model over a bf16 cache (and the reverse): _arctic_verify leaves the call to vLLM's backend."""
    streams = _requests(2, 200, seed=9)
    monkeypatch.delenv(ENV, raising=False)
    H.load_plugin()
    from vllm.config import SpeculativeConfig, set_current_vllm_config
    from vllm.v1.worker.gpu_model_runner import GPUModelRunner
    from arcticinference_amd.vllm_plugin import step_context
    for model_dtype, cache_dtype in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)):
        cfg = _vllm_config(SpeculativeConfig(method="ngram", num_speculative_tokens=2), dtype=model_dtype)
        H.init_single_process_groups(cfg)
        r = GPUModelRunner(cfg, torch.device(DEV))
        set_current_vllm_config(cfg)
        r.load_model()
        r.initialize_kv_cache((200, cache_dtype))
        sched = H.MiniScheduler(16, 400)
        for rid, s in streams.items():
            sched.add(rid, [int(x) for x in s[:20]])
        steer = Steered(r, sched, streams)
        step_context.calls.update(verify=0, fallback=0, prefill=0)
        for _ in range(3):
            so = sched.schedule()
            steer.plan(so)
            sched.update(r.execute_model(so))
        assert step_context.calls["fallback"] == 3 * L and step_context.calls["verify"] == 0, step_context.calls
