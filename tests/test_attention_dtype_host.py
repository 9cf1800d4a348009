"""CPU: the host half of the dtype-carrying attention entry points (aic_verify_attention_dt, aic_step_attention_dt) —
the exports, the answer without a device, and the dtype checks ops.verify_attention / ops.step_attention /
ops.VerifyAttentionPlan make before any launch.  No GPU needed."""
import pytest
import torch

from arcticinference_amd import _native as N
from arcticinference_amd import ops


def test_the_dtype_entry_points_are_exported():
    L = N.lib()
    for new, old in (("aic_verify_attention_dt", "aic_verify_attention_win"), ("aic_step_attention_dt", "aic_step_attention_win")):
        assert new in N._SIGNATURES and new in N.EXPORTED_SYMBOLS
        a, b = getattr(L, new).argtypes, getattr(L, old).argtypes
        # the _win signature plus q_dtype, in front of the stream
        assert len(a) == len(b) + 1 and list(a[:len(b) - 1]) == list(b[:-1]) and a[-1] is b[-1]
        from ctypes import c_int
        assert a[-2] is c_int


def _tensors(q_dtype=torch.float16, kv_dtype=torch.float16, Hq=8, Hkv=2, D=128, T=3):
    q = torch.zeros(T, Hq, D, dtype=q_dtype)
    kc = torch.zeros(4, 16, Hkv, D, dtype=kv_dtype)
    return (q, kc, kc.clone(), torch.zeros(2, 4, dtype=torch.int32), torch.tensor([40, 17], dtype=torch.int32),
            torch.tensor([0, 2, 3], dtype=torch.int32))


def test_entry_points_answer_no_device_like_their_siblings():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    L = N.lib()
    q, kc, vc, bt, sl, qsl = _tensors()
    out = torch.zeros_like(q)
    ws = torch.zeros(L.aic_step_attention_workspace_bytes(3, 0, 0, 8, 2, 128, 64), dtype=torch.uint8)
    lists = torch.tensor([0, 1], dtype=torch.int32)

    def verify(fn, kv_dtype, *tail):
        return fn(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), kv_dtype, None, None, bt.data_ptr(),
                  bt.size(1), sl.data_ptr(), qsl.data_ptr(), 2, 3, 2, 8, 2, 128, 16, 0.1, out.data_ptr(), out.stride(0),
                  ws.data_ptr(), ws.numel(), 40, None, 0, None, 0, 0, None, *tail, None)

    def step(fn, kv_dtype, *tail):
        return fn(q.data_ptr(), q.stride(0), kc.data_ptr(), vc.data_ptr(), kc.stride(0), kv_dtype, None, None, bt.data_ptr(),
                  bt.size(1), sl.data_ptr(), qsl.data_ptr(), 2, 3, 8, 2, 128, 16, 0.1, out.data_ptr(), out.stride(0),
                  ws.data_ptr(), ws.numel(), 40, lists.data_ptr(), 2, 0, 0, qsl.data_ptr(), None, 0, 2, 0, 0, None, *tail, None)

    assert verify(L.aic_verify_attention_win, N.DT_BF16) == N.AIC_ERR_NO_DEVICE
    assert step(L.aic_step_attention_win, N.DT_BF16) == N.AIC_ERR_NO_DEVICE
    for qd in (N.DT_BF16, N.DT_F16):
        assert verify(L.aic_verify_attention_dt, qd, qd) == N.AIC_ERR_NO_DEVICE
        assert step(L.aic_step_attention_dt, qd, qd) == N.AIC_ERR_NO_DEVICE
    # the dtype rules come first: they need no device
    for qd, kvd in ((N.DT_F32, N.DT_F16), (N.DT_F16, N.DT_BF16), (N.DT_BF16, N.DT_F16), (N.DT_F16, N.DT_FP8_E5M2)):
        assert verify(L.aic_verify_attention_dt, kvd, qd) == N.AIC_ERR_UNSUPPORTED
        assert b"dtype" in L.aic_last_error()
        assert step(L.aic_step_attention_dt, kvd, qd) == N.AIC_ERR_UNSUPPORTED
    # the bf16-only entry points say so for an fp16 cache
    assert verify(L.aic_verify_attention_win, N.DT_F16) == N.AIC_ERR_UNSUPPORTED
    # an empty call is served whatever it names (as before)
    assert L.aic_verify_attention_dt(None, 0, None, None, 0, N.DT_F16, None, None, None, 0, None, None, 0, 0, 0, 8, 2, 128,
                                     16, 0.1, None, 0, None, 0, 0, None, 0, None, 0, 0, None, N.DT_F16, None) == N.AIC_OK


def _calls(t, **kw):
    return (lambda: ops.verify_attention(*t, 2, 40, 0.1, **kw),
            lambda: ops.verify_attention(*t, 2, 40, 0.1, q_lens_host=[2, 1], **kw),
            lambda: ops.step_attention(*t, 40, 0.1, q_lens_host=[2, 1], **kw))


@pytest.mark.parametrize("q_dtype", [torch.float32, torch.float64, torch.int16])
def test_a_query_that_is_neither_bf16_nor_fp16_is_a_value_error(q_dtype):
    for call in _calls(_tensors(q_dtype=q_dtype)):
        with pytest.raises(ValueError, match="bfloat16 and float16"):
            call()


@pytest.mark.parametrize("q_dtype,out_dtype", [(torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16),
                                               (torch.float16, torch.float32)])
def test_out_of_another_dtype_is_a_value_error(q_dtype, out_dtype):
    t = _tensors(q_dtype=q_dtype, kv_dtype=q_dtype)
    for call in _calls(t, out=torch.zeros(t[0].shape, dtype=out_dtype)):
        with pytest.raises(ValueError, match="out must have the query's dtype"):
            call()


@pytest.mark.parametrize("q_dtype,kv_dtype", [(torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16)])
def test_a_cache_of_the_other_16_bit_type_is_a_value_error(q_dtype, kv_dtype):
    for call in _calls(_tensors(q_dtype=q_dtype, kv_dtype=kv_dtype)):
        with pytest.raises(ValueError, match="16-bit kv cache must have the query's dtype"):
            call()


@pytest.mark.parametrize("q_dtype,kv_dtype", [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16),
                                              (torch.float16, torch.float8_e4m3fn)])
def test_served_dtypes_get_past_the_dtype_checks(q_dtype, kv_dtype):
    """On CPU tensors the next check answers: the ops run on the GPU only."""
    for call in _calls(_tensors(q_dtype=q_dtype, kv_dtype=kv_dtype)):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()


@pytest.mark.parametrize("q_dtype,out_dtype,kv_dtype", [(torch.float16, torch.float16, torch.float16),
                                                        (torch.bfloat16, torch.float16, torch.bfloat16),
                                                        (torch.bfloat16, torch.bfloat16, torch.float16),
                                                        (torch.float32, torch.float32, torch.bfloat16)])
def test_the_plan_is_bf16_only_and_says_so(q_dtype, out_dtype, kv_dtype):
    q, kc, _, bt, sl, qsl = _tensors(q_dtype=q_dtype, kv_dtype=kv_dtype)
    with pytest.raises(ValueError, match="VerifyAttentionPlan serves bfloat16"):
        ops.VerifyAttentionPlan(q, torch.zeros(q.shape, dtype=out_dtype), kc, bt, sl, qsl, 2, 40, 0.1)
