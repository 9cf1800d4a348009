"""CPU: the cache-layout check the paged wrappers make before any launch (ops._check_kv_layout): a cache is
[num_blocks, block_size, Hkv, D] with contiguous pages, only the block stride is free, and K, V and every layer of a call
share shape, dtype and strides.  A permuted view (an HND cache seen as [nb, bs, Hkv, D]), a layer with another block
stride, and K and V with different strides are ValueErrors; both layouts of tests/high_page_arena.py are accepted (on
CPU tensors the next check answers: the ops run on the GPU only).  No GPU needed."""
import pytest
import torch

from arcticinference_amd import ops

NB, BS, HKV, D, HQ = 6, 16, 2, 128, 8


def _step(dtype=torch.bfloat16):
    q = torch.zeros(3, HQ, D, dtype=dtype)
    return q, torch.zeros(2, 4, dtype=torch.int32), torch.tensor([40, 17], dtype=torch.int32), \
        torch.tensor([0, 2, 3], dtype=torch.int32)


def _contiguous(dtype=torch.bfloat16):
    return torch.zeros(NB, BS, HKV, D, dtype=dtype), torch.zeros(NB, BS, HKV, D, dtype=dtype)


def _hnd(dtype=torch.bfloat16):
    """Pages stored [Hkv, bs, D], seen as [nb, bs, Hkv, D]."""
    mk = lambda: torch.zeros(NB, HKV, BS, D, dtype=dtype).permute(0, 2, 1, 3)
    return mk(), mk()


def _shifted(dtype=torch.bfloat16):
    buf = torch.zeros((NB + 1) * BS * HKV * D, dtype=dtype)
    page = BS * HKV * D
    return buf[:NB * page].view(NB, BS, HKV, D), buf[page:].view(NB, BS, HKV, D)


def _interleaved(dtype=torch.bfloat16):
    buf = torch.zeros(NB, 2, BS, HKV, D, dtype=dtype)
    return buf[:, 0], buf[:, 1]


def _attention_calls(kc, vc):
    q, bt, sl, qsl = _step(kc.dtype if kc.dtype != torch.float8_e4m3fn else torch.bfloat16)
    t = (q, kc, vc, bt, sl, qsl)

    class _Tree:                                        # the fields the wrapper reads before the layout check
        num_tokens, batch, max_q_len = 3, 2, 2
        tree_mask = torch.zeros(3, dtype=torch.int64)
    return {
        "verify_attention": lambda: ops.verify_attention(*t, 2, 40, 0.1),
        "verify_attention-lists": lambda: ops.verify_attention(*t, 2, 40, 0.1, q_lens_host=[2, 1]),
        "step_attention": lambda: ops.step_attention(*t, 40, 0.1, q_lens_host=[2, 1]),
        "verify_attention_tree": lambda: ops.verify_attention_tree(q, kc, vc, bt, sl, _Tree(), 40, 0.1),
    }


@pytest.mark.parametrize("call", ["verify_attention", "verify_attention-lists", "step_attention", "verify_attention_tree"])
def test_a_permuted_view_is_a_value_error(call):
    kc, vc = _hnd()
    assert kc.shape == (NB, BS, HKV, D) and kc.stride(3) == 1 and kc.stride(2) != D
    with pytest.raises(ValueError, match="contiguous pages"):
        _attention_calls(kc, vc)[call]()


@pytest.mark.parametrize("call", ["verify_attention", "verify_attention-lists", "step_attention", "verify_attention_tree"])
def test_k_and_v_with_different_strides_are_a_value_error(call):
    kc, _ = _contiguous()
    _, vc = _interleaved()
    assert kc.shape == vc.shape and kc.stride(0) != vc.stride(0)
    with pytest.raises(ValueError, match="share shape, dtype and strides"):
        _attention_calls(kc, vc)[call]()
    with pytest.raises(ValueError, match="share shape, dtype and strides"):
        _attention_calls(kc, torch.zeros(NB + 1, BS, HKV, D, dtype=kc.dtype))[call]()


@pytest.mark.parametrize("layout", [_contiguous, _shifted, _interleaved], ids=["contiguous", "shifted", "interleaved"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float8_e4m3fn], ids=["bf16", "f16", "e4m3"])
def test_both_arena_layouts_get_past_the_layout_check(layout, dtype):
    kc, vc = layout(dtype)
    assert kc.data_ptr() != vc.data_ptr()
    for name, call in _attention_calls(kc, vc).items():
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.KvBulkWriter([kc], [vc], "auto", [torch.ones(1)], [torch.ones(1)], HKV, D)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.KvPathCompactor([kc, kc], [vc, vc])


def test_the_plan_checks_its_caches_at_every_door():
    q, bt, sl, qsl = _step()
    out = torch.zeros_like(q)
    with pytest.raises(ValueError, match="contiguous pages"):
        ops.VerifyAttentionPlan(q, out, _hnd()[0], bt, sl, qsl, 2, 40, 0.1)
    # past __init__ a plan needs a device; layer_tables / run check before they touch one
    plan = ops.VerifyAttentionPlan.__new__(ops.VerifyAttentionPlan)
    kc, vc = _contiguous()
    plan._kv_shape, plan._kv_dtype, plan._kv_stride = tuple(kc.shape), kc.dtype, tuple(kc.stride())
    plan.layer_tables([kc], [vc])
    for bad in (_hnd()[0], _interleaved()[0], kc.to(torch.float16), torch.zeros(NB + 1, BS, HKV, D, dtype=kc.dtype)):
        with pytest.raises(ValueError, match="another shape / dtype / strides"):
            plan.layer_tables([kc, bad], [vc, vc])
        with pytest.raises(ValueError, match="another shape / dtype / strides"):
            plan.layer_tables([kc, kc], [vc, bad])
        with pytest.raises(ValueError, match="another shape / dtype / strides"):
            plan.run(bad, vc)
        with pytest.raises(ValueError, match="another shape / dtype / strides"):
            plan.run(kc, bad)                           # V as well: it was not looked at before
    with pytest.raises(ValueError, match="same length"):
        plan.layer_tables([kc, kc], [vc])


def test_the_bulk_writer_checks_every_layer():
    kc, vc = _contiguous()
    ik, iv = _interleaved()
    one = [torch.ones(1)] * 2
    with pytest.raises(ValueError, match="layer 1"):                      # a layer with another block stride
        ops.KvBulkWriter([kc, ik], [vc, iv], "auto", one, one, HKV, D)
    with pytest.raises(ValueError, match="contiguous pages"):             # a permuted layer behind a good one
        ops.KvBulkWriter([kc, _hnd()[0]], [vc, _hnd()[1]], "auto", one, one, HKV, D)
    with pytest.raises(ValueError, match="share shape, dtype and strides"):   # K and V of one layer
        ops.KvBulkWriter([kc, kc], [vc, iv], "auto", one, one, HKV, D)
    with pytest.raises(ValueError, match="layer 1"):
        ops.KvBulkWriter([kc, kc.to(torch.float16)], [vc, vc.to(torch.float16)], "auto", one, one, HKV, D)


def test_the_compactor_keeps_its_check():
    kc, vc = _contiguous()
    with pytest.raises(ValueError):
        ops.KvPathCompactor([_hnd()[0]], [_hnd()[1]])
    with pytest.raises(ValueError):
        ops.KvPathCompactor([kc, _interleaved()[0]], [vc, _interleaved()[1]])
    with pytest.raises(ValueError):
        ops.KvPathCompactor([kc], [_interleaved()[1]])
