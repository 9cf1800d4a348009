"""CPU: the host half of whole-step attention on gpt-oss-class layers (aic_step_attention_win) — the export, the sink
checks ops.step_attention makes before any launch, and the workspace bound for head size 64.  No GPU needed."""
import pytest
import torch

from arcticinference_amd import _native as N
from arcticinference_amd import ops


def test_step_attention_win_is_exported():
    assert "aic_step_attention_win" in N._SIGNATURES
    fn = N.lib().aic_step_attention_win
    assert len(fn.argtypes) == len(N.lib().aic_step_attention.argtypes) + 2


def _args(Hq=8, Hkv=1, D=64):
    q = torch.zeros(40, Hq, D, dtype=torch.bfloat16)
    kc = torch.zeros(4, 16, Hkv, D, dtype=torch.bfloat16)
    return (q, kc, kc.clone(), torch.zeros(1, 4, dtype=torch.int32), torch.tensor([40], dtype=torch.int32),
            torch.tensor([0, 40], dtype=torch.int32), 40, D ** -0.5)


@pytest.mark.parametrize("sinks", [
    torch.zeros(8, dtype=torch.float64),               # wrong dtype
    torch.zeros(8, dtype=torch.bfloat16),
    torch.zeros(7, dtype=torch.float32),               # wrong length
    torch.zeros(16, dtype=torch.float32),
    torch.zeros(16, dtype=torch.float32)[::2],         # one per head, but not contiguous
], ids=["f64", "bf16", "short", "long", "strided"])
def test_malformed_sinks_are_rejected_before_any_launch(sinks):
    with pytest.raises(ValueError, match="sinks"):
        ops.step_attention(*_args(), q_lens_host=[40], sliding_window=128, sinks=sinks)


@pytest.mark.parametrize("Hq,Hkv", [(64, 8), (8, 1), (32, 8)])
def test_workspace_for_head_size_64_is_at_most_head_size_128(Hq, Hkv):
    ws = N.lib().aic_step_attention_workspace_bytes
    n_dec = sum(1 + (i % 33) for i in range(63))
    for n_pf, chunk in ((1, 34), (1, 512), (1, 2048), (1, 8192), (4, 300)):
        for nd in (0, n_dec):
            assert ws(nd, n_pf, chunk, Hq, Hkv, 64, 64) <= ws(nd, n_pf, chunk, Hq, Hkv, 128, 64), (nd, n_pf, chunk)
    # a split prefill call (one small chunk on one kv head) keeps partials of the head size: strictly less at D = 64
    assert ws(0, 1, 64, 8, 1, 64, 64) < ws(0, 1, 64, 8, 1, 128, 64)
