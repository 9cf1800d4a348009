"""Per-step geometry the model-runner patch publishes for the attention patch.

vLLM's Attention.forward sees device tensors only; the runner knows on the HOST how many tokens each request of
the step has (scheduler_output.num_scheduled_tokens).  aic_verify_attention_ex wants the batch partitioned by
query length (short requests / long suffix drafts, include/arctic_hip.h), so the runner publishes the step's
per-request query lengths here and every attention layer of the step reuses one partition built from them.
One runner per process (vLLM worker), one step at a time: a module-level slot is the whole mechanism.

Steps with prefill chunks (a request of more than MAX_SPEC_LEN + 1 query tokens) go to aic_step_attention when the
PREFILL_ENV switch is on (read once per step, in publish()); step_split() is its per-step partition."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np

PREFILL_ENV = "ARCTIC_INFERENCE_HIP_PREFILL"   # 1: steps with prefill chunks on the HIP route too (default off)

_q_lens: Optional[np.ndarray] = None
_shift_mode: bool = False
_prefill_on: bool = False
_shared_prefix_on: bool = False
_prefix_groups_on: bool = False
_group_inputs = None                             # (host block table, computed tokens per request, block size) or None
_groups: Dict[Tuple[int, bool, int], object] = {}   # (kv heads, fp8 cache, device index) -> ops.PrefixGroups | None
_splits: Dict[Tuple[int, int], object] = {}     # (group size, device index) -> ops.split_requests(...) of this step
_step_splits: Dict[Tuple[int, int], object] = {}  # (group size, device index) -> ops.StepSplit of this step
# attention calls routed to the HIP kernels (verify: all of them; prefill: those of them with prefill chunks) / left to
# vLLM's backend
# shared_prefix: those of the verify calls that read a shared prompt prefix once (SHARED_PREFIX_ENV)
# prefix_groups: those that read a prefix per group of requests once (PREFIX_GROUPS_ENV)
calls = {"verify": 0, "fallback": 0, "prefill": 0, "shared_prefix": 0, "prefix_groups": 0}


def prefill_switch() -> bool:
    return os.environ.get(PREFILL_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


def publish(num_scheduled_tokens: np.ndarray, shift_mode: bool, *, block_table=None, num_computed=None,
            block_size: Optional[int] = None) -> None:
    """`block_table` (the step's HOST block table, anything runner_logic.host_block_table reads), `num_computed` (tokens
    already in the cache per request) and `block_size`: what the prefix-group detection needs; the runner passes them
    only with PREFIX_GROUPS_ENV on.  Without them a step has no groups."""
    global _q_lens, _shift_mode, _prefill_on, _shared_prefix_on, _prefix_groups_on, _group_inputs
    _q_lens = np.asarray(num_scheduled_tokens)
    _shift_mode = bool(shift_mode)
    _prefill_on = prefill_switch()
    _shared_prefix_on = shared_prefix_switch()
    _prefix_groups_on = prefix_groups_switch()
    _group_inputs = None
    if _prefix_groups_on and block_table is not None and num_computed is not None and block_size:
        _group_inputs = (block_table, num_computed, int(block_size))
    _splits.clear()
    _step_splits.clear()
    _groups.clear()


def clear() -> None:
    global _q_lens, _group_inputs
    _q_lens = None
    _group_inputs = None
    _splits.clear()
    _step_splits.clear()
    _groups.clear()


def prefill_on() -> bool:
    return _prefill_on


def shared_prefix_switch() -> bool:
    from .runner_logic import SHARED_PREFIX_ENV
    return os.environ.get(SHARED_PREFIX_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


def shared_prefix_on() -> bool:
    """ARCTIC_INFERENCE_HIP_SHARED_PREFIX as read when the step was published (default off)."""
    return _shared_prefix_on


def prefix_groups_switch() -> bool:
    from .runner_logic import PREFIX_GROUPS_ENV
    return os.environ.get(PREFIX_GROUPS_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


def prefix_groups_on() -> bool:
    """ARCTIC_INFERENCE_HIP_PREFIX_GROUPS as read when the step was published (default off)."""
    return _prefix_groups_on


def prefix_groups(num_kv_heads: int, fp8: bool, device):
    """ops.PrefixGroups of the published step for a layer with `num_kv_heads` local kv heads (built once per step and
    shared by its layers), or None: switch off, nothing published for it, or runner_logic.prefix_groups said no."""
    if not _prefix_groups_on or _group_inputs is None or _q_lens is None:
        return None
    key = (int(num_kv_heads), bool(fp8), device.index)
    if key not in _groups:
        from .. import ops
        from .runner_logic import prefix_groups as decide
        found = decide(_group_inputs[0], _group_inputs[1], _q_lens, _group_inputs[2], num_kv_heads, fp8)
        _groups[key] = None if found is None else ops.PrefixGroups(found[0], found[1], _q_lens, device)
    return _groups[key]


def q_lens() -> Optional[np.ndarray]:
    return _q_lens


def shift_mode() -> bool:
    return _shift_mode


def request_split(group_size: int, device):
    """(short ids, n_short, long ids, n_long) for the step, or None when every request is short / nothing is published."""
    if _q_lens is None:
        return None
    key = (group_size, device.index)
    if key not in _splits:
        from .. import ops
        _splits[key] = ops.split_requests(_q_lens, group_size, device)
    return _splits[key]


def step_split(group_size: int, device):
    """ops.StepSplit of the published step (three-way request lists + compact decode layout), or None when nothing is
    published."""
    if _q_lens is None:
        return None
    key = (group_size, device.index)
    if key not in _step_splits:
        from .. import ops
        _step_splits[key] = ops.StepSplit(_q_lens, group_size, device)
    return _step_splits[key]


def route(max_query_len: int, q_lens, batch: int, prefill_on: bool, layer_ok: bool, capturing: bool) -> str:
    """Which attention serves a call: "verify" (every request has at most MAX_SPEC_LEN + 1 query tokens: the verify
    bodies, as before), "step" (prefill chunks in the step, served by aic_step_attention) or "fallback" (vLLM's
    backend).  Prefill steps take the HIP route only with the switch on, on a layer the prefill body serves (head size
    128 with a 16-bit / fp8 cache, or 64 with a 16-bit cache; any sliding window, sinks or none; the caller has already
    sent alibi and soft-cap layers back), with published q_lens that describe the call
    (`batch` requests, the longest `max_query_len` tokens) and outside graph capture."""
    from .runner_logic import MAX_SPEC_LEN
    if max_query_len <= MAX_SPEC_LEN + 1:
        return "verify"
    if not (prefill_on and layer_ok) or capturing or q_lens is None:
        return "fallback"
    if len(q_lens) != batch or int(np.max(q_lens)) != int(max_query_len):
        return "fallback"
    return "step"
