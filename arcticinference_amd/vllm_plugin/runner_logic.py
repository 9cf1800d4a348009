"""The selection / slicing / clamp rules of GPUModelRunnerPatch's proposal code
(/root/reference/arctic_inference/vllm/model_runner.py:526-744) as vLLM-free functions, shared by the
stand-alone engine and by the vLLM patch (model_runner.py in this package)."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

from .logits_edits import LOGITS_EDITS_ENV, has_edits, logits_edits_switch  # noqa: F401  (the switch lives with the packing)

MAX_SPEC_LEN = 32  # vllm.v1.sample.rejection_sampler.MAX_SPEC_LEN

# ---------------------------------------------------------------------------------------------------
# Where a request's row ends when the proposers look at it.
#
# The reference's execute_model appends the step's sampled ids to token_ids_cpu and ADVANCES num_tokens_no_spec
# (model_runner.py:469-486); propose_suffix_draft_token_ids (:696-709) and propose_arctic_draft_token_ids (:623-636)
# then take `start_idx = num_tokens_no_spec[i]` and `end_idx = start_idx + len(sampled_ids)` once more and write the
# sampled ids again at [start_idx, end_idx).  Both readings are available:
#   "reference"       the literal arithmetic: the suffix pattern ends with the sampled ids repeated, every
#                     `max_model_len - end_idx - 1` clamp is len(sampled_ids) tighter, the row is re-written;
#   "single_advance"  the row is taken as execute_model left it (end_idx = num_tokens_no_spec[i]): the algorithm of the
#                     reference's own simulator (`(prompt + response)[-max_depth:]`, simulator.py:70-90) and of the golden
#                     fixtures.
# Chosen by the speculative config key `proposal_indexing` (ArcticSpeculativeConfig / engine.SpecConfig) or, above it,
# the environment variable ARCTIC_INFERENCE_PROPOSAL_INDEXING.
#
# DEFAULT (r04): "single_advance".  The literal arithmetic is a leftover of the vLLM 0.8-era runner, whose execute_model
# did not commit the sampled ids before the proposers ran; against vLLM 0.9.2's commit loop (kept verbatim in the
# reference's execute_model, :469-486) it counts every sampled id twice, a suffix pattern that ends in a repeated token
# almost never matches, and suffix decoding contributes nothing (measured: 1.002 tokens per request-step, BENCH_r03
# `other_indexing_mode`).  The emitted tokens are the target's in either mode — only the drafts differ — so the default
# is the algorithm the reference's simulator, its published acceptance numbers and the golden fixtures describe, and
# `proposal_indexing="reference"` is the opt-in switch that reproduces the plugin's drafts, clamps and row contents
# line for line (pinned per step in tests/test_proposal_indexing.py and on the GPU in both modes).
# ---------------------------------------------------------------------------------------------------
INDEXING_REFERENCE = "reference"
INDEXING_SINGLE_ADVANCE = "single_advance"
INDEXING_MODES = (INDEXING_REFERENCE, INDEXING_SINGLE_ADVANCE)
DEFAULT_INDEXING = INDEXING_SINGLE_ADVANCE
INDEXING_ENV = "ARCTIC_INFERENCE_PROPOSAL_INDEXING"


def proposal_indexing(config=None) -> str:
    """The mode in force for a speculative config (any object with an optional `proposal_indexing` attribute)."""
    mode = os.environ.get(INDEXING_ENV) or getattr(config, "proposal_indexing", None) or DEFAULT_INDEXING
    if mode not in INDEXING_MODES:
        raise ValueError(f"proposal_indexing must be one of {INDEXING_MODES}, got {mode!r}")
    return mode


def proposal_end_index(num_tokens_no_spec: int, num_sampled: int, mode: str) -> int:
    """`end_idx` of the proposers (model_runner.py:623-624, :698-699) for a row execute_model has already advanced."""
    return int(num_tokens_no_spec) + (int(num_sampled) if mode == INDEXING_REFERENCE else 0)


def rewrite_sampled(row, start_idx: int, sampled_ids: Sequence[int], max_model_len: int) -> None:
    """The row write of propose_suffix_draft_token_ids in "reference" mode (model_runner.py:701-709): the sampled ids
    once more at [start_idx, end_idx), cut at max_model_len when the request is at the limit."""
    end_idx = start_idx + len(sampled_ids)
    if end_idx >= max_model_len:
        room = max_model_len - start_idx          # numpy slicing rules, as in the reference (a negative bound wraps)
        row[start_idx:max_model_len] = list(sampled_ids)[:room]
    else:
        row[start_idx:end_idx] = sampled_ids


def suffix_query(row: Sequence[int], end_idx: int, spec_ids: Sequence[int], max_model_len: int, max_depth: int,
                 factor: float, offset: float, min_token_prob: float) -> Optional[Tuple[List[int], dict]]:
    """(pattern, kwargs) of one request's SuffixCache.speculate call (model_runner.py:709-740), or None when
    the request is at max_model_len (:701-707)."""
    if end_idx >= max_model_len:
        return None
    size = min(end_idx, max_depth)
    pattern = list(row[end_idx - size:end_idx]) + list(spec_ids)
    if len(pattern) > max_depth:
        pattern = pattern[-max_depth:]
    max_spec_tokens = min(MAX_SPEC_LEN - len(spec_ids), max_depth, max_model_len - end_idx - 1)
    # the offset is rewritten as if the already-speculated tokens came from suffix decoding (:719-733)
    max_spec_offset = offset - len(spec_ids) * (factor + 1)
    return pattern, dict(max_spec_tokens=max_spec_tokens, max_spec_factor=factor, max_spec_offset=max_spec_offset,
                         min_token_prob=min_token_prob)


def min_suffix_score(method: str, num_speculative_tokens: int) -> int:
    """Suffix drafts replace the draft model's iff score >= this (model_runner.py:555-566)."""
    return 0 if method == "suffix" else num_speculative_tokens


def merge_proposals(suffix_ids: Optional[List[List[int]]], model_ids: Optional[List[List[int]]]) -> Optional[List[List[int]]]:
    """`suffix_spec_token_ids[i] or spec_token_ids[i]` (model_runner.py:595-601)."""
    if model_ids is None:
        return suffix_ids
    if suffix_ids is None:
        return model_ids
    return [suffix_ids[i] or model_ids[i] for i in range(len(suffix_ids))]


def arctic_max_spec_tokens(num_speculative_tokens: int, end_indices: Sequence[int], max_model_len: int) -> int:
    """The running clamp of propose_arctic_draft_token_ids (model_runner.py:629-641): one value for the batch."""
    m = num_speculative_tokens
    for end_idx in end_indices:
        m = min(m, max_model_len - end_idx - 1)
        if m <= 0:
            break
    return m


TOP_K_TOP_P_ENV = "ARCTIC_INFERENCE_HIP_TOP_K_TOP_P"   # 1: top-k / top-p batches on the HIP acceptance too (default off)
KIND_TOP_K_TOP_P = "random_topk_topp"


def top_k_top_p_switch() -> bool:
    return os.environ.get(TOP_K_TOP_P_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


LOGPROBS_ENV = "ARCTIC_INFERENCE_HIP_LOGPROBS"   # 1: steps with logprobs requests keep the HIP sampler / acceptance (default off)


def logprobs_switch() -> bool:
    return os.environ.get(LOGPROBS_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


def logprobs_cap() -> int:
    """The largest `max_num_logprobs` aic_token_logprobs serves (aic_logprobs_max)."""
    from .. import _native
    return int(_native.lib().aic_logprobs_max())


def _logprobs_excluded(sm, logprobs: bool) -> bool:
    n = getattr(sm, "max_num_logprobs", None)
    if n is None:
        return False
    return not (logprobs and 0 <= int(n) <= logprobs_cap())


def hip_acceptance_kind(sm, top_k_top_p: bool = False, logprobs: bool = False, logits_edits: bool = False) -> Optional[str]:
    """Which acceptance kernel serves a verify step with this vLLM SamplingMetadata: "greedy" (aic_rejection_greedy),
    "random" (aic_rejection_random: temperature-only rows, greedy rows mixed in), "random_topk_topp"
    (aic_rejection_random_topk_topp: rows with top-k / top-p as well; only when `top_k_top_p`, the TOP_K_TOP_P_ENV
    switch) or None (vLLM's sampler + RejectionSampler: min-p, penalties, logit bias, min_tokens, bad words and
    allowed-token masks live there, and top-k / top-p with the switch off).  A step that reports logprobs
    (`max_num_logprobs` not None) is excluded too unless `logprobs` (the LOGPROBS_ENV switch) is set and
    `max_num_logprobs` is within 0 .. aic_logprobs_max(): the acceptance never touches logprobs, they are those of the
    bonus rows' sampler call, which the caller serves (ops.token_logprobs, or vLLM's sampler where it still draws the
    bonus tokens).  Read field by field the way vLLM 0.9.2's InputBatch fills it: `logit_bias` is a list with one
    entry per request (None where unused) and is therefore never empty; `min_tokens` / `bad_words_token_ids` are dicts;
    tensors are None when no request uses them.
    With `logits_edits` (the LOGITS_EDITS_ENV switch) the edit fields — min-p, penalties, logit bias, min_tokens, bad
    words, allowed-token masks: logits_edits.has_edits — no longer exclude a step, and the result is that of the same
    metadata without them: vLLM's rejection sampler never reads them (its probabilities come from temperature and
    top-k / top-p alone), they act on the bonus rows' sampler call only.  The caller then draws the bonus tokens from
    the edited rows (ops.edit_logits, or vLLM's sampler on its own copy) and hands them to the acceptance as
    `bonus_token_ids`, the all-greedy launch included: its own bonus arg-max reads the raw rows."""
    if _logprobs_excluded(sm, logprobs) or (not logits_edits and has_edits(sm)):
        return None
    if getattr(sm, "all_greedy", False):
        return "greedy"
    if getattr(sm, "temperature", None) is None:
        return None
    if getattr(sm, "top_k", None) is not None or getattr(sm, "top_p", None) is not None:
        return KIND_TOP_K_TOP_P if top_k_top_p else None
    return "random"


HIP_SAMPLER_ENV = "ARCTIC_INFERENCE_HIP_SAMPLER"   # 1: bonus tokens and draft-free steps sampled by aic_sample_topk_topp (default off)


def hip_sampler_switch() -> bool:
    return os.environ.get(HIP_SAMPLER_ENV, "0").strip().lower() in ("1", "true", "yes", "on")


def hip_sampler_ok(sm, logprobs: bool = False, logits_edits: bool = False) -> bool:
    """Whether ops.sample_tokens (aic_sample_topk_topp: temperature, top-k, top-p; greedy rows mixed in or all-greedy)
    can stand in for vLLM's Sampler on this SamplingMetadata.  The exclusions are those of hip_acceptance_kind:
    penalties, allowed-token masks, bad words, logit bias, min_tokens and min-p keep vLLM's sampler, and so does a step
    that reports logprobs unless `logprobs` (the LOGPROBS_ENV switch) is set and `max_num_logprobs` is within
    0 .. aic_logprobs_max(): the caller then reports them with ops.token_logprobs.  `top_k` / `top_p` are served as
    tensors and as None.  With `logits_edits` (the LOGITS_EDITS_ENV switch) the edit fields no longer exclude a step:
    the caller samples the rows ops.edit_logits returns (logits_edits.pack_edits), and reports logprobs of the RAW
    rows as vLLM does."""
    if _logprobs_excluded(sm, logprobs) or (not logits_edits and has_edits(sm)):
        return False
    return bool(getattr(sm, "all_greedy", False)) or getattr(sm, "temperature", None) is not None


SHARED_PREFIX_ENV = "ARCTIC_INFERENCE_HIP_SHARED_PREFIX"   # 1: cascade steps read their common prefix once (default off)
# From where on the plugin hands a common prefix to aic_verify_attention_prefix.  The kernel's own floor is one 32-token
# tile, and vLLM sets use_cascade from 256 common tokens and 8 requests on — but at those sizes the call LOSES: it adds a
# launch, a stream fork / join and partials for every row.  Measured on the MI355X (tools/microbench.py prefix,
# profiles/shared_prefix_microbench.txt; 4224-token contexts, 4 query tokens per request, time of the prefix call / time
# of the plain call; "items" = requests x kv heads of this rank, what the plain call spreads over the chip):
#   bf16 cache, 8 kv heads, 64 requests (512 items): P = 256 1.06, P = 1024 0.97, P = 2048 0.82
#               8 kv heads, 32 requests (256 items), P = 2048: 0.90;  8 requests (64 items): 1.44
#               1 kv head (a rank of SP = 8), 64 requests (64 items), P = 2048: 1.49
#   fp8 cache,  8 kv heads, 64 requests (512 items): P = 256 1.12, P = 1024 1.06, P = 2048 0.90
#               8 kv heads, 32 requests (256 items), P = 2048: 1.20;  8 requests (64 items): 1.93
# So: the smallest measured length at which both cache kinds win, and the smallest measured item count at which each
# cache kind wins there.  A rank of Ulysses SP = 8 with one kv head therefore needs 256 requests (512 with fp8): at the
# 64 requests measured it loses, and is refused.
SHARED_PREFIX_MIN_LEN = 2048
SHARED_PREFIX_MIN_ITEMS = 256        # requests x local kv heads, bf16 / fp16 cache
SHARED_PREFIX_MIN_ITEMS_FP8 = 512    # the same with an fp8 cache
SHARED_PREFIX_FLOOR = 32             # below one tile the kernel serves nothing: never less than this, whatever the constants
_MEASURED_KV_HEADS = 8               # a caller that does not name its kv heads is taken for the measured 8-head shape


def shared_prefix_len(meta, window: int, capturing: bool, switch_on: bool, num_kv_heads: Optional[int] = None,
                      fp8: bool = False) -> int:
    """How many leading tokens of EVERY request of a verify call the HIP route reads once (ops.verify_attention's
    `shared_prefix_len`), or 0 for the plain call: the whole decision, in one place.  vLLM 0.9.2's FlashAttentionMetadata
    says so itself: `use_cascade` with `common_prefix_len` tokens whose pages are the leading columns of every
    block-table row (field names recalled from 0.9.2; parity unpinned).  Taken only with the switch on,
    on a layer without a sliding window, outside graph capture, from SHARED_PREFIX_MIN_LEN tokens (never fewer than 32),
    with at least one query token behind the prefix (`max_seq_len`, where the metadata has it) and — where the metadata
    carries `seq_lens` — from SHARED_PREFIX_MIN_ITEMS (fp8 cache: _FP8) requests x `num_kv_heads` (the layer's kv heads
    on this rank) on.  Metadata without `seq_lens` has no request count to hold against that threshold: deliberately, the
    length rule alone then decides (vLLM's metadata always carries it, so the plugin's own call is always counted).
    Metadata without the cascade fields gives 0.  Correctness never depends on the answer: the block
    table holds the shared pages either way."""
    if not switch_on or capturing or int(window or 0) > 0:
        return 0
    if not getattr(meta, "use_cascade", False):
        return 0
    n = int(getattr(meta, "common_prefix_len", 0) or 0)
    if n < max(SHARED_PREFIX_FLOOR, SHARED_PREFIX_MIN_LEN):
        return 0
    max_seq_len = getattr(meta, "max_seq_len", None)
    if max_seq_len is not None and int(max_seq_len) <= n:
        return 0
    seq_lens = getattr(meta, "seq_lens", None)
    if seq_lens is not None:
        items = int(seq_lens.numel()) * int(num_kv_heads or _MEASURED_KV_HEADS)
        if items < (SHARED_PREFIX_MIN_ITEMS_FP8 if fp8 else SHARED_PREFIX_MIN_ITEMS):
            return 0
    return n


PREFIX_GROUPS_ENV = "ARCTIC_INFERENCE_HIP_PREFIX_GROUPS"   # 1: steps whose requests share prefixes in groups (default off)
PREFIX_GROUPS_MAX = 16               # aic_prefix_max_groups(): groups one call takes (a host test holds the two together)
# From where on the plugin hands groups to aic_verify_attention_prefix_groups.  Measured on the MI355X (tools/microbench.py
# prefixgroups, profiles/prefix_groups_microbench.txt; 64 requests x 4 query tokens, 4224-token contexts, 8 kv heads, both
# forms alternating, medians of 5 windows; time of the grouped call / time of the plain call, the plain call's own
# max - min spread 1.3 .. 6.1 us of ~144 (bf16) and 0.8 .. 7.0 of ~81 (fp8)):
#   every request grouped, P = 2048:  bf16 1 x 64 0.81, 2 x 32 0.83, 4 x 16 0.84, 8 x 8 0.83, 16 x 4 0.95
#                                     fp8  1 x 64 0.94, 2 x 32 0.95, 4 x 16 0.95, 8 x 8 0.93, 16 x 4 1.06
#   2 x 32 with two lengths:          bf16 2048 / 3072 0.86, 1536 / 2560 0.92, 1024 / 3072 1.01
#                                     fp8  2048 / 3072 1.02, 1536 / 2560 1.05, 1024 / 3072 1.11
#   requests in no group:             bf16 2 x 24 + 16 1.20, 2 x 31 + 2 1.18;  fp8 1.34, 1.26
# MIN_MEMBERS: the smallest measured members per group at which the grouped call beats the plain one by more than twice the
# plain call's spread, per cache kind (bf16: 4 members 139.0 against 146.9 +- 1.6 us; fp8: 4 lose, 8 win 77.0 against 82.5
# +- 1.4).  What the group size does not decide: the suffix launch lasts as long as its longest request, so ONE request
# that keeps (nearly) its whole context — a request in no group, or a group with a short prefix beside long ones — costs
# the call all it saved, and the prefix launch on top (two ungrouped requests of 64: 1.18).  MAX_SUFFIX_FRACTION: the
# largest measured (longest range left to a request behind its prefix) / (longest context) at which the call still wins:
# bf16 2688 / 4224 (1536 / 2560: 0.92; 3200 / 4224 does not win); fp8 2176 / 4224, and only with one length for all groups
# (MAX_LEN_SPREAD_FP8: the smallest measured difference, 1024 tokens, loses).  A step with a long request in no group is
# therefore REFUSED; one whose ungrouped requests are short against the longest context is taken.
PREFIX_GROUPS_MIN_MEMBERS = 4
PREFIX_GROUPS_MIN_MEMBERS_FP8 = 8
PREFIX_GROUPS_MAX_SUFFIX_FRACTION = 0.64       # 2688 / 4224 = 0.636 wins, 3200 / 4224 = 0.758 does not
PREFIX_GROUPS_MAX_SUFFIX_FRACTION_FP8 = 0.52   # 2176 / 4224 = 0.515, the one ratio measured to win
PREFIX_GROUPS_MAX_LEN_SPREAD_FP8 = 31          # tokens between the longest and the shortest group prefix (one served length)


def host_block_table(block_table):
    """The step's block table as a host numpy array [requests, blocks], or None.  Accepts a numpy array (the stand-in's
    `input_batch.block_table`), an object with `get_numpy_array()` or `block_table_np` (vLLM 0.9.2's BlockTable; names
    recalled from 0.9.2, parity unpinned: DESIGN section 3), or a one-element sequence of such (its MultiGroupBlockTable
    with one kv-cache group).  More than one kv-cache group, or anything else, is None: no groups."""
    import numpy as np
    for _ in range(2):
        if isinstance(block_table, np.ndarray):
            return block_table if block_table.ndim == 2 else None
        get = getattr(block_table, "get_numpy_array", None)
        if callable(get):
            block_table = get()
            continue
        inner = getattr(block_table, "block_table_np", None)
        if inner is not None:
            block_table = inner
            continue
        tables = getattr(block_table, "block_tables", block_table)
        if isinstance(tables, (list, tuple)) and len(tables) == 1:
            block_table = tables[0]
            continue
        return None
    return block_table if isinstance(block_table, np.ndarray) and block_table.ndim == 2 else None


def prefix_groups(block_table_np, num_computed, q_lens, block_size, num_kv_heads, fp8):
    """Which requests of a verify step read a shared prefix once, in groups (ops.PrefixGroups' `req_group` and
    `group_prefix_len`), or None for the plain call: the whole decision, on host arrays alone.  Requests are bucketed by
    their first SHARED_PREFIX_MIN_LEN // block_size block ids (prefix caching gives requests with the same leading tokens
    the same pages); a bucket's shared length is its longest run of equal leading block-table columns times the block
    size, capped by its members' smallest computed-token count (so that every query token lies behind it).  Kept: groups
    of at least PREFIX_GROUPS_MIN_MEMBERS (_FP8) members and SHARED_PREFIX_MIN_LEN tokens (never fewer than 32), at most
    PREFIX_GROUPS_MAX of them, largest first — the rest stay ungrouped — and only when the grouped requests x
    `num_kv_heads` reach SHARED_PREFIX_MIN_ITEMS (_FP8), no request keeps more than PREFIX_GROUPS_MAX_SUFFIX_FRACTION
    (_FP8) of the longest context behind its prefix (a request in no group keeps all of its own) and, with an fp8 cache,
    the groups' served lengths are within PREFIX_GROUPS_MAX_LEN_SPREAD_FP8 of each other.  Correctness never depends on
    the answer."""
    import numpy as np
    bt = host_block_table(block_table_np)
    if bt is None or num_computed is None or q_lens is None or not block_size:
        return None
    B = len(q_lens)
    block_size = int(block_size)
    if B == 0 or bt.shape[0] < B or len(num_computed) < B:
        return None
    bt = bt[:B]
    computed = np.asarray(num_computed)[:B].astype(np.int64)
    min_len = max(SHARED_PREFIX_FLOOR, SHARED_PREFIX_MIN_LEN)
    n_key = max(1, min_len // block_size)
    if bt.shape[1] < n_key:
        return None
    min_members = max(1, PREFIX_GROUPS_MIN_MEMBERS_FP8 if fp8 else PREFIX_GROUPS_MIN_MEMBERS)
    buckets = {}
    for i in np.flatnonzero(computed >= min_len):
        buckets.setdefault(bt[i, :n_key].tobytes(), []).append(int(i))
    found = []
    for members in buckets.values():
        if len(members) < min_members:
            continue
        rows = bt[members]
        differ = np.flatnonzero((rows != rows[0]).any(axis=0))
        run = int(differ[0]) if differ.size else rows.shape[1]
        length = min(run * block_size, int(computed[members].min()))
        if length >= min_len:
            found.append((members, length))
    found.sort(key=lambda f: (-len(f[0]), f[0][0]))
    found = found[:PREFIX_GROUPS_MAX]
    grouped = sum(len(m) for m, _ in found)
    if grouped * int(num_kv_heads or _MEASURED_KV_HEADS) < (SHARED_PREFIX_MIN_ITEMS_FP8 if fp8 else SHARED_PREFIX_MIN_ITEMS):
        return None
    if not found:
        return None
    req_group = np.full(B, -1, dtype=np.int32)
    begin = np.zeros(B, dtype=np.int64)
    for g, (members, length) in enumerate(found):
        req_group[members] = g
        begin[members] = length & ~31
    # the measured limits of the win (above): the longest range any request keeps, and (fp8) one length for all groups
    seq = computed + np.asarray(q_lens, dtype=np.int64)
    fraction = PREFIX_GROUPS_MAX_SUFFIX_FRACTION_FP8 if fp8 else PREFIX_GROUPS_MAX_SUFFIX_FRACTION
    if int((seq - begin).max()) > fraction * int(seq.max()):
        return None
    served = [length & ~31 for _, length in found]
    if fp8 and max(served) - min(served) > PREFIX_GROUPS_MAX_LEN_SPREAD_FP8:
        return None
    return req_group, [length for _, length in found]

