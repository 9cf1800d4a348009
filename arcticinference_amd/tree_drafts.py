"""Host layout of a step's tree-shaped drafts (numpy only, no device, no torch).

The suffix trees answer tree-mode queries as `SuffixSpecResult(token_ids, parents)`: draft nodes in emission order,
`parents[c]` the index of node c's parent in `token_ids`, or -1 for a child of the match point.  The verify kernels
(aic_verify_attention_tree, aic_rejection_tree_greedy, aic_kv_compact_paths) want the ROOTED form of a request with
q_len = 1 + n query tokens: token 0 is the root (the last accepted token), tokens 1 .. n the draft nodes, parent[0] = -1
and parent[t] in [0, t - 1] — both of the result's arrays shifted by one.  Per token they also want the ancestor mask
(bit u set: query token u is token t itself or one of its ancestors, the root included) and the depth, which is the
node's rotary position relative to the root.

The reference flattens a tree to its best path before verification (arctic_inference/vllm/model_runner.py:734-740);
here the whole tree travels as the flat draft list of the request.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

MAX_TREE_DRAFT = 32   # vllm.v1.sample.rejection_sampler.MAX_SPEC_LEN: draft nodes of one request


class TreeLayout(NamedTuple):
    tokens: np.ndarray           # int32 [T]: token 0 of a request = `root_tokens[i]` (or -1), then its draft nodes
    parents: np.ndarray          # int32 [T]: rooted in-request indices, -1 at a request's root
    masks: np.ndarray            # uint64 [T]: ancestor-or-self bits over the request's query tokens
    depths: np.ndarray           # int32 [T]: 0 at the root
    query_start_loc: np.ndarray  # int32 [B + 1]
    q_lens: np.ndarray           # int32 [B]


def chain_masks(q_len: int) -> np.ndarray:
    """The lower-triangular masks of a chain of `q_len` query tokens: exactly the causal rule."""
    if not 0 <= q_len <= 64:
        raise ValueError(f"q_len {q_len} outside 0 .. 64 (one mask word)")
    t = np.arange(q_len, dtype=np.uint64)
    return ((np.uint64(2) << t) - np.uint64(1)).astype(np.uint64) if q_len else np.zeros(0, dtype=np.uint64)


def rooted_parents(parents: Sequence[int]) -> np.ndarray:
    """`SuffixSpecResult.parents` (-1 = child of the match point) -> rooted form with the root in front.  ValueError
    unless every parent precedes its child."""
    p = np.asarray(parents, dtype=np.int64).reshape(-1)
    idx = np.arange(p.size)
    if p.size and (int(p.min()) < -1 or bool((p >= idx).any())):
        bad = int(np.flatnonzero((p < -1) | (p >= idx))[0])
        raise ValueError(f"draft node {bad}: parent {int(p[bad])} must be -1 or an earlier node (parent before child)")
    return np.concatenate([[-1], p + 1]).astype(np.int32)


def ancestor_masks(rooted: np.ndarray):
    """(uint64 masks, int32 depths) of one request from its rooted parents: mask[t] = bit t | mask[parent[t]] — the
    transitive closure in one pass, because a parent precedes its child."""
    n = int(rooted.size)
    if n > 64:
        raise ValueError(f"{n} query tokens: one mask word covers 64")
    masks = [0] * n
    depths = [0] * n
    for t in range(n):
        p = int(rooted[t])
        masks[t] = (1 << t) | (masks[p] if p >= 0 else 0)
        depths[t] = depths[p] + 1 if p >= 0 else 0
    return np.array(masks, dtype=np.uint64), np.array(depths, dtype=np.int32)


def build_tree_layout(trees: Sequence, root_tokens: Optional[Sequence[int]] = None,
                      max_draft: int = MAX_TREE_DRAFT, strict: bool = False) -> TreeLayout:
    """The step's layout from per-request `(token_ids, parents)` pairs (or objects with those attributes) in
    SuffixSpecResult form.  A request without a draft is `([], [])`: q_len = 1.  Results longer than `max_draft` nodes are
    cut to their first `max_draft` (emission order, so the cut is still a tree) the way the runner cuts paths to
    MAX_SPEC_LEN; `strict=True` raises instead.  ValueError: arrays of different lengths, a parent that does not precede
    its child, siblings carrying the same token, more than 32 nodes under `strict`."""
    if not 0 <= max_draft <= MAX_TREE_DRAFT:
        raise ValueError(f"max_draft {max_draft} outside 0 .. {MAX_TREE_DRAFT}")
    toks, pars, masks, depths, qlens = [], [], [], [], []
    for i, tr in enumerate(trees):
        ids, par = (tr.token_ids, tr.parents) if hasattr(tr, "token_ids") else tr
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        par = np.asarray(par, dtype=np.int64).reshape(-1)
        if ids.size != par.size:
            raise ValueError(f"request {i}: {ids.size} token ids, {par.size} parents")
        if ids.size > max_draft:
            if strict:
                raise ValueError(f"request {i}: {ids.size} draft nodes, at most {max_draft}")
            ids, par = ids[:max_draft], par[:max_draft]
        try:
            rooted = rooted_parents(par)
        except ValueError as e:
            raise ValueError(f"request {i}: {e}") from None
        key = par * (1 << 32) + ids
        if np.unique(key).size != key.size:
            raise ValueError(f"request {i}: two children of one node carry the same token")
        m, d = ancestor_masks(rooted)
        root = -1 if root_tokens is None else int(root_tokens[i])
        toks.append(np.concatenate([[root], ids]))
        pars.append(rooted)
        masks.append(m)
        depths.append(d)
        qlens.append(1 + ids.size)
    q_lens = np.asarray(qlens, dtype=np.int32)
    qsl = np.zeros(len(qlens) + 1, dtype=np.int32)
    np.cumsum(q_lens, out=qsl[1:])
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt))
    return TreeLayout(cat(toks, np.int32), cat(pars, np.int32), cat(masks, np.uint64), cat(depths, np.int32), qsl, q_lens)


def positions(layout: TreeLayout, seq_lens: Sequence[int]) -> np.ndarray:
    """int64 [T]: the rotary position of every query token, base + depth with base = seq_len - q_len per request
    (`seq_lens` counts the step's query tokens, as the attention call's does)."""
    base = np.asarray(seq_lens, dtype=np.int64).reshape(-1) - layout.q_lens
    if base.size != layout.q_lens.size or (base.size and int(base.min()) < 0):
        raise ValueError("seq_lens: one length per request, each at least the request's q_len")
    return np.repeat(base, layout.q_lens) + layout.depths
