"""Fixtures for the grouped shared-prefix attention call, aic_verify_attention_prefix_groups / ops.verify_attention(...,
prefix_groups=): steps whose requests fall into groups that each hold their first tokens in the SAME physical pages, beside
requests that share nothing.

share_in_groups      shared_prefix_fixtures.share_prefix per group: an attention_fixtures.planted_case whose group members
                     take their leader's pages below the group's length.
grouped_marked_case  the single-marked-key probe of shared_prefix_fixtures.marked_key_case with a shared length per
                     request: q = 0, V zero except at key position t, so a row at position p >= t must return 1 / (p + 1)
                     and a row below it zero.  shared_prefix_fixtures.marked_reference is its mutable restatement (it
                     reads V through the block table, whatever is shared)."""
from types import SimpleNamespace

import numpy as np
import torch

from shared_prefix_fixtures import ATOL, RTOL, bar, marked_reference  # noqa: F401  (re-exported for the tests)

# The seam probe's step: groups A (32 tokens) and B (64), members interleaved, request 2 in no group and shorter than either
# prefix; request 1 has ctx - q_len == 64 exactly.  Every context <= 92: a row at position p that counts key t twice moves
# by p / ((p + 1) (p + 2)), ten times the bar up to p = 92 and no further (tests/test_shared_prefix_host.py).
SEAM_REQ_GROUP, SEAM_GROUP_LEN = [0, 1, -1, 0, 1], [32, 64]
SEAM_Q_LENS, SEAM_CTXS = [1, 2, 3, 5, 20], [40, 66, 20, 60, 92]
SEAM_KEYS = [31, 32, 63, 64]          # P_g - 1 and P_g of both groups


def leaders(req_group, n_groups):
    """The first member of every group."""
    return [next(i for i, g in enumerate(req_group) if g == k) for k in range(n_groups)]


def share_in_groups(case, req_group, group_len):
    """`case` (attention_fixtures.planted_case) with, for every member i of group g, bt[i, :ceil(group_len[g] / bs)] =
    the leader's (the group's first member), in place; returns the case with `req_group`, `group_len` and `leader`.
    The planted keys are position-coded, so K is unchanged; V below the length becomes the leader's for the group.
    Requires what the kernel's call requires: every member keeps its query tokens behind its group's length."""
    assert len(req_group) == len(case.q_lens)
    lead = leaders(req_group, len(group_len))
    for i, g in enumerate(req_group):
        if g < 0:
            continue
        assert case.ctxs[i] - case.q_lens[i] >= group_len[g], f"request {i}: a query token inside its group's prefix"
        n = -(-group_len[g] // case.bs)
        case.bt[i, :n] = case.bt[lead[g], :n]
    case.req_group, case.group_len, case.leader = list(req_group), list(group_len), lead
    return case


def grouped_marked_case(t, q_lens, ctxs, Hq, Hkv, D, bs, req_group, group_len, seed=0, dtype=torch.bfloat16):
    """The probe described above.  Members of group g name the same pages in their first ceil(group_len[g] / bs)
    block-table columns; every other page is a request's own.  Returns a namespace with the fields
    attention_fixtures.oracle() reads, plus `pos` [T] (every token's position), `expected` [T, Hq, D] (the closed form),
    `t`, `req_group`, `group_len` and `leader`."""
    gen = torch.Generator().manual_seed(seed)
    B = len(q_lens)
    lead = leaders(req_group, len(group_len))
    nblk = [(c + bs - 1) // bs for c in ctxs]
    n_sh = [0 if g < 0 else -(-group_len[g] // bs) for g in req_group]
    for i, g in enumerate(req_group):
        assert nblk[i] >= n_sh[i] and (g < 0 or ctxs[i] - q_lens[i] >= group_len[g])
    own = [n if (g < 0 or lead[g] == i) else n - s for i, (n, s, g) in enumerate(zip(nblk, n_sh, req_group))]
    total = sum(own) + 2
    perm = torch.randperm(total, generator=gen).to(torch.int32)
    bt = torch.full((B, max(nblk) + 1), int(perm[-1]), dtype=torch.int32)
    kc = torch.randn(total, bs, Hkv, D, generator=gen)      # q = 0: the keys do not matter, as long as they are finite
    vc = torch.zeros(total, bs, Hkv, D)
    k = 0
    for i in sorted(range(B), key=lambda i: (req_group[i] >= 0 and lead[req_group[i]] != i, i)):   # leaders first
        g = req_group[i]
        first = 0
        if g >= 0 and lead[g] != i:
            first = n_sh[i]
            bt[i, :first] = bt[lead[g], :first]
        bt[i, first:nblk[i]] = perm[k:k + nblk[i] - first]
        k += nblk[i] - first
    for i, n in enumerate(nblk):
        if t < n * bs:
            vc[int(bt[i, t // bs]), t % bs] = 1.0
    T = int(sum(q_lens))
    pos = torch.cat([torch.arange(c - q, c) for q, c in zip(q_lens, ctxs)])
    val = torch.where(pos >= t, 1.0 / (pos + 1).double(), torch.zeros(T, dtype=torch.float64))
    expected = val.view(T, 1, 1).expand(T, Hq, D).float().contiguous()
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    return SimpleNamespace(q=torch.zeros(T, Hq, D, dtype=dtype), kc=kc.to(dtype), vc=vc.to(dtype), bt=bt, qsl=qsl, ks=None,
                           vs=None, q_lens=list(q_lens), ctxs=list(ctxs), Hq=Hq, Hkv=Hkv, D=D, bs=bs, window=0, sinks=None,
                           scale=D ** -0.5, pos=pos, expected=expected, t=t, req_group=list(req_group),
                           group_len=list(group_len), leader=lead)
