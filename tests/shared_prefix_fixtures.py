"""Fixtures for the shared-prefix (cascade) attention call, aic_verify_attention_prefix / ops.verify_attention(...,
shared_prefix_len, prefix_block_table): steps whose requests hold their first P tokens in the SAME physical pages.

share_prefix       an attention_fixtures.planted_case whose requests share request 0's pages below P.
marked_key_case    the single-marked-key probe of the seam at P: q = 0, so every visible key of a row has weight 1, and
                   V is zero except at key position t, where it is 1 in every head and dimension.  A row at position
                   p >= t must return 1 / (p + 1), a row at p < t zero.  A key that is dropped at the seam (or counted on
                   both sides of it) moves every such row by about 1 / p: at contexts <= 92, ten times the project's bar.
marked_reference   float64 restatement on that case with the weight of key t movable (0: dropped, 2: counted twice)."""
from types import SimpleNamespace

import numpy as np
import torch

ATOL, RTOL = 1e-3, 2 ** -8


def share_prefix(case, P):
    """`case` (attention_fixtures.planted_case) with bt[i, :P // bs] = bt[0, :P // bs] for every request, in place; returns
    the case.  The planted keys are position-coded, so K is unchanged; V below P becomes request 0's for everybody.
    Requires what the kernel's call requires: every request keeps its query tokens behind P."""
    n = P // case.bs
    assert n > 0 and n * case.bs == P, "whole pages"
    for ql, ctx in zip(case.q_lens, case.ctxs):
        assert ctx - ql >= P, "a query token inside the shared prefix"
    case.bt[:, :n] = case.bt[0, :n]
    case.shared_len = P
    case.prefix_table = case.bt[0, :n].clone()
    return case


def marked_key_case(t, q_lens, ctxs, Hq, Hkv, D, bs, shared_len, seed=0, dtype=torch.bfloat16):
    """The probe described above.  The first ceil(shared_len / bs) block-table columns of every request name the same
    pages.  Returns a namespace with the fields attention_fixtures.oracle() reads, plus `pos` [T] (every token's
    position), `expected` [T, Hq, D] (the closed form), `prefix_table` and `shared_len`."""
    g = torch.Generator().manual_seed(seed)
    B = len(q_lens)
    n_sh = -(-shared_len // bs)
    nblk = [(c + bs - 1) // bs for c in ctxs]
    assert all(n >= n_sh for n in nblk) and all(c - q >= shared_len for q, c in zip(q_lens, ctxs))
    total = n_sh + sum(n - n_sh for n in nblk) + 2
    perm = torch.randperm(total, generator=g).to(torch.int32)
    bt = torch.full((B, max(nblk) + 1), int(perm[-1]), dtype=torch.int32)
    k = n_sh
    kc = torch.randn(total, bs, Hkv, D, generator=g)      # q = 0: the keys do not matter, as long as they are finite
    vc = torch.zeros(total, bs, Hkv, D)
    for i, n in enumerate(nblk):
        bt[i, :n_sh] = perm[:n_sh]
        bt[i, n_sh:n] = perm[k:k + n - n_sh]
        k += n - n_sh
        if t < n * bs:
            vc[int(bt[i, t // bs]), t % bs] = 1.0
    T = int(sum(q_lens))
    pos = torch.cat([torch.arange(c - q, c) for q, c in zip(q_lens, ctxs)])
    val = torch.where(pos >= t, 1.0 / (pos + 1).double(), torch.zeros(T, dtype=torch.float64))
    expected = val.view(T, 1, 1).expand(T, Hq, D).float().contiguous()
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    return SimpleNamespace(q=torch.zeros(T, Hq, D, dtype=dtype), kc=kc.to(dtype), vc=vc.to(dtype), bt=bt, qsl=qsl, ks=None,
                           vs=None, q_lens=list(q_lens), ctxs=list(ctxs), Hq=Hq, Hkv=Hkv, D=D, bs=bs, window=0, sinks=None,
                           scale=D ** -0.5, pos=pos, expected=expected, t=t, shared_len=shared_len,
                           prefix_table=bt[0, :n_sh].clone())


def marked_reference(c, weight_of_t=1.0):
    """out [T, Hq, D] in float64 with q = 0 taken at its word (every visible key weighs 1) except key t, which weighs
    `weight_of_t`: 1 is the attention itself, 0 a key lost at the seam, 2 a key both phases counted.  V is read through
    the block table."""
    G = c.Hq // c.Hkv
    out = torch.zeros(int(c.qsl[-1]), c.Hq, c.D, dtype=torch.float64)
    for i, ctx in enumerate(c.ctxs):
        q0, q1 = int(c.qsl[i]), int(c.qsl[i + 1])
        blocks = c.bt[i, :(ctx + c.bs - 1) // c.bs].long()
        V = c.vc[blocks].reshape(-1, c.Hkv, c.D)[:ctx].double().repeat_interleave(G, dim=1)   # [ctx, Hq, D]
        for n in range(q1 - q0):
            p = ctx - (q1 - q0) + n
            w = torch.ones(p + 1, dtype=torch.float64)
            if c.t <= p:
                w[c.t] = weight_of_t
            out[q0 + n] = torch.einsum("k,khd->hd", w, V[:p + 1]) / w.sum()
    return out


def bar(want):
    """The project's tolerance at `want`."""
    return ATOL + RTOL * want.abs()
