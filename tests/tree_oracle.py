"""Test-side restatements for tree-shaped drafts (arcticinference_amd/tree_drafts.py, aic_verify_attention_tree,
aic_rejection_tree_greedy, aic_kv_compact_paths), and the fixtures their tests share.

Nothing here is a reference implementation from elsewhere: the reference project verifies paths only
(arctic_inference/vllm/model_runner.py:734-740).  What is pinned is parity with the chain oracles on chains
(oracle.spec_oracle.verify_attention / rejection_greedy) and the rules stated in include/arctic_hip.h.

Discriminating fixture.  With random Q / K / V one key carries ~1/ctx of a row's weight, so a wrong mask bit hides under
the tolerance.  `plant` gives, for chosen (token t, node u) pairs of a request, the key at base + u the value
K = c q_row with c = AMP / (sm_scale |q_row|^2): row (t, one query head per kv head) scores AMP = 40 nats against it and
~N(0, AMP^2 / D) against everything else.  u is either invisible to t (a sibling, a descendant, a later non-ancestor) —
then one wrong bit moves the row onto V[u] — or a visible ancestor (or t itself) — then one wrong bit moves it off."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import spec_oracle as O

AMP = 40.0
K_SCALE, V_SCALE = 0.05, 0.021     # fp8 cache: planted keys reach |K| ~ 16 -> |K / k_scale| <= 448 (e4m3)


# ---- trees -------------------------------------------------------------------------------------------------------------
def chain(n):
    """(token_ids, parents) of an n-node chain in SuffixSpecResult form."""
    return list(range(100, 100 + n)), list(range(-1, n - 1))


def random_tree(n, rng, bushy=0.5):
    """n draft nodes in SuffixSpecResult form: a node's parent is the previous node with probability 1 - bushy, else any
    earlier node or the match point.  Tokens are distinct, so siblings are."""
    par = [c - 1 if rng.random() >= bushy else int(rng.integers(-1, c)) for c in range(n)]
    return [int(x) for x in rng.permutation(1000)[:n]], par


def star(n):
    """the match point with n children"""
    return list(range(200, 200 + n)), [-1] * n


def naive_masks(rooted):
    """Ancestor-or-self masks by walking up from every node: the slow restatement."""
    out = []
    for t in range(len(rooted)):
        m, u = 0, t
        while u >= 0:
            m |= 1 << u
            u = int(rooted[u])
        out.append(m)
    return np.array(out, dtype=np.uint64)


# ---- attention ---------------------------------------------------------------------------------------------------------
def tree_attention(q, k_cache, v_cache, block_table, seq_lens, query_start_loc, masks, sm_scale, k_scale=1.0, v_scale=1.0,
                   sinks=None, dtype=torch.float32):
    """fp32 attention with an explicit mask: key j of request i is visible to its token t iff j < base, or
    base <= j < seq_len and bit j - base of masks[q0 + t] is set (base = seq_len - q_len)."""
    T, Hq, D = q.shape
    _, bs, Hkv, _ = k_cache.shape
    G = Hq // Hkv
    out = torch.zeros(T, Hq, D, dtype=dtype)
    for i, ctx in enumerate(seq_lens):
        q0, q1 = int(query_start_loc[i]), int(query_start_loc[i + 1])
        ql = q1 - q0
        if ql == 0:
            continue
        base = ctx - ql
        blocks = block_table[i, :(ctx + bs - 1) // bs].long()
        K = k_cache[blocks].reshape(-1, Hkv, D)[:ctx].to(dtype) * k_scale
        V = v_cache[blocks].reshape(-1, Hkv, D)[:ctx].to(dtype) * v_scale
        s = torch.einsum("qhd,khd->hqk", q[q0:q1].to(dtype), K.repeat_interleave(G, dim=1)) * sm_scale
        vis = torch.ones(ql, ctx, dtype=torch.bool)
        for t in range(ql):
            m = int(masks[q0 + t])
            vis[t, base:] = torch.tensor([(m >> u) & 1 == 1 for u in range(ql)])
        s = s.masked_fill(~vis.unsqueeze(0), float("-inf"))
        if sinks is not None:
            s = torch.cat([s, sinks.to(dtype).view(Hq, 1, 1).expand(Hq, ql, 1)], dim=-1)
        p = torch.softmax(s, dim=-1)[..., :ctx]
        out[q0:q1] = torch.einsum("hqk,khd->qhd", p, V.repeat_interleave(G, dim=1))
    return out


def relation(rooted, t, u):
    """How node u stands to node t: 'self', 'ancestor', 'descendant', 'sibling' (same parent), 'later' / 'earlier'
    (an unrelated node after / before t)."""
    if u == t:
        return "self"
    a = t
    while a >= 0:
        a = int(rooted[a])
        if a == u:
            return "ancestor"
    a = u
    while a >= 0:
        a = int(rooted[a])
        if a == t:
            return "descendant"
    if rooted[u] == rooted[t]:
        return "sibling"
    return "later" if u > t else "earlier"


def pick_plants(rooted, rng, want=("sibling", "descendant", "later", "ancestor", "self"), last_self=False):
    """[(t, u, relation)] with distinct t and distinct u: for every relation in `want` that the tree still has a free pair
    for, one pair (the first found in a random order).  `last_self`: the last node against itself first (the highest bit
    of the request's mask words)."""
    n = len(rooted)
    used_t, used_u, out = set(), set(), []
    if last_self and n > 1:
        out.append((n - 1, n - 1, "self"))
        used_t.add(n - 1)
        used_u.add(n - 1)
    for rel in want:
        order = [int(x) for x in rng.permutation(n)]
        hit = next(((t, u) for t in order for u in order
                    if t > 0 and t not in used_t and u not in used_u and relation(rooted, t, u) == rel), None)
        if hit:
            out.append((hit[0], hit[1], rel))
            used_t.add(hit[0])
            used_u.add(hit[1])
    return out


def attention_case(trees, ctxs, Hq, Hkv, D, bs, seed, dtype=torch.bfloat16, fp8=False, plant=True, last_self=False):
    """A step of len(trees) requests with random q / K / V behind a shuffled block table, laid out by
    tree_drafts.build_tree_layout, with the planted keys described above.  ctxs count the query tokens.  Returns a
    namespace: q, kc, vc, bt, lay (the TreeLayout), ctxs, ks / vs, scale, plants [(request, t, u, relation)], and
    rows [(token row of the call, query head, token row's request-local u)] — the rows a plant concerns."""
    from arcticinference_amd import tree_drafts as TD
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    lay = TD.build_tree_layout(trees)
    G = Hq // Hkv
    nblk = [(c + bs - 1) // bs for c in ctxs]
    nb = sum(nblk) + 3
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(ctxs), max(nblk), dtype=torch.int32)
    p = 0
    for i, k in enumerate(nblk):
        bt[i, :k] = perm[p:p + k].to(torch.int32)
        p += k
    kc = torch.randn(nb, bs, Hkv, D, generator=g)
    vc = torch.randn(nb, bs, Hkv, D, generator=g)
    q = torch.randn(int(lay.tokens.size), Hq, D, generator=g).to(dtype)
    scale = D ** -0.5
    plants, rows = [], []
    if plant:
        for i, ctx in enumerate(ctxs):
            q0, ql = int(lay.query_start_loc[i]), int(lay.q_lens[i])
            if ql < 2:
                continue
            rooted = lay.parents[q0:q0 + ql]
            for t, u, rel in pick_plants(rooted, rng, last_self=last_self and ql == 33):
                key = ctx - ql + u
                page, off = int(bt[i, key // bs]), key % bs
                for h in range(Hkv):
                    hq = h * G + t % G
                    qr = q[q0 + t, hq].float()
                    kc[page, off, h] = qr * (AMP / (scale * float(qr @ qr)))
                    rows.append((q0 + t, hq, u))
                plants.append((i, t, u, rel))
    ks = vs = None
    if fp8:
        ks, vs = K_SCALE, V_SCALE
        kc, vc = O.fp8_sat(kc / ks, "e4m3"), O.fp8_sat(vc / vs, "e4m3")
    else:
        kc, vc = kc.to(dtype), vc.to(dtype)
    return SimpleNamespace(q=q, kc=kc, vc=vc, bt=bt, lay=lay, ctxs=list(ctxs), ks=ks, vs=vs, scale=scale, plants=plants,
                           rows=rows, Hq=Hq, Hkv=Hkv, D=D, bs=bs)


def case_oracle(c, masks=None, sinks=None, dtype=torch.float32):
    sc = dict(k_scale=c.ks, v_scale=c.vs) if c.ks is not None else {}
    return tree_attention(c.q, c.kc, c.vc, c.bt, c.ctxs, c.lay.query_start_loc, c.lay.masks if masks is None else masks,
                          c.scale, sinks=sinks, dtype=dtype, **sc)


# ---- acceptance --------------------------------------------------------------------------------------------------------
def tree_accept(logits, tokens, parents, query_start_loc, width):
    """The greedy walk of aic_rejection_tree_greedy on the values as stored: (out [B, width], num_accepted, last_token,
    hidden_index, path [B, width])."""
    B = len(query_start_loc) - 1
    out = np.full((B, width), -1, dtype=np.int32)
    path = np.full((B, width), -1, dtype=np.int32)
    nacc = np.zeros(B, dtype=np.int32)
    last = np.full(B, -1, dtype=np.int32)
    hidx = np.zeros(B, dtype=np.int32)
    am = torch.argmax(logits.float(), dim=-1).numpy() if logits.numel() else np.zeros(0, np.int64)
    for i in range(B):
        q0, q1 = int(query_start_loc[i]), int(query_start_loc[i + 1])
        cur, d = 0, 0
        while q1 > q0:
            a = int(am[q0 + cur])
            out[i, d], path[i, d], last[i] = a, cur, a
            d += 1
            nxt = next((c for c in range(1, q1 - q0) if parents[q0 + c] == cur and tokens[q0 + c] == a), None)
            if nxt is None:
                break
            cur = nxt
        nacc[i], hidx[i] = d, q0 + cur
    return out, nacc, last, hidx, path


# ---- compaction --------------------------------------------------------------------------------------------------------
def compact(cache, block_table, seq_lens, q_lens, path, num_accepted):
    """numpy restatement of aic_kv_compact_paths on one cache [nb, bs, ...] (any dtype, viewed as bytes by the caller):
    new[base + d] = old[base + path[d]] for d < num_accepted."""
    old = cache.copy()
    bs = cache.shape[1]
    for i, (ctx, ql) in enumerate(zip(seq_lens, q_lens)):
        base = int(ctx) - int(ql)
        for d in range(int(num_accepted[i])):
            src, dst = base + int(path[i, d]), base + d
            cache[int(block_table[i, dst // bs]), dst % bs] = old[int(block_table[i, src // bs]), src % bs]
    return cache
