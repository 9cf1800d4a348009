"""GPU: aic_kv_compact_paths (csrc/kv_compact.hip) byte for byte against its numpy restatement (tests/tree_oracle.py),
and the composed step — write node K/V, tree-attend, accept, compact, decode one token — whose claim is the feature's:
afterwards the cache is what decoding the accepted chain alone would have left.  The reference has no counterpart (it
verifies paths only, arctic_inference/vllm/model_runner.py:734-740)."""
import numpy as np
import pytest
import torch

import tree_oracle as TO
from oracle import spec_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = 1e-3, 2 ** -8


def _ops():
    from arcticinference_amd import ops
    return ops


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy()


def _paths(rows, W):
    path = np.full((len(rows), W), -1, dtype=np.int32)
    for i, r in enumerate(rows):
        path[i, :len(r)] = r
    return path, np.array([len(r) for r in rows], dtype=np.int32)


@pytest.mark.parametrize("dtype,Hkv,D", [(torch.bfloat16, 2, 128), (torch.float8_e4m3fn, 8, 128), (torch.float16, 3, 64)],
                         ids=["bf16", "fp8", "f16-d64-3heads"])
def test_compaction_is_the_gather(dtype, Hkv, D):
    ops = _ops()
    bs, L = 16, 3
    # q_len, context (query tokens counted), accepted path.  request 0: the overlapping move of the header ([0, 2, 3]);
    # 1: across a page border (base 27: slots 27 .. 47), a long strictly increasing path; 2: n_path = 1; 3: the identity
    # (nothing moves); 4: base 0, the path ends at the last node; 5: q_len 1.
    reqs = [(5, 40, [0, 2, 3]), (21, 48, [0, 3, 4, 9, 15, 16, 20]), (9, 100, [0]), (4, 33, [0, 1, 2]),
            (33, 33, [0, 5, 9, 17, 31, 32]), (1, 7, [0])]
    q_lens, ctxs = [r[0] for r in reqs], [r[1] for r in reqs]
    td = ops.TreeDrafts([TO.chain(n - 1) for n in q_lens], DEV)         # only the geometry matters here
    W = td.max_q_len
    path, nacc = _paths([r[2] for r in reqs], W)
    g = torch.Generator().manual_seed(1)
    nblk = [(c + bs - 1) // bs for c in ctxs]
    nb = sum(nblk) + 2
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(reqs), max(nblk), dtype=torch.int32)
    p = 0
    for i, k in enumerate(nblk):
        bt[i, :k] = perm[p:p + k].to(torch.int32)
        p += k
    def rand_cache():
        raw = torch.randint(0, 256, (nb, bs, Hkv, D * torch.empty(0, dtype=dtype).element_size()), generator=g, dtype=torch.int32)
        return raw.to(torch.uint8).view(dtype).contiguous()
    kcs, vcs = [rand_cache() for _ in range(L)], [rand_cache() for _ in range(L)]
    dk, dv = [c.to(DEV) for c in kcs], [c.to(DEV) for c in vcs]
    ops.compact_accepted_paths(dk, dv, bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV), td,
                               torch.from_numpy(path).to(DEV), torch.from_numpy(nacc).to(DEV))
    torch.cuda.synchronize()
    moved = 0
    for host, dev in zip(kcs + vcs, dk + dv):
        before = _bytes(host).reshape(nb, bs, -1)
        want = TO.compact(before.copy(), bt.numpy(), ctxs, q_lens, path, nacc)
        got = _bytes(dev).reshape(nb, bs, -1)
        assert np.array_equal(got, want)                                 # the destination slots AND everything else
        moved += int((want != before).any(axis=-1).sum())
    # 2 + 6 + 5 destination slots differ from before in each of the 2 L caches (random bytes: a row never equals another)
    assert moved == 2 * L * (2 + 6 + 5)


def test_write_attend_accept_compact_decode():
    """The composed step.  K/V of every tree node are written at base + t by the ordinary bulk write, the tree call
    attends, planted logits accept a path through each tree, the caches are compacted, and the NEXT step — the plain
    verify_attention with q_len = 1 on a new token — must meet the bar against the oracle on a cache built from the
    accepted chain alone (the old context, then the accepted nodes' K/V in path order, then the new token)."""
    ops = _ops()
    Hq, Hkv, D, bs, L = 8, 2, 128, 16, 2
    rng = np.random.default_rng(2)
    g = torch.Generator().manual_seed(3)
    trees = [TO.random_tree(32, rng, 0.6), ([], []), TO.random_tree(9, rng, 0.7), TO.chain(4)]
    td = ops.TreeDrafts(trees, DEV)
    lay = td.layout
    B, T = td.batch, td.num_tokens
    bases = [150, 31, 15, 64]                                             # old context lengths
    ctxs = [b + int(n) for b, n in zip(bases, lay.q_lens)]
    nblk = [(c + 1 + bs - 1) // bs for c in ctxs]                         # room for the next step's token
    nb = sum(nblk) + 2
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    p = 0
    for i, k in enumerate(nblk):
        bt[i, :k] = perm[p:p + k].to(torch.int32)
        p += k
    slot = lambda i, key: int(bt[i, key // bs]) * bs + key % bs
    kcs = [torch.randn(nb, bs, Hkv, D, generator=g).to(torch.bfloat16).to(DEV) for _ in range(L)]
    vcs = [torch.randn(nb, bs, Hkv, D, generator=g).to(torch.bfloat16).to(DEV) for _ in range(L)]
    one = [torch.ones(1, device=DEV) for _ in range(L)]
    # 1. node K/V of all layers through the ordinary slot mapping: node t of request i at key base_i + t
    k_new = torch.randn(T, L * Hkv * D, generator=g).to(torch.bfloat16)
    v_new = torch.randn(T, L * Hkv * D, generator=g).to(torch.bfloat16)
    slots = torch.tensor([slot(i, bases[i] + t) for i in range(B) for t in range(int(lay.q_lens[i]))], dtype=torch.int64)
    ops.reshape_and_cache_flash_bulk(k_new.to(DEV), v_new.to(DEV), kcs, vcs, slots.to(DEV), "auto", one, one, Hkv, D)
    # ... and tree-attend on layer 0
    q = torch.randn(T, Hq, D, generator=g).to(torch.bfloat16)
    seq = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    got = ops.verify_attention_tree(q.to(DEV), kcs[0], vcs[0], bt.to(DEV), seq, td, max(ctxs), D ** -0.5).float().cpu()
    want = TO.tree_attention(q, kcs[0].cpu(), vcs[0].cpu(), bt, ctxs, lay.query_start_loc, lay.masks, D ** -0.5)
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), float((got - want).abs().max())
    # 2. accept: planted logits follow a random root-to-node walk in every tree
    V = 2000
    logits = torch.randn(T, V, generator=g).to(torch.bfloat16)
    walks = []
    for i in range(B):
        q0, ql = int(lay.query_start_loc[i]), int(lay.q_lens[i])
        cur, walk = 0, [0]
        while True:
            kids = [c for c in range(1, ql) if lay.parents[q0 + c] == cur]
            if not kids or len(walk) == 6:
                logits[q0 + cur, V - 1] = 64.0                            # no node carries V - 1 (draft tokens are below 1000)
                break
            nxt = kids[-1]                                                # the LAST child: the walk skips its elder siblings
            logits[q0 + cur, int(lay.tokens[q0 + nxt])] = 64.0
            cur = nxt
            walk.append(cur)
        walks.append(walk)
    res = ops.rejection_sample_tree(logits.to(DEV), td)
    assert [res.path[i, :len(w)].tolist() for i, w in enumerate(walks)] == walks
    assert res.num_accepted.tolist() == [len(w) for w in walks]
    assert any(w != list(range(len(w))) for w in walks), "every walk is the identity: nothing would move"
    # 3. compact every layer
    before = [_bytes(c) for c in kcs + vcs]
    ops.compact_accepted_paths(kcs, vcs, bt.to(DEV), seq, td, res.path, res.num_accepted)
    torch.cuda.synchronize()
    for b, c in zip(before, kcs + vcs):
        wantc = TO.compact(b.reshape(nb, bs, -1).copy(), bt.numpy(), ctxs, lay.q_lens, res.path.cpu().numpy(),
                           res.num_accepted.cpu().numpy())
        assert np.array_equal(_bytes(c).reshape(nb, bs, -1), wantc)
    # 4. the next step: one new token per request behind the accepted chain, the plain call
    n_acc = [len(w) for w in walks]
    new_ctx = [bases[i] + n_acc[i] + 1 for i in range(B)]
    k1 = torch.randn(B, L * Hkv * D, generator=g).to(torch.bfloat16)
    v1 = torch.randn(B, L * Hkv * D, generator=g).to(torch.bfloat16)
    slots1 = torch.tensor([slot(i, new_ctx[i] - 1) for i in range(B)], dtype=torch.int64)
    ops.reshape_and_cache_flash_bulk(k1.to(DEV), v1.to(DEV), kcs, vcs, slots1.to(DEV), "auto", one, one, Hkv, D)
    q1 = torch.randn(B, Hq, D, generator=g).to(torch.bfloat16)
    qsl1 = np.arange(B + 1, dtype=np.int32)
    # 5. the oracle's cache: built from the accepted chain alone
    kn, vn = k_new.view(T, L, Hkv, D), v_new.view(T, L, Hkv, D)
    for layer in range(L):
        ref_k = torch.zeros(nb, bs, Hkv, D, dtype=torch.bfloat16)
        ref_v = torch.zeros(nb, bs, Hkv, D, dtype=torch.bfloat16)
        dev_k, dev_v = kcs[layer].cpu(), vcs[layer].cpu()
        for i in range(B):
            q0 = int(lay.query_start_loc[i])
            for key in range(bases[i]):                                   # the old context, untouched by the step
                pg, off = int(bt[i, key // bs]), key % bs
                ref_k[pg, off], ref_v[pg, off] = dev_k[pg, off], dev_v[pg, off]
            for d, node in enumerate(walks[i]):                           # the accepted nodes, in path order
                pg, off = int(bt[i, (bases[i] + d) // bs]), (bases[i] + d) % bs
                ref_k[pg, off], ref_v[pg, off] = kn[q0 + node, layer], vn[q0 + node, layer]
            pg, off = int(bt[i, (new_ctx[i] - 1) // bs]), (new_ctx[i] - 1) % bs
            ref_k[pg, off], ref_v[pg, off] = k1.view(B, L, Hkv, D)[i, layer], v1.view(B, L, Hkv, D)[i, layer]
        want1 = O.verify_attention(q1, ref_k, ref_v, bt, new_ctx, qsl1, D ** -0.5)
        got1 = ops.verify_attention(q1.to(DEV), kcs[layer], vcs[layer], bt.to(DEV), torch.tensor(new_ctx, dtype=torch.int32, device=DEV),
                                    torch.from_numpy(qsl1).to(DEV), 1, max(new_ctx), D ** -0.5).float().cpu()
        err = (got1 - want1).abs()
        print("layer", layer, "next-step max abs err", float(err.max()))
        assert torch.allclose(got1, want1, atol=ATOL, rtol=RTOL), (layer, float(err.max()))
