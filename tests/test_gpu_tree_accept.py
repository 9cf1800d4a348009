"""GPU: aic_rejection_tree_greedy (csrc/rejection.hip) — greedy acceptance over tree-shaped drafts.  Every comparison is
exact.  On chains every output equals aic_rejection_greedy with bonus_row_index (the chain kernel the project already
pins against vLLM's RejectionSampler semantics, model_runner.py:405-411); on trees the walk is compared with its
restatement (tests/tree_oracle.py), with logits planted so that walks of every length happen."""
import numpy as np
import pytest
import torch

import tree_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from arcticinference_amd import ops
    return ops


def _plant_walks(logits, lay, rng, p_follow=0.7):
    """Raise, at every node, the logit of one child's token (probability p_follow, when the node has children) or of a
    token no child carries: the walks then have every length.  Values are exact in bf16 / f16 / f32."""
    V = logits.shape[1]
    for i in range(len(lay.q_lens)):
        q0, ql = int(lay.query_start_loc[i]), int(lay.q_lens[i])
        for t in range(ql):
            kids = [c for c in range(1, ql) if lay.parents[q0 + c] == t]
            if kids and rng.random() < p_follow:
                tok = int(lay.tokens[q0 + kids[int(rng.integers(len(kids)))]])
            else:
                tok = int(rng.integers(V))
            logits[q0 + t, tok] = 64.0
    return logits


def _check(res, want, W):
    out, nacc, last, hidx, path = want
    assert np.array_equal(res.output_token_ids.cpu().numpy(), out[:, :W])
    assert np.array_equal(res.path.cpu().numpy(), path[:, :W])
    assert np.array_equal(res.num_accepted.cpu().numpy(), nacc)
    assert np.array_equal(res.last_token.cpu().numpy(), last)
    assert np.array_equal(res.hidden_index.cpu().numpy(), hidx)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_chains_equal_the_chain_kernel(dtype):
    ops = _ops()
    rng = np.random.default_rng(1)
    n = [3, 0, 5, 32, 1, 7]
    V = 1000
    td = ops.TreeDrafts([TO.chain(k) for k in n], "cpu")
    lay = td.layout
    logits = torch.randn(int(lay.tokens.size), V, generator=torch.Generator().manual_seed(2)).to(dtype)
    am = torch.argmax(logits.float(), dim=-1).numpy()
    tokens = lay.tokens.copy()
    for i, keep in enumerate([3, 0, 2, 32, 0, 6]):           # drafts accepted per request
        q0 = int(lay.query_start_loc[i])
        for t in range(1, n[i] + 1):
            tokens[q0 + t] = am[q0 + t - 1] if t <= keep else (am[q0 + t - 1] + 1) % V
    trees = [(tokens[lay.query_start_loc[i] + 1:lay.query_start_loc[i + 1]].tolist(), list(range(-1, n[i] - 1))) for i in range(len(n))]
    td = ops.TreeDrafts(trees, DEV)
    res = ops.rejection_sample_tree(logits.to(DEV), td)
    qsl = lay.query_start_loc
    draft_rows = np.concatenate([np.arange(qsl[i], qsl[i] + k) for i, k in enumerate(n)]).astype(np.int64)
    drafts = np.concatenate([tokens[qsl[i] + 1:qsl[i + 1]] for i in range(len(n))]).astype(np.int32)
    chain = ops.rejection_sample(logits.to(DEV), torch.from_numpy(drafts).to(DEV),
                                 torch.tensor(np.cumsum(n), dtype=torch.int32, device=DEV), None, 32,
                                 target_row_index=torch.from_numpy(draft_rows).to(DEV),
                                 bonus_row_index=torch.from_numpy((qsl[1:] - 1).astype(np.int64)).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(res.output_token_ids, chain.output_token_ids)            # [B, 33] both
    assert torch.equal(res.num_accepted, chain.num_accepted) and torch.equal(res.last_token, chain.last_token)
    assert torch.equal(res.hidden_index, chain.hidden_index)
    assert res.num_accepted.tolist() == [4, 1, 3, 33, 1, 7]
    _check(res, TO.tree_accept(logits, tokens, lay.parents, qsl, 33), 33)


@pytest.mark.parametrize("dtype,V,sizes", [(torch.float32, 1000, (32, 32, 15, 0, 7, 1, 20, 32)),
                                           (torch.bfloat16, 1000, (32, 32, 15, 0, 7, 1, 20, 32)),
                                           (torch.float16, 1000, (32, 9, 0, 3)),
                                           (torch.float32, 128256, (6, 0, 3)), (torch.bfloat16, 128256, (6, 0, 3)),
                                           (torch.float16, 128256, (4, 2))],
                         ids=["f32-1000", "bf16-1000", "f16-1000", "f32-128256", "bf16-128256", "f16-128256"])
def test_random_trees_equal_the_restatement(dtype, V, sizes):
    ops = _ops()
    rng = np.random.default_rng(V + len(sizes))
    trees = []
    for k, n in enumerate(sizes):
        ids, par = TO.random_tree(n, rng, 0.3 + 0.1 * (k % 6))
        trees.append(([int(x) for x in rng.permutation(V)[:n]], par))
    td = ops.TreeDrafts(trees, DEV, root_tokens=[1] * len(sizes))
    lay = td.layout
    logits = torch.randn(int(lay.tokens.size), V, generator=torch.Generator().manual_seed(3)).to(dtype)
    logits = _plant_walks(logits, lay, rng)
    want = TO.tree_accept(logits, lay.tokens, lay.parents, lay.query_start_loc, td.max_q_len)
    assert len(set(want[1].tolist())) > 1 or len(sizes) < 4           # walks of several lengths
    res = ops.rejection_sample_tree(logits.to(DEV), td)
    torch.cuda.synchronize()
    _check(res, want, td.max_q_len)


def test_specific_walks_and_the_lowest_index_tie():
    ops = _ops()
    V = 4099                                                 # rows that are not 16-byte multiples: the scalar loads
    # request 0: rejection at the root.  request 1: root -> {10, 11, 12}, 12 -> {13}: the THIRD sibling matches, then its
    # child.  request 2: a full-depth path through a tree with decoys.  request 3: a tie at the root between tokens 7 and
    # 3000 (equal stored values, in different vocabulary segments of the row phase): the lowest index, 7, is emitted and
    # its child followed.
    trees = [([5, 6], [-1, 0]),
             ([10, 11, 12, 13], [-1, -1, -1, 2]),
             ([20, 21, 22, 23, 24, 25], [-1, -1, 1, 1, 3, 2]),
             ([3000, 7, 8], [-1, -1, 1])]
    td = ops.TreeDrafts(trees, DEV)
    lay = td.layout
    logits = torch.randn(int(lay.tokens.size), V, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    q = lay.query_start_loc

    def say(req, node, tok, val=64.0):
        logits[q[req] + node, tok] = val
    say(0, 0, 99)
    say(1, 0, 12), say(1, 3, 13), say(1, 4, 4000)
    say(2, 0, 21), say(2, 2, 23), say(2, 4, 24), say(2, 5, 3)
    say(3, 0, 7, 32.0), say(3, 0, 3000, 32.0), say(3, 2, 8), say(3, 3, 1)
    res = ops.rejection_sample_tree(logits.to(DEV), td)
    torch.cuda.synchronize()
    W = td.max_q_len
    assert W == 7
    assert res.output_token_ids.tolist() == [[99, -1, -1, -1, -1, -1, -1], [12, 13, 4000, -1, -1, -1, -1],
                                             [21, 23, 24, 3, -1, -1, -1], [7, 8, 1, -1, -1, -1, -1]]
    assert res.path.tolist() == [[0, -1, -1, -1, -1, -1, -1], [0, 3, 4, -1, -1, -1, -1], [0, 2, 4, 5, -1, -1, -1],
                                 [0, 2, 3, -1, -1, -1, -1]]
    assert res.num_accepted.tolist() == [1, 3, 4, 3] and res.last_token.tolist() == [99, 4000, 3, 1]
    assert res.hidden_index.tolist() == [int(q[0]), int(q[1]) + 4, int(q[2]) + 5, int(q[3]) + 3]
    _check(res, TO.tree_accept(logits, lay.tokens, lay.parents, q, W), W)


def test_gathered_and_row_index_forms_agree():
    ops = _ops()
    rng = np.random.default_rng(5)
    trees = [TO.random_tree(n, rng, 0.5) for n in (9, 0, 32, 4)]
    td = ops.TreeDrafts(trees, DEV)
    lay = td.layout
    T, V = int(lay.tokens.size), 1000
    logits = _plant_walks(torch.randn(T, V, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16), lay, rng)
    full = torch.randn(T + 11, V + 24, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16)   # a wider, longer buffer
    rows = rng.permutation(T + 11)[:T].astype(np.int64)
    full[torch.from_numpy(rows), :V] = logits
    a = ops.rejection_sample_tree(logits.to(DEV), td)
    b = ops.rejection_sample_tree(full.to(DEV)[:, :V], td, row_index=torch.from_numpy(rows).to(DEV))
    torch.cuda.synchronize()
    for f in ("output_token_ids", "path", "num_accepted", "last_token", "hidden_index"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    _check(a, TO.tree_accept(logits, lay.tokens, lay.parents, lay.query_start_loc, td.max_q_len), td.max_q_len)
