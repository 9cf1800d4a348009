"""Host: the layout of tree-shaped drafts (arcticinference_amd/tree_drafts.py), the test-side oracles of the tree verify
kernels (tests/tree_oracle.py) against the chain oracles, the discriminating fixture on references alone, and what the
three C entry points answer before they look for a device.

The reference verifies paths only (arctic_inference/vllm/model_runner.py:734-740); on chains the tree forms must be the
chain forms, and that is what is pinned here: oracle.spec_oracle.verify_attention to 1e-6 under lower-triangular masks,
oracle.spec_oracle.rejection_greedy exactly."""
import numpy as np
import pytest
import torch

import tree_oracle as TO
from arcticinference_amd import tree_drafts as TD
from oracle import spec_oracle as O


def _masks_of(tree):
    return TD.ancestor_masks(TD.rooted_parents(tree[1]))[0]


# ---- the mask builder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 32])
def test_chains_give_the_lower_triangular_masks(n):
    lay = TD.build_tree_layout([TO.chain(n)])
    want = np.array([(2 << t) - 1 for t in range(n + 1)], dtype=np.uint64)
    assert np.array_equal(lay.masks, want) and np.array_equal(lay.masks, TD.chain_masks(n + 1))
    assert np.array_equal(lay.depths, np.arange(n + 1)) and np.array_equal(lay.parents, np.arange(-1, n))
    assert lay.masks.dtype == np.uint64 and lay.q_lens.tolist() == [n + 1] and lay.query_start_loc.tolist() == [0, n + 1]


def test_random_trees_equal_a_naive_ancestor_walk():
    rng = np.random.default_rng(0)
    deep = TO.chain(32)                                                 # depth 32
    bushy = (list(range(32)), [-1] * 15 + [int(rng.integers(0, 15)) for _ in range(17)])   # a root with 15 children
    trees = [deep, bushy, TO.star(15), ([], [])] + [TO.random_tree(int(n), rng, b) for n, b in
                                                     ((32, 0.5), (32, 0.9), (7, 0.3), (1, 0.5), (20, 1.0))]
    lay = TD.build_tree_layout(trees, root_tokens=list(range(len(trees))))
    assert lay.q_lens.tolist() == [33, 33, 16, 1, 33, 33, 8, 2, 21]
    for i, tr in enumerate(trees):
        q0, q1 = lay.query_start_loc[i], lay.query_start_loc[i + 1]
        rooted = lay.parents[q0:q1]
        assert rooted[0] == -1 and np.array_equal(rooted[1:], np.asarray(tr[1], dtype=np.int64) + 1)
        assert np.array_equal(lay.masks[q0:q1], TO.naive_masks(rooted)), i
        assert np.array_equal(lay.tokens[q0:q1], [i] + list(tr[0]))
        depth = [0] * (q1 - q0)
        for t in range(1, q1 - q0):
            depth[t] = depth[rooted[t]] + 1
        assert lay.depths[q0:q1].tolist() == depth
        m = lay.masks[q0:q1]
        assert all(int(m[t]) >> t == 1 for t in range(q1 - q0))        # bit t set, none above: the kernel's precondition
    assert int(lay.masks[32]) >> 32 == 1                               # node 32 of the deep tree needs the 33rd bit
    pos = TD.positions(lay, lay.q_lens + 100)
    assert np.array_equal(pos, 100 + lay.depths)


def test_bad_input_raises_and_long_results_are_cut():
    with pytest.raises(ValueError, match="parent before child"):
        TD.build_tree_layout([([5, 6], [-1, 1])])
    with pytest.raises(ValueError, match="parent before child"):
        TD.build_tree_layout([([5, 6, 7], [-1, 2, 0])])
    with pytest.raises(ValueError, match="parent before child"):
        TD.build_tree_layout([([5], [-2])])
    with pytest.raises(ValueError, match="token ids"):
        TD.build_tree_layout([([5, 6], [-1])])
    with pytest.raises(ValueError, match="same token"):
        TD.build_tree_layout([([5, 5], [-1, -1])])
    TD.build_tree_layout([([5, 5], [-1, 0])])                           # the same token under different parents is fine
    long = TO.random_tree(40, np.random.default_rng(1))
    lay = TD.build_tree_layout([long])
    assert lay.q_lens.tolist() == [33] and np.array_equal(lay.tokens[1:], long[0][:32])
    assert np.array_equal(lay.masks, TO.naive_masks(lay.parents))
    with pytest.raises(ValueError, match="at most 32"):
        TD.build_tree_layout([long], strict=True)
    with pytest.raises(ValueError):
        TD.chain_masks(65)
    with pytest.raises(ValueError):
        TD.positions(lay, [10])


def test_tree_drafts_uploads_one_buffer():
    from arcticinference_amd import ops
    trees = [TO.chain(3), TO.star(4), ([], [])]
    td = ops.TreeDrafts(trees, "cpu", root_tokens=[7, 8, 9])
    assert (td.batch, td.num_tokens, td.max_q_len) == (3, 10, 5)
    assert td.tree_mask.dtype == torch.int64 and np.array_equal(td.tree_mask.numpy().view(np.uint64), td.layout.masks)
    assert td.draft_token_ids.tolist() == [7, 100, 101, 102, 8, 200, 201, 202, 203, 9]
    assert td.parents.tolist() == [-1, 0, 1, 2, -1, 0, 0, 0, 0, -1] and td.query_start_loc.tolist() == [0, 4, 9, 10]


# ---- the oracles on chains ---------------------------------------------------------------------------------------------
def test_tree_attention_oracle_equals_the_chain_oracle_on_chains():
    c = TO.attention_case([TO.chain(3), TO.chain(0), TO.chain(32)], [70, 33, 200], 8, 2, 128, 16, seed=2, plant=False)
    sinks = torch.randn(8, generator=torch.Generator().manual_seed(1))
    for sk in (None, sinks):
        want = O.verify_attention(c.q, c.kc, c.vc, c.bt, c.ctxs, c.lay.query_start_loc, c.scale, sinks=sk)
        got = TO.case_oracle(c, sinks=sk)
        assert float((got - want).abs().max()) <= 1e-6
    c8 = TO.attention_case([TO.chain(5)], [90], 4, 1, 128, 16, seed=3, fp8=True, plant=False)
    want = O.verify_attention(c8.q, c8.kc, c8.vc, c8.bt, c8.ctxs, c8.lay.query_start_loc, c8.scale, k_scale=c8.ks, v_scale=c8.vs)
    assert float((TO.case_oracle(c8) - want).abs().max()) <= 1e-6


def test_tree_acceptance_oracle_equals_the_chain_oracle_on_chains():
    g = torch.Generator().manual_seed(4)
    n = [3, 0, 5, 2]
    V = 50
    lay = TD.build_tree_layout([TO.chain(k) for k in n])
    logits = torch.randn(int(lay.tokens.size), V, generator=g)
    am = torch.argmax(logits, dim=-1).numpy()
    tokens = lay.tokens.copy()
    # request 0 accepts everything, request 2 its first two drafts, request 3 nothing
    for i, keep in ((0, 3), (2, 2), (3, 0)):
        q0 = lay.query_start_loc[i]
        for t in range(1, n[i] + 1):
            tokens[q0 + t] = am[q0 + t - 1] if t <= keep else (am[q0 + t - 1] + 1) % V
    out, nacc, last, hidx, path = TO.tree_accept(logits, tokens, lay.parents, lay.query_start_loc, 6)
    # the chain form: draft rows are the rows of tokens 0 .. n - 1 of a request, the bonus row that of token n
    draft_rows = np.concatenate([np.arange(lay.query_start_loc[i], lay.query_start_loc[i] + k) for i, k in enumerate(n)])
    bonus_rows = lay.query_start_loc[1:] - 1
    drafts = np.concatenate([tokens[lay.query_start_loc[i] + 1:lay.query_start_loc[i + 1]] for i in range(len(n))])
    want = O.rejection_greedy(logits[draft_rows], drafts, n, am[bonus_rows], 5)
    assert np.array_equal(out, want)
    assert nacc.tolist() == [4, 1, 3, 1] and np.array_equal(hidx, O.hidden_state_index(want, n))
    assert path[0].tolist() == [0, 1, 2, 3, -1, -1] and path[2].tolist() == [0, 1, 2, -1, -1, -1]
    assert last.tolist() == [int(want[i, nacc[i] - 1]) for i in range(4)]


def test_tree_acceptance_oracle_takes_the_matching_sibling():
    # root -> {a: 1, b: 2, c: 3}; c -> {d: 4}; the target says 3 at the root, 4 at c, 9 at d
    tokens, parents = np.array([-1, 1, 2, 3, 4]), np.array([-1, 0, 0, 0, 3])
    logits = torch.zeros(5, 10)
    logits[0, 3], logits[3, 4], logits[4, 9] = 1, 1, 1
    out, nacc, last, hidx, path = TO.tree_accept(logits, tokens, parents, [0, 5], 5)
    assert out[0].tolist() == [3, 4, 9, -1, -1] and path[0].tolist() == [0, 3, 4, -1, -1]
    assert (int(nacc[0]), int(last[0]), int(hidx[0])) == (3, 9, 4)


def test_compaction_restatement_reads_before_it_writes():
    cache = np.arange(4 * 4, dtype=np.int32).reshape(4, 4, 1).copy()     # pages [1, 3]: keys 0 .. 7 -> values 4 .. 7, 12 .. 15
    bt = np.array([[1, 3]])
    got = TO.compact(cache.copy(), bt, [8], [5], np.array([[0, 2, 3, -1, -1]]), [3])   # base 3: slots 5 -> 4, 6 -> 5
    want = cache.copy()
    want[3, 0], want[3, 1] = cache[3, 1], cache[3, 2]
    assert np.array_equal(got, want)


# ---- the discriminating fixture, on references alone -------------------------------------------------------------------
def _flip_cases():
    rng = np.random.default_rng(5)
    bushy = (list(range(32)), [-1] * 15 + [int(rng.integers(0, 15)) for _ in range(17)])
    return [
        ("q33", [TO.random_tree(32, rng, 0.6)], [200], 8, 2, 128, False, True),
        ("bushy-fp8", [bushy, TO.random_tree(9, rng, 0.7)], [64, 40], 4, 4, 128, True, False),
        ("d64", [TO.random_tree(12, rng, 0.8), TO.chain(4)], [28, 100], 8, 1, 64, False, False),
    ]


@pytest.mark.parametrize("name,trees,ctxs,Hq,Hkv,D,fp8,last_self", _flip_cases(), ids=[c[0] for c in _flip_cases()])
def test_one_flipped_mask_bit_moves_every_concerned_row(name, trees, ctxs, Hq, Hkv, D, fp8, last_self):
    """The bar tests/test_attention_fixtures_host.py uses for moved edges: a reference in which the ONE bit of a plant is
    flipped lies at least 0.1 from the true reference on every row the plant concerns."""
    c = TO.attention_case(trees, ctxs, Hq, Hkv, D, 16, seed=6, fp8=fp8, last_self=last_self)
    true = TO.case_oracle(c, dtype=torch.float64)
    rels = {p[3] for p in c.plants}
    assert {"sibling", "descendant", "later", "ancestor"} <= rels or name != "q33", rels
    assert c.rows and (not last_self or (0, 32, 32, "self") in c.plants)
    for i, t, u, rel in c.plants:
        q0 = int(c.lay.query_start_loc[i])
        masks = c.lay.masks.copy()
        assert bool((int(masks[q0 + t]) >> u) & 1) == (rel in ("ancestor", "self"))
        masks[q0 + t] ^= np.uint64(1 << u)
        flipped = TO.case_oracle(c, masks=masks, dtype=torch.float64)
        G = Hq // Hkv
        for h in range(Hkv):
            hq = h * G + t % G
            d = float((flipped[q0 + t, hq] - true[q0 + t, hq]).abs().max())
            assert d >= 0.1, (name, i, t, u, rel, hq, d)
        other = torch.ones(true.shape[0], dtype=torch.bool)
        other[q0 + t] = False
        assert torch.equal(flipped[other], true[other])                  # and no other token's row moves


# ---- the entry points before they look for a device --------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    import os
    from arcticinference_amd import _native as N
    text = open(os.path.join(os.path.dirname(N._PKG), "include", "arctic_hip.h")).read()
    for name in ("aic_verify_attention_tree", "aic_rejection_tree_greedy", "aic_kv_compact_paths"):
        assert f"int {name}(" in text and name in N.EXPORTED_SYMBOLS and hasattr(N.lib(), name), name
    dt, tr = N._SIGNATURES["aic_verify_attention_dt"][1], N._SIGNATURES["aic_verify_attention_tree"][1]
    assert tr[:25] == dt[:25]                                            # dt's arguments up to max_seq_len, no request lists
    doc = text[text.index("Verify attention for TREE-shaped drafts"):text.index("int aic_verify_attention_tree(")]
    assert "model_runner.py:734-740" in doc
    acc = text[text.index("Greedy acceptance over TREE-shaped drafts"):text.index("int aic_rejection_tree_greedy(")]
    assert "multi-draft rejection sampling" in acc                       # random acceptance over trees: said to be out of scope


def test_tree_entry_points_answer_before_any_launch():
    from arcticinference_amd import _native as N
    L = N.lib()

    def attn(window=0, prefix=0, head=128, kv=N.DT_BF16, qd=N.DT_BF16, max_q=5, mask=1, bs=16):
        return L.aic_verify_attention_tree(1, 512, 1, 1, 16 * 128, kv, 1, 1, 1, 8, 1, 1, 2, 6, max_q, 4, 1, head, bs, 0.088,
                                           1, 512, 1, 1 << 20, 200, window, prefix, None, qd, mask, None)
    assert attn(window=128) == N.AIC_ERR_UNSUPPORTED
    assert attn(prefix=64) == N.AIC_ERR_UNSUPPORTED
    assert attn(head=96) == N.AIC_ERR_UNSUPPORTED
    assert attn(head=64, kv=N.DT_FP8_E4M3) == N.AIC_ERR_UNSUPPORTED     # as the plain call: head size 64 needs a 16-bit cache
    assert attn(qd=N.DT_F32) == N.AIC_ERR_UNSUPPORTED and attn(kv=N.DT_F16) == N.AIC_ERR_UNSUPPORTED
    assert attn(bs=8) == N.AIC_ERR_UNSUPPORTED
    assert attn(max_q=65) == N.AIC_ERR_INVALID and attn(mask=None) == N.AIC_ERR_INVALID

    def accept(dt=N.DT_F32, max_q=5, parent=1):
        return L.aic_rejection_tree_greedy(1, dt, 64, 64, 1, parent, 1, 2, 6, max_q, 1, None, None, None, None, None, 1, None)
    assert accept(dt=N.DT_FP8_E4M3) == N.AIC_ERR_UNSUPPORTED
    assert accept(max_q=65) == N.AIC_ERR_INVALID and accept(parent=None) == N.AIC_ERR_INVALID

    import ctypes
    tab = (ctypes.c_void_p * 2)(256, 512)

    def compact(heads=8, max_q=5, es=2):
        return L.aic_kv_compact_paths(tab, tab, 2, 1, 8, 1, 1, 1, 1, 2, max_q, heads, 128, es, 16, 16 * heads * 128, None)
    assert compact(es=3) == N.AIC_ERR_INVALID and compact(max_q=65) == N.AIC_ERR_INVALID
    assert L.aic_kv_compact_paths(tab, tab, 2, 1, 8, 1, 1, 1, 1, 2, 5, 1, 24, 1, 16, 16 * 24, None) == N.AIC_ERR_UNSUPPORTED
    if not torch.cuda.is_available():                     # (with a device these would launch on the dummy pointers)
        assert attn() == N.AIC_ERR_NO_DEVICE and attn(head=64) == N.AIC_ERR_NO_DEVICE
        assert attn(kv=N.DT_FP8_E4M3) == N.AIC_ERR_NO_DEVICE and attn(qd=N.DT_F16, kv=N.DT_F16) == N.AIC_ERR_NO_DEVICE
        assert accept() == N.AIC_ERR_NO_DEVICE and accept(dt=N.DT_BF16) == N.AIC_ERR_NO_DEVICE
        assert compact() == N.AIC_ERR_NO_DEVICE and compact(es=1) == N.AIC_ERR_NO_DEVICE


def test_ops_refuse_windows_and_prefixes_with_the_native_status():
    from arcticinference_amd import _native as N
    from arcticinference_amd import ops
    td = ops.TreeDrafts([TO.chain(2)], "cpu")
    q = torch.zeros(3, 4, 128, dtype=torch.bfloat16)
    kc = torch.zeros(2, 16, 1, 128, dtype=torch.bfloat16)
    bt = torch.zeros(1, 2, dtype=torch.int32)
    sl = torch.tensor([20], dtype=torch.int32)
    for kw in (dict(sliding_window=128), dict(shared_prefix_len=64)):
        with pytest.raises(N.NativeError) as e:
            ops.verify_attention_tree(q, kc, kc, bt, sl, td, 20, 0.088, **kw)
        assert e.value.code == N.AIC_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.verify_attention_tree(q, kc, kc, bt, sl, td, 20, 0.088)
    with pytest.raises(ValueError, match="TreeDrafts describes"):
        ops.verify_attention_tree(q[:2], kc, kc, bt, sl, td, 20, 0.088)
