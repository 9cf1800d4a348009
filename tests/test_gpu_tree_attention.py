"""GPU: aic_verify_attention_tree (csrc/verify_attn.hip, the TREE instantiations of the generic body) against the fp32
oracle with an explicit mask (tests/tree_oracle.py) at the project's bar, atol 1e-3 + rtol 2^-8, the output pre-filled
with NaN.  The reference verifies paths only (arctic_inference/vllm/model_runner.py:734-740): there is nothing to compare
trees against but the stated rule, and on chains the plain call.

Every case carries the planted keys of tree_oracle.attention_case: for chosen rows ONE draft key scores 40 nats — an
invisible sibling, descendant or later node, or a visible ancestor / the node itself — so one wrong mask bit moves a row
by order 1 (tests/test_tree_drafts_host.py asserts >= 0.1 on references alone).  Shapes are the smallest that reach a
path: the 33rd mask bit, base = 0 / 15 / 31 (the draft region straddles a page and a 32-token tile), contexts of 40, 200
and ~1100 tokens in pages of 16, G = 1 / 4 / 8 (both heads-per-workgroup forms, one and two row tiles, several row
groups), every cache / dtype combination, q as a column slice, sinks, forced splits with a boundary inside the draft
region, and batches mixing q_len = 1, chains and trees."""
import numpy as np
import pytest
import torch

import tree_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = 1e-3, 2 ** -8


def _ops():
    from arcticinference_amd import ops
    return ops


def _native():
    from arcticinference_amd import _native as N
    return N


class _forced_splits:
    def __init__(self, splits):
        self.splits = splits

    def __enter__(self):
        _native().lib().aic_debug_attn_layout(0, self.splits)

    def __exit__(self, *exc):
        _native().lib().aic_debug_attn_layout(0, 0)
        return False


def _rng(seed):
    return np.random.default_rng(seed)


def _bushy(seed):
    r = _rng(seed)
    return list(range(32)), [-1] * 15 + [int(r.integers(0, 15)) for _ in range(17)]


def _tree_call(c, td, sinks=None, q=None, masks=None):
    ops = _ops()
    kw = {}
    if c.ks is not None:
        kw.update(k_scale=torch.tensor([c.ks], device=DEV), v_scale=torch.tensor([c.vs], device=DEV))
    if sinks is not None:
        kw["sinks"] = sinks.to(DEV)
    qd = c.q.to(DEV) if q is None else q
    out = torch.full((qd.shape[0], c.Hq, c.D), float("nan"), dtype=c.q.dtype, device=DEV)
    ops.verify_attention_tree(qd, c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), torch.tensor(c.ctxs, dtype=torch.int32, device=DEV),
                              td, max(c.ctxs), c.scale, out=out, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _assert_close(got, want, what):
    err = (got - want).abs()
    print(what, "max abs err", float(err.max()), "worst err / bound", float((err / (ATOL + RTOL * want.abs())).max()))
    assert torch.isfinite(got).all(), f"{what}: non-finite output (a row was not written)"
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL), (what, float(err.max()))


# name: trees, contexts (query tokens counted), Hq, Hkv, D, dtype, fp8, extras
_CASES = {
    # q_len = 33: node 32 attends to itself through bit 32 (planted: a 32-bit mask word, or a 32-bit shift, loses it)
    "q33-bit32": dict(trees=lambda: [TO.random_tree(32, _rng(1), 0.6)], ctxs=[200], Hq=8, Hkv=2, last_self=True),
    "deep-and-bushy": dict(trees=lambda: [TO.chain(32), _bushy(2), TO.star(15)], ctxs=[200, 333, 40], Hq=8, Hkv=2),
    "base-0": dict(trees=lambda: [TO.random_tree(19, _rng(3), 0.7), TO.random_tree(32, _rng(4), 0.5)], ctxs=[20, 33], Hq=8, Hkv=2),
    "base-31-and-15": dict(trees=lambda: [TO.random_tree(10, _rng(5), 0.7), TO.random_tree(24, _rng(6), 0.6)],
                           ctxs=[31 + 11, 15 + 25], Hq=8, Hkv=2),
    "ctx-1100": dict(trees=lambda: [TO.random_tree(12, _rng(7), 0.6), TO.random_tree(5, _rng(8), 0.9)], ctxs=[1100, 1093], Hq=8, Hkv=2),
    "G1-hpw4": dict(trees=lambda: [TO.random_tree(20, _rng(9), 0.6), TO.chain(2)], ctxs=[200, 77], Hq=4, Hkv=4),
    "G4-hpw4-two-tiles": dict(trees=lambda: [TO.random_tree(32, _rng(10), 0.6), TO.random_tree(30, _rng(11), 0.4)],
                              ctxs=[200, 131], Hq=16, Hkv=4),
    "G8-ranges": dict(trees=lambda: [TO.random_tree(32, _rng(12), 0.6), TO.random_tree(3, _rng(13), 0.9)], ctxs=[300, 40], Hq=8, Hkv=1),
    "fp8": dict(trees=lambda: [TO.random_tree(32, _rng(14), 0.6), TO.random_tree(6, _rng(15), 0.8)], ctxs=[200, 95], Hq=8, Hkv=2, fp8=True),
    "d64": dict(trees=lambda: [TO.random_tree(32, _rng(16), 0.6), TO.random_tree(6, _rng(17), 0.8)], ctxs=[200, 47], Hq=16, Hkv=2, D=64),
    "f16": dict(trees=lambda: [TO.random_tree(32, _rng(18), 0.6), TO.random_tree(6, _rng(19), 0.8)], ctxs=[200, 40], Hq=8, Hkv=2,
                dtype=torch.float16),
    "f16-fp8": dict(trees=lambda: [TO.random_tree(32, _rng(20), 0.6), TO.random_tree(6, _rng(21), 0.8)], ctxs=[200, 40], Hq=8, Hkv=2,
                    dtype=torch.float16, fp8=True),
    "sinks": dict(trees=lambda: [TO.random_tree(14, _rng(22), 0.6), TO.random_tree(32, _rng(23), 0.8)], ctxs=[40, 200], Hq=8, Hkv=2,
                  sinks=True),
    "sinks-d64": dict(trees=lambda: [TO.random_tree(14, _rng(24), 0.6)], ctxs=[40], Hq=16, Hkv=2, D=64, sinks=True),
    # 7 tiles, 7 splits: boundaries at 160 and 192, the draft region is [167, 200); G8: the four waves split further
    "splits-inside-draft": dict(trees=lambda: [TO.random_tree(32, _rng(25), 0.6), TO.random_tree(9, _rng(26), 0.6)], ctxs=[200, 190],
                                Hq=8, Hkv=2, splits=7),
    "splits-inside-draft-G8": dict(trees=lambda: [TO.random_tree(32, _rng(27), 0.6)], ctxs=[200], Hq=8, Hkv=1, splits=3),
    "splits-fp8": dict(trees=lambda: [TO.random_tree(32, _rng(28), 0.6)], ctxs=[200], Hq=8, Hkv=2, fp8=True, splits=7),
    # mostly decodes: the call takes the one-row-tile form, the 33-token tree nine row groups of it (G1-hpw4 above: two)
    "one-tile-row-groups": dict(trees=lambda: [([], [])] * 3 + [TO.random_tree(32, _rng(34), 0.6)] + [([], [])] * 4,
                                ctxs=[40, 64, 97, 200, 33, 1, 130, 16], Hq=8, Hkv=2, last_self=True),
    "one-tile-fp8": dict(trees=lambda: [TO.random_tree(32, _rng(35), 0.6)] + [([], [])] * 7,
                         ctxs=[200, 40, 64, 97, 33, 1, 130, 16], Hq=8, Hkv=2, fp8=True),
    "one-tile-d64": dict(trees=lambda: [TO.random_tree(32, _rng(36), 0.6)] + [([], [])] * 15,
                         ctxs=[200] + [40 + 3 * i for i in range(15)], Hq=16, Hkv=2, D=64),
    "mixed-batch": dict(trees=lambda: [([], []), TO.chain(3), TO.random_tree(32, _rng(29), 0.6), ([], []), TO.chain(7),
                                       TO.random_tree(4, _rng(30), 1.0)], ctxs=[40, 200, 333, 1, 64, 97], Hq=8, Hkv=2),
}


@pytest.mark.parametrize("name", list(_CASES))
def test_tree_attention_matches_the_oracle(name):
    k = _CASES[name]
    D, dtype = k.get("D", 128), k.get("dtype", torch.bfloat16)
    c = TO.attention_case(k["trees"](), k["ctxs"], k["Hq"], k["Hkv"], D, 16, seed=len(name), dtype=dtype, fp8=k.get("fp8", False),
                          last_self=k.get("last_self", False))
    sinks = (torch.randn(k["Hq"], generator=torch.Generator().manual_seed(3)) * 2).float() if k.get("sinks") else None
    want = TO.case_oracle(c, sinks=sinks)
    td = _ops().TreeDrafts(k["trees"](), DEV)
    assert c.plants, "the case plants nothing"
    if k.get("last_self"):
        assert any(p[1:] == (32, 32, "self") for p in c.plants)
    with _forced_splits(k.get("splits", 0)):
        got = _tree_call(c, td, sinks=sinks)
    _assert_close(got, want, name)


def test_q_as_a_column_slice():
    trees = [TO.random_tree(9, _rng(31), 0.6), TO.chain(2)]
    c = TO.attention_case(trees, [100, 40], 8, 2, 128, 16, seed=7)
    td = _ops().TreeDrafts(trees, DEV)
    wide = torch.randn(c.q.shape[0], 8 * 128 + 2 * 2 * 128, dtype=torch.float32).to(torch.bfloat16).to(DEV)
    wide[:, :8 * 128] = c.q.to(DEV).view(c.q.shape[0], -1)
    qv = wide[:, :8 * 128].view(c.q.shape[0], 8, 128)
    assert qv.stride(0) == 8 * 128 + 4 * 128
    _assert_close(_tree_call(c, td, q=qv), TO.case_oracle(c), "column slice")


def test_chain_masks_are_the_plain_call():
    """With lower-triangular masks the tree call IS the plain call.  Bit-identical against the plain call WITHOUT host
    query lengths: that call takes the generic launch form with the split count pick_splits gives, and so does the tree
    call — same body, same tiles, same order, and a mask test that hides exactly what the causal test hides.  Against the
    plain call WITH host query lengths (the host-partitioned forms: per-request tile choice, other heads-per-workgroup and
    split rules, the long-draft body for the 33-token request) and under a forced split count (which the generic plain call
    does not honour) the summation order differs: there both must meet the bar against the oracle."""
    ops = _ops()
    from oracle import spec_oracle as O
    q_lens = [1, 4, 33, 2, 8]
    trees = [TO.chain(n - 1) for n in q_lens]
    for Hq, Hkv, fp8, ctxs in ((8, 2, False, [40, 200, 333, 64, 1100]), (16, 4, True, [40, 200, 333, 64, 500])):
        c = TO.attention_case(trees, ctxs, Hq, Hkv, 128, 16, seed=9, fp8=fp8, plant=False)
        td = ops.TreeDrafts(trees, DEV)
        got = _tree_call(c, td)
        kw = dict(k_scale=torch.tensor([c.ks], device=DEV), v_scale=torch.tensor([c.vs], device=DEV)) if fp8 else {}
        args = (c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), torch.tensor(c.ctxs, dtype=torch.int32, device=DEV),
                torch.tensor(c.lay.query_start_loc, device=DEV), 33, max(ctxs), c.scale)
        plain = ops.verify_attention(*args, **kw).float().cpu()
        assert torch.equal(got, plain), float((got - plain).abs().max())
        sc = dict(k_scale=c.ks, v_scale=c.vs) if fp8 else {}
        want = O.verify_attention(c.q, c.kc, c.vc, c.bt, c.ctxs, c.lay.query_start_loc, c.scale, **sc)
        hosted = ops.verify_attention(*args, q_lens_host=q_lens, **kw).float().cpu()
        print("tree vs host-partitioned plain call: max abs diff", float((got - hosted).abs().max()))
        _assert_close(hosted, want, "plain call, host lengths")
        _assert_close(got, want, "tree call, chain masks")
        with _forced_splits(5):
            _assert_close(_tree_call(c, td), want, "tree call, chain masks, 5 splits")


def test_a_wrong_bit_is_seen_on_the_device():
    """The fixture discriminates on the device too: the kernel fed a mask with one planted bit flipped lands >= 0.1 from
    the true oracle on the concerned rows (and still on the oracle of the flipped mask)."""
    trees = [TO.random_tree(32, _rng(33), 0.6)]
    c = TO.attention_case(trees, [200], 8, 2, 128, 16, seed=11, last_self=True)
    td = _ops().TreeDrafts(trees, DEV)
    true = TO.case_oracle(c)
    i, t, u, rel = c.plants[0]
    assert (t, u) == (32, 32)
    masks = c.lay.masks.copy()
    masks[t] ^= np.uint64(1 << u)
    td.tree_mask.copy_(torch.from_numpy(masks.view(np.int64)).to(DEV))
    got = _tree_call(c, td)
    _assert_close(got, TO.case_oracle(c, masks=masks), "flipped mask")
    for h in range(2):
        assert float((got[t, h * 4 + t % 4] - true[t, h * 4 + t % 4]).abs().max()) >= 0.1
