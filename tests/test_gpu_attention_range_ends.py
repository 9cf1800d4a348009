"""GPU: the END of a wave's token range in the short verify body (csrc/verify_attn.hip, verify_attn_body).  The body
requests nothing past its range: the last tile of a range issues no K / V loads and the one before it no page lookup.
What can go wrong there: a last tile that is dropped or half consumed, a tile of the neighbouring range consumed twice,
a one-tile range that reads the page entry of a tile it does not have, and anything behind the context reaching the result.

Smallest shapes at which that shows (Hq 32 / Hkv 8 / D 128, pages of 16, four requests, one layer): contexts of one to
six 32-token tiles, ending on and beside tile and page borders, under forced layouts (heads per workgroup, splits) of
1, 2, 4, 8 and 12 ranges per head, so that ranges of zero, one, two and more tiles all occur; query lengths 1 and 4 take
the one-row-tile body, 8 the two-row-tile one, a 10-token draft the pair kernel (its short part beside a long workgroup).
Every call goes through the host-partitioned path with the identity list of short requests.  Reference: the fp32
oracle at the bar of the planted-key tests (imported from there)."""
import pytest
import torch

import attention_fixtures as F
import test_gpu_attention_planted as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
HQ, HKV, D, BS = 32, 8, 128, 16
LAYOUTS = [(4, 1), (4, 2), (4, 4), (2, 2), (1, 1), (1, 3)]      # (kv heads per workgroup, cross-workgroup splits)
CTX_POOL = (1, 17, 32, 33, 64, 95, 96, 97, 129, 161)
# three batches of four cover the pool; a request's context holds its own query tokens, so context 1 exists for q_len 1 only
BATCHES = ([1, 17, 32, 33], [64, 95, 96, 97], [129, 161, 33, 97])
KTILE = 32


@pytest.fixture(autouse=True)
def _reset_layout(request):
    from arcticinference_amd import _native as N
    request.addfinalizer(lambda: N.lib().aic_debug_attn_layout(0, 0))


def _force(hpw, splits):
    from arcticinference_amd import _native as N
    N.lib().aic_debug_attn_layout(hpw, splits)


def _run(c):
    """One verify call with the host's query lengths (identity short list when no request is long); NaN-prefilled output."""
    from arcticinference_amd import ops
    args, kw = P._dev(c)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    ops.verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out, q_lens_host=c.q_lens, **kw)
    return out


def _check(c, got, want, what):
    got = got.float().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert torch.allclose(got, want, atol=P.ATOL, rtol=P.RTOL), f"{what}:\n" + F.describe(c, got, want, P.ATOL, P.RTOL)


def _all_layouts(c, what):
    want = F.oracle(c)          # once per case, shared by the layouts
    for hpw, splits in LAYOUTS:
        _force(hpw, splits)
        _check(c, _run(c), want, (what, "hpw", hpw, "splits", splits))


def _batches(q_len):
    return [[x if x >= q_len else CTX_POOL[(i + 3) % len(CTX_POOL)] for i, x in enumerate(b)] for b in BATCHES]


def test_the_batches_cover_the_pool():
    assert {x for b in BATCHES for x in b} == set(CTX_POOL)
    for q_len in (4, 8):
        assert {x for b in _batches(q_len) for x in b} == set(CTX_POOL) - {1}


# ---- oracle parity at range edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_len", [1, 4, 8])
def test_range_edges_every_layout(q_len):
    assert q_len * (HQ // HKV) <= 32          # every request short: the identity list
    for i, ctxs in enumerate(_batches(q_len)):
        c = F.planted_case([q_len] * 4, ctxs, HQ, HKV, D, BS, seed=40 + 3 * q_len + i)
        _all_layouts(c, (q_len, ctxs))


def _f16(c):
    c.q, c.kc, c.vc = c.q.to(torch.float16), c.kc.to(torch.float16), c.vc.to(torch.float16)
    return c


@pytest.mark.parametrize("kind", ["fp8", "D64", "f16", "window48"])
def test_range_edges_other_instantiations(kind):
    if kind == "fp8":
        c = F.planted_case([4, 1, 4, 8], [97, 33, 161, 64], HQ, HKV, D, BS, seed=51, fp8=True)
    elif kind == "D64":
        c = F.planted_case([4, 1, 4, 8], [97, 33, 161, 64], HQ, HKV, 64, BS, seed=52)
    elif kind == "f16":
        c = _f16(F.planted_case([4, 1, 4, 8], [97, 33, 161, 64], HQ, HKV, D, BS, seed=53))
    else:
        c = F.planted_case([4, 1, 4, 8], [130, 130, 97, 64], HQ, HKV, D, BS, seed=54, window=48)
    _all_layouts(c, kind)


def test_range_edges_short_part_of_a_mixed_call():
    """A 10-token draft (40 rows: the long-draft body) at context 97 beside three short requests: the pair kernel."""
    c = F.planted_case([10, 1, 4, 8], [97, 33, 161, 64], HQ, HKV, D, BS, seed=55)
    assert 10 * (HQ // HKV) > 32
    _all_layouts(c, "mixed")


# ---- planted keys at the seams ----------------------------------------------------------------------------------------
def _seams(ctx, hpw, splits):
    """First tokens of the ranges 1 .. n - 1 of a request (equal splits: the short-only call), as verify_attn_body cuts them."""
    n_parts = splits * (4 // hpw)
    tiles = (ctx + KTILE - 1) // KTILE
    per = (tiles + n_parts - 1) // n_parts
    return [p * per * KTILE for p in range(1, n_parts) if p * per * KTILE < ctx]


def _seam_case(q_len, ctxs, seams, seed):
    """planted_case's phase code with TWO equal aims per row: the last key of a range and the first key of the next one
    (seam b: keys b - 1 and b; both score A (1 + mean cos theta), so the row's output is (V[b - 1] + V[b]) / 2).  A last
    tile that is dropped gives V[b]; the neighbour's first tile consumed by both ranges gives (V[b - 1] + 2 V[b]) / 3."""
    c = F.planted_case([q_len] * len(ctxs), ctxs, HQ, HKV, D, BS, seed)
    g = torch.Generator().manual_seed(seed)       # planted_case's first draw: the frequencies of every kv head
    M, G = D // 2, HQ // HKV
    theta = (torch.rand(HKV, M, generator=g, dtype=torch.float64) * (1 - 2e-6) + 1e-6) * torch.pi
    head_theta = theta[torch.arange(HQ) // G]
    # the fixture's keys are this code (bf16-rounded): key j of kv head h is phase(j, theta[h])
    blk = c.bt[-1, 0].long()
    assert torch.allclose(c.kc[blk, 1].float(), F._phase(torch.tensor([[1]]), theta).float().view(HKV, D), atol=2 ** -8)
    q = torch.zeros(c.q.shape, dtype=torch.float64)
    seam_of = torch.full(c.kind.shape, -1, dtype=torch.int64)
    for i, ctx in enumerate(ctxs):
        ok = [b for b in seams[i] if b <= ctx - q_len]            # both keys visible to every token of the request
        for n in range(q_len):
            row = int(c.qsl[i]) + n
            if not ok:
                q[row] = c.q[row].double()
                continue
            b = torch.tensor([ok[(n * G + h % G + h // G) % len(ok)] for h in range(HQ)])
            seam_of[row] = b
            q[row] = (F.AMP / (M * c.scale)) * (F._phase(b - 1, head_theta) + F._phase(b, head_theta))
    c.q = q.float().to(torch.bfloat16)
    return c, seam_of


def _expected_pairs(c, seam_of):
    """(V[b - 1] + V[b]) / 2 for every row that aims at a seam, from the cache: rows [n, D], their (token, head) index,
    and the smallest max |V[b] - V[b - 1]| among them."""
    G = HQ // HKV
    idx, rows, gap = [], [], float("inf")
    for i, ctx in enumerate(c.ctxs):
        for n in range(c.q_lens[i]):
            tok = int(c.qsl[i]) + n
            for h in range(HQ):
                b = int(seam_of[tok, h])
                if b < 0:
                    continue
                v = [c.vc[c.bt[i, t // BS].long(), t % BS, h // G].float() for t in (b - 1, b)]
                idx.append((tok, h))
                rows.append(0.5 * (v[0] + v[1]))
                gap = min(gap, float((v[0] - v[1]).abs().max()))
    return idx, torch.stack(rows), gap


@pytest.mark.parametrize("q_len", [1, 4, 8])
def test_planted_keys_at_every_seam(q_len):
    # 13, 25, 6 and 4 tiles: under 12 ranges the first request has ranges of two tiles and one of one, the second of
    # three and one of one, the others ranges of one tile and empty ones
    ctxs = [385 + q_len, 770 + q_len, 161 + q_len, 97 + q_len]
    covered, built = set(), {}
    for hpw, splits in LAYOUTS:
        seams = [_seams(ctx, hpw, splits) for ctx in ctxs]
        if not any(seams):
            continue            # (4, 1): one range per head, no seam
        key = repr(seams)       # layouts with the same number of ranges per head share their fixture and reference
        if key not in built:
            c, seam_of = _seam_case(q_len, ctxs, seams, seed=60 + q_len)
            want = F.oracle(c)
            idx, pair, gap = _expected_pairs(c, seam_of)
            t, h = torch.tensor(idx).t()
            # the fixture does what it says: the oracle's rows are the mean of the two planted values.  (0.1: the two
            # weights differ from 1/2 by the bf16 rounding of q and k, ~0.03 on the largest element; V is randn, so a
            # dropped or doubled key moves a row by at least max |V[b] - V[b - 1]| / 6, asserted > 0.2)
            assert (want[t, h] - pair).abs().max() < 0.1, float((want[t, h] - pair).abs().max())
            assert gap / 6 > 0.2, gap
            built[key] = (c, seam_of, want, t, h, pair)
        c, seam_of, want, t, h, pair = built[key]
        for i in range(len(ctxs)):
            for b in seams[i]:
                if b <= ctxs[i] - q_len:
                    assert (seam_of[int(c.qsl[i]):int(c.qsl[i + 1])] == b).any(), (hpw, splits, i, b)
                    covered.add((hpw, splits, i, b))
        _force(hpw, splits)
        got = _run(c)
        _check(c, got, want, ("seams", q_len, hpw, splits))
        # each planted key exactly once: dropping one or doubling one moves the row by |V[b] - V[b - 1]| / 2 or / 6
        assert (got.float().cpu()[t, h] - pair).abs().max() < 0.1
    assert len({(hpw, splits) for hpw, splits, _, _ in covered}) == len(LAYOUTS) - 1


# ---- nothing read past the range is used ------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_nothing_behind_the_context_reaches_the_result(fp8):
    """Block-table columns behind a request's last page name a valid page full of NaN, and the slots of the last page
    behind the context hold NaN: finite output, bit-identical to the same call with zeros there."""
    q_lens, ctxs = [4, 1, 8, 4], [97, 33, 129, 161]
    outs = {}
    for fill in ("nan", "zero"):
        c = F.planted_case(q_lens, ctxs, HQ, HKV, D, BS, seed=70, fp8=fp8)
        spare = int(c.bt[0, -1])                   # the page every padded column names (a page of the cache: valid memory)
        assert all(int(c.bt[i, (ctx + BS - 1) // BS]) == spare for i, ctx in enumerate(ctxs))
        for cache in (c.kc, c.vc):
            if fp8:        # e4m3 codes: 0x7f is NaN
                cache, bad = cache.view(torch.uint8), 0x7f if fill == "nan" else 0
            else:
                bad = float("nan") if fill == "nan" else 0.0
            cache[spare] = bad
            for i, ctx in enumerate(ctxs):
                if ctx % BS:
                    cache[int(c.bt[i, ctx // BS]), ctx % BS:] = bad
        if fill == "nan":
            assert torch.isnan(c.kc[spare].float()).all() and torch.isnan(c.vc[spare].float()).all()
        want = F.oracle(c) if fill == "zero" else None
        for hpw, splits in LAYOUTS:
            _force(hpw, splits)
            got = _run(c)
            assert torch.isfinite(got.float()).all(), (fill, hpw, splits)
            if want is not None:
                _check(c, got, want, ("zeros behind the context", hpw, splits))
            outs[fill, hpw, splits] = got.cpu()
    for hpw, splits in LAYOUTS:
        assert torch.equal(outs["nan", hpw, splits].view(torch.int16), outs["zero", hpw, splits].view(torch.int16)), (hpw, splits)


# ---- run-to-run bit identity ------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits():
    c = F.planted_case([4, 1, 8, 4], [97, 33, 129, 161], HQ, HKV, D, BS, seed=80)
    for hpw, splits in LAYOUTS:
        _force(hpw, splits)
        a, b = _run(c), _run(c)
        assert torch.equal(a, b), (hpw, splits)
