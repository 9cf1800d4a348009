"""CPU: the proof that tests/test_gpu_high_pages.py would fail on a kernel whose page product is narrowed — on offsets
alone, no big allocation.  For every case that module relocates (tests/high_page_arena.py has the one table), in both
layouts: the map's rules (a) - (d), injectivity, disjoint K / V / layer pages, no poisoned region on a used page; then the
address computation restated in numpy, exactly and with one step narrowed (the byte product in int32, in uint32, the
element product in int32, the in-page offset added to a 64-bit base in the low word only): every address a mutant
forms lies inside the allocation, every request has a read that differs from the exact address, and every differing
address lies in a poisoned region.  The same bargain as tests/test_attention_fixtures_host.py and
tests/test_fp8_codes_host.py: the sensitivity is proven here, the GPU test uses it."""
import numpy as np
import pytest
import torch

import high_page_arena as A

_MAPS = list(A.all_maps())
_IDS = [f"{name}-{layout}-flip{flip}" for name, layout, flip, _, _ in _MAPS]


def test_the_arena_is_what_the_bands_assume():
    assert A.GUARD == 2 ** 32 and A.SPAN == 2 ** 32 + 2 ** 26 and A.TOTAL == A.GUARD + A.SPAN
    # every alias of band H (O - 2^32 < 2^26, plus the phase of a view: below 2^27) lies below L
    assert A.SPAN - 2 ** 32 + 66 * 65536 < A.L_FLOOR
    assert A.NAN_PATTERN[torch.bfloat16] == 0x7FC0 and A.NAN_PATTERN[torch.float16] == 0x7E00
    for dtype, pat in A.NAN_PATTERN.items():
        raw = torch.tensor([pat], dtype=torch.int16 if dtype.itemsize == 2 else torch.uint8)
        assert torch.isnan(raw.view(dtype).float()).all()


def test_the_table_has_the_cases_the_module_claims():
    names = {m[0] for m in _MAPS}
    assert {f"read:{n}" for n in A.READ_CASES} <= names and {f"write:{n}" for n in A.WRITE_CASES} <= names
    assert {"compact", "round-trip"} <= names
    pages = {m[4].geom.bs for m in _MAPS}
    assert pages == {16, 32, 48}
    assert {m[4].geom.elem_bytes for m in _MAPS} == {1, 2}
    assert any(m[4].geom.layers > 32 for m in _MAPS)
    c = A.compaction_case()
    assert max(int(n) for n in c.nacc) > 16 and c.layers > 32


@pytest.mark.parametrize("entry", _MAPS, ids=_IDS)
def test_the_map_keeps_its_rules(entry):
    name, layout, flip, case, pm = entry
    read_bands = A.check_map(pm)                       # injective, disjoint, poison off the used pages, (a)
    assert read_bands == {"L", "M", "H"}
    A.check_boundaries(pm)                             # (b), (c)
    assert pm.stride_bytes == (pm.pb if layout == "shifted" else pm.unit * pm.pb)
    if layout == "interleaved":
        assert pm.stride_bytes != pm.pb                # a block stride that is not the page
    # K and V of a page are different physical pages, one page apart
    bases = pm.view_bases()
    assert bases[1] - bases[0] == pm.pb and len(set(bases)) == pm.unit
    # every page is in a band proper, except the pages that straddle a boundary (pages of 48 tokens, 33 layers)
    odd = [int(o) for o in pm.offset if A.strict_band(int(o), pm.pb) is None]
    assert all(o < b < o + pm.pb for o in odd for b in [A.B31 if o < A.B31 else A.B32])
    if (A.B32 % pm.slot_bytes) and (A.B32 % pm.slot_bytes) < pm.pb:
        assert odd, "a page whose view-relative extent straddles 2^32 exists and is used"


def test_first_and_last_pages_reach_H_and_M():
    """(d), per case and layout: over the case's flips (one flip wherever one map can do it)."""
    seen = {}
    for name, layout, flip, case, pm in _MAPS:
        f, l = A.first_last_bands(pm)
        e = seen.setdefault((name, layout), [set(), set(), 0])
        e[0] |= f
        e[1] |= l
        e[2] += 1
    for (name, layout), (f, l, n) in seen.items():
        assert {"H", "M"} <= f and {"H", "M"} <= l, (name, layout, f, l)
    # two flips only where the step has one request, or one first page for all
    for name, (build, kind, kw, flips, layers) in A.READ_CASES.items():
        c = build()
        firsts = {int(c.bt[i, 0]) for i in range(len(c.ctxs))}
        assert (len(flips) == 2) == (len(firsts) == 1), name


@pytest.mark.parametrize("mutant", A.MUTANTS)
@pytest.mark.parametrize("entry", _MAPS, ids=_IDS)
def test_a_narrowed_product_reads_poison(entry, mutant):
    name, layout, flip, case, pm = entry
    g = pm.geom
    row_bytes = g.Hkv * g.D * g.elem_bytes
    poison = pm.poison()
    straddles = (A.B32 % pm.slot_bytes) != 0 and (A.B32 % pm.slot_bytes) < pm.pb
    differing_requests = 0
    per_request = A.reads(pm, case.ctxs)
    for ids, in_page in per_request:
        exact = A.address(ids, in_page, pm.stride_bytes, g.elem_bytes)
        got = A.address(ids, in_page, pm.stride_bytes, g.elem_bytes, mutant)
        diff = got != exact
        for base in pm.view_bases():                  # K and V of every layer
            lo, hi = base + got, base + got + row_bytes
            assert (lo >= 0).all() and (hi <= A.TOTAL).all(), "a mutant address leaves the allocation"
            assert A.inside(poison, (base + got)[diff], row_bytes).all(), "a wrong address that is not poisoned"
            assert A.inside(pm.used(), (base + exact), row_bytes).all()
        differing_requests += bool(diff.any())
    if mutant == "in-page-low32":
        assert (differing_requests >= 1) == straddles, "bites exactly where a page straddles 2^32 behind its base"
    else:
        assert differing_requests == len(per_request), "a request every read of which the mutant gets right"


def test_the_pages_of_48_cases_have_a_page_astride_2_32_behind_its_base():
    """... so that the last mutant has something to bite on (the test above asserts that it does)."""
    hit = [m for m in _MAPS if m[4].geom.bs == 48 and m[0].startswith("read:")]
    assert len(hit) >= 4
    for name, layout, flip, case, pm in hit:
        assert pm.pb & (pm.pb - 1), "no power of two"
        assert 0 < A.B32 % pm.slot_bytes < pm.pb, name
