"""KV page addressing above 2 GiB and 4 GiB: the arena, the page map and the case table of tests/test_gpu_high_pages.py
(GPU) and tests/test_high_page_arena_host.py (the CPU proof that a kernel with a narrowed page product fails those tests).
Plain Python + torch; nothing here needs a GPU to import.

The arena is one byte buffer
    | guard: 2^32 bytes | cache span: 2^32 + 2^26 bytes |
with the cache base at the start of the span.  Only the pages a case uses are ever written.

Views.  A case with geometry (bs, Hkv, D, elem_bytes) and `layers` layers sees the span as 2 * layers caches
[nb, bs, Hkv, D] — K and V of every layer — in one of two layouts.  With pb the bytes of a page and U = 2 * layers:
  shifted      view number ph (K of layer l: 2 l, V of layer l: 2 l + 1) starts ph pages behind the base and has the
               contiguous block stride pb; the map uses the page ids U s only (even ids, for one layer), so that page id
               U s of view ph is physical page U s + ph of the span;
  interleaved  span.view(nb, U, bs, Hkv, D)[:, ph]: the block stride is U pages, the map uses the ids s.
In both, slot s holds one page of every view, and that page lies O = s U pb bytes behind the base pointer OF ITS VIEW:
every view of a case forms the same products, which is what a kernel computes from (pointer, block table, block stride).

Bands of a page, by O:   L  2^27 <= O, O + pb <= 2^31      M  2^31 <= O, O + pb <= 2^32      H  2^32 <= O.
Every plausible narrowing of the product lands 2^32 bytes lower (the byte offset kept in int32 or uint32), or 2^33 lower
(the element offset of a 2-byte cache kept in int32); with the guard all of that is inside the allocation, so a narrowed
kernel reads or writes poison instead of faulting: `PageMap.poison` lists those regions, L begins above every one of them.

The map (build_map) places, for every case:
  a. consecutive logical pages of a request in different bands;
  b. the slots next to 2^31 and 2^32 — where U pb divides the boundary, the slot whose last page ends there and the slot
     whose first page starts there — and the span's last slot;
  c. where it does not (pages of 48 tokens, 33 layers), the slot that straddles each boundary, and its neighbour below;
  d. first pages and last pages of requests in H and in M.  One map cannot do that for a step of one request, or one whose
     requests all begin with the same page: such cases run with `flip` 0 and 1 (H and M trade places), and (d) holds over
     the two.  A straddling page counts to the band of its first byte.
A request of one page gets H: only there do all narrowings differ from the exact address."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import attention_fixtures as F
import fp8_codes as C
import prefix_group_fixtures as PG
import shared_prefix_fixtures as S
import tree_oracle as TO

GUARD = 1 << 32
SPAN = (1 << 32) + (1 << 26)
TOTAL = GUARD + SPAN
LAYOUTS = ("shifted", "interleaved")
B31, B32 = 1 << 31, 1 << 32
L_FLOOR = 1 << 27
NAN_PATTERN = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00, torch.float8_e4m3fn: 0x7F}
SENTINEL = 0xA5                         # the write tests' poison, every byte

Geometry = namedtuple("Geometry", "bs Hkv D elem_bytes layers")


def geometry(cache, layers=1):
    nb, bs, Hkv, D = cache.shape
    return Geometry(int(bs), int(Hkv), int(D), int(cache.element_size()), int(layers))


def page_bytes(g):
    return g.bs * g.Hkv * g.D * g.elem_bytes


def loose_band(O):
    return "H" if O >= B32 else "M" if O >= B31 else "L"


def strict_band(O, pb):
    if O >= B32:
        return "H"
    if O >= B31 and O + pb <= B32:
        return "M"
    if O >= L_FLOOR and O + pb <= B31:
        return "L"
    return None


class PageMap:
    """slot[p]: the slot of small page p.  Everything else follows from the geometry and the layout."""

    def __init__(self, geom, layout, slot, rows, specials):
        assert layout in LAYOUTS
        self.geom, self.layout = geom, layout
        self.slot = np.asarray(slot, dtype=np.int64)
        self.rows = rows                                   # per request: its logical pages (small ids)
        self.specials = specials                           # name -> slot, the slots of (b) / (c)
        self.pb = page_bytes(geom)
        self.unit = 2 * geom.layers
        self.slot_bytes = self.unit * self.pb
        self.ids = self.slot * self.unit if layout == "shifted" else self.slot.copy()
        self.stride_bytes = self.pb if layout == "shifted" else self.slot_bytes
        self.offset = self.slot * self.slot_bytes          # O of every small page, the same in every view
        assert np.array_equal(self.ids * self.stride_bytes, self.offset)

    def view_bases(self):
        """Arena byte offset of every view's base pointer, [K0, V0, K1, V1, ...]."""
        return [GUARD + ph * self.pb for ph in range(self.unit)]

    def used(self):
        """[(start, end)] in arena bytes: every page of every view the map names."""
        return [(b + int(o), b + int(o) + self.pb) for b in self.view_bases() for o in self.offset]

    def poison(self):
        """[(start, end)] in arena bytes: where a narrowed product puts each used page (those inside the arena)."""
        out = []
        for b in self.view_bases():
            for o in self.offset:
                for d in (B32,) + ((1 << 33,) if self.geom.elem_bytes == 2 else ()):
                    a = b + int(o) - d
                    if a >= 0 and a + self.pb <= TOTAL:
                        out.append((a, a + self.pb))
        return out

    def table(self, t):
        """A block table (or prefix table) of small ids -> arena ids, same dtype and shape."""
        return torch.from_numpy(self.ids)[t.long()].to(t.dtype)

    def index(self):
        """int64 [n_small]: views[...][index] = small cache copies the case's pages into a view."""
        return torch.from_numpy(self.ids.copy())

    def slots_of(self, small_slots):
        """A slot mapping (token slots page * bs + offset, -1 = padding) on the small cache -> on the views."""
        s = small_slots.long()
        bs = self.geom.bs
        moved = torch.from_numpy(self.ids)[s.clamp(min=0) // bs] * bs + s.clamp(min=0) % bs
        return torch.where(s < 0, s, moved)


def build_map(rows, n_small, geom, layout, flip=0, seed=0):
    """rows: per request the small page ids of its logical pages, in order (shared pages appear in several rows)."""
    pb = page_bytes(geom)
    sb = 2 * geom.layers * pb
    s31, s32, s_last = B31 // sb, B32 // sb, SPAN // sb - 1
    exact31, exact32 = B31 % sb == 0, B32 % sb == 0
    specials = {"below-2^31": s31 - 1, "at-2^31": s31, "below-2^32": s32 - 1, "at-2^32": s32, "last": s_last}
    rng = np.random.default_rng(seed)
    need = n_small + 8

    def pool(first, lo, hi):
        lo, hi = int(lo), int(hi)
        rest = lo + rng.choice(hi - lo, size=min(need, hi - lo), replace=False)
        return [int(x) for x in first] + [int(x) for x in rest]

    # the specials lead their pools: they go to the first requests' pages, which are read
    lo_l = -(-L_FLOOR // sb)
    pools = {
        "L": pool([s31 - 1] if exact31 else [s31, s31 - 1], lo_l, s31 - 1),
        "M": pool(([s32 - 1] if exact32 else [s32, s32 - 1]) + ([s31] if exact31 else []), s31 + 1, s32 - 1),
        "H": pool(([s32] if exact32 else []) + [s_last], s32 + 1, s_last),
    }
    for name, p in pools.items():
        for s in p:
            assert loose_band(s * sb) == name, (name, s)
    slot = np.full(n_small, -1, dtype=np.int64)
    band = {}
    nxt = {"H": "M", "M": "L", "L": "H"}

    def take(p, b):
        band[p] = b
        slot[p] = pools[b].pop(0)

    first_last = ("H", "M") if not flip else ("M", "H")
    for i, row in enumerate(rows):
        row = [int(p) for p in row]
        n = len(row)
        fb, lb = first_last if i % 2 == 0 else first_last[::-1]
        for j, p in enumerate(row):
            if p in band:
                continue
            prev = band[row[j - 1]] if j else None
            if n == 1:
                b = "H"
            elif j == 0:
                b = fb
            else:
                has_h = any(band.get(x) == "H" for x in row)
                cands = [x for x in (nxt[prev], nxt[nxt[prev]]) if not (j == n - 2 and x == lb)]
                if j == n - 1 and lb != prev:
                    cands = [lb] + cands
                b = "H" if (not has_h and "H" in cands) else cands[0]
            assert b != prev or n == 1
            take(p, b)
    b = "L"
    for p in range(n_small):                           # spare pages, the pages padded columns name
        if slot[p] < 0:
            take(p, b)
            b = nxt[b]
    return PageMap(geom, layout, slot, [[int(p) for p in r] for r in rows], specials)


def rows_of(bt, ctxs, bs):
    return [bt[i, :-(-int(c) // bs)].tolist() for i, c in enumerate(ctxs)]


def relocate(case, layout, flip=0, layers=1):
    """`case`: a namespace with kc, vc (or kcs / vcs: lists, one per layer), bt and ctxs, as the fixture builders return
    them.  Returns (moved case, PageMap): `bt`, and `prefix_table` where there is one, name arena pages; kc / vc are the
    small caches still (the oracle runs on the unrelocated case; the test copies them with map.index())."""
    cache = case.kc if hasattr(case, "kc") else case.kcs[0]
    geom = geometry(cache, layers)
    pm = build_map(rows_of(case.bt, case.ctxs, geom.bs), int(cache.shape[0]), geom, layout, flip)
    d = dict(vars(case))
    d["bt"] = pm.table(case.bt)
    if getattr(case, "prefix_table", None) is not None:
        d["prefix_table"] = pm.table(case.prefix_table)
    return SimpleNamespace(**d), pm


# ---- the properties (asserted on the CPU for every case; cheap enough to assert again where a map is used) ------------
def check_map(pm):
    """Injective, K / V / layers disjoint, nothing poisoned is used, every page inside a view.  Returns the bands read."""
    assert len(set(pm.slot.tolist())) == pm.slot.size and (pm.slot >= 0).all()
    used, poison = sorted(pm.used()), sorted(pm.poison())
    for (a0, a1), (b0, b1) in zip(used, used[1:]):
        assert a1 <= b0, "two used pages overlap"
    assert used[0][0] >= GUARD + L_FLOOR and used[-1][1] <= TOTAL
    starts = np.array([u[0] for u in used])
    ends = np.array([u[1] for u in used])
    for p0, p1 in poison:
        assert 0 <= p0 and p1 <= TOTAL
        k = np.searchsorted(ends, p0, side="right")
        assert k == len(used) or starts[k] >= p1, "a poisoned region overlaps a used page"
    nb = views_blocks(pm.geom, pm.layout)
    assert int(pm.ids.max()) < nb
    for row in pm.rows:                                             # (a)
        bands = [loose_band(int(pm.offset[p])) for p in row]
        assert all(x != y for x, y in zip(bands, bands[1:])), bands
    return {loose_band(int(pm.offset[p])) for row in pm.rows for p in row}


def check_boundaries(pm):
    """(b) / (c): the slots at the two boundaries and the last slot are used; what they are, by arithmetic."""
    sb, pb = pm.slot_bytes, pm.pb
    have = set(pm.slot.tolist())
    sp = pm.specials
    for name, s in sp.items():
        assert s in have, name
    for bound, below, at in ((B31, sp["below-2^31"], sp["at-2^31"]), (B32, sp["below-2^32"], sp["at-2^32"])):
        if bound % sb == 0:
            assert (below + 1) * sb == bound and at * sb == bound      # a page ends exactly there, a page starts there
        else:
            assert at * sb < bound < (at + 1) * sb                     # (c) the slot straddles the boundary ...
            if bound % pb:                                             # ... and so does one of its pages
                ph = (bound - at * sb) // pb
                assert at * sb + ph * pb < bound < at * sb + (ph + 1) * pb
    assert (sp["last"] + 2) * sb > SPAN >= (sp["last"] + 1) * sb       # the span's last whole slot


def first_last_bands(pm):
    firsts = {loose_band(int(pm.offset[r[0]])) for r in pm.rows}
    lasts = {loose_band(int(pm.offset[r[-1]])) for r in pm.rows}
    return firsts, lasts


def views_blocks(geom, layout):
    """num_blocks of every view."""
    pb = page_bytes(geom)
    unit = 2 * geom.layers
    return (SPAN - (unit - 1) * pb) // pb if layout == "shifted" else SPAN // (unit * pb)


# ---- the arena itself (tests/test_gpu_high_pages.py allocates it once) -------------------------------------------------
class Arena:
    def __init__(self, device):
        self.buf = torch.empty(TOTAL, dtype=torch.uint8, device=device)

    def views(self, geom, layout, dtype):
        """[(K, V)] per layer: [nb, bs, Hkv, D] views of the span."""
        pb = page_bytes(geom)
        unit = 2 * geom.layers
        nb = views_blocks(geom, layout)
        span = self.buf[GUARD:]
        assert torch.empty(0, dtype=dtype).element_size() == geom.elem_bytes
        if layout == "shifted":
            vs = [span[ph * pb:(ph + nb) * pb].view(dtype).view(nb, geom.bs, geom.Hkv, geom.D) for ph in range(unit)]
        else:
            whole = span[:nb * unit * pb].view(dtype).view(nb, unit, geom.bs, geom.Hkv, geom.D)
            vs = [whole[:, ph] for ph in range(unit)]
        return [(vs[2 * l], vs[2 * l + 1]) for l in range(geom.layers)]

    def load(self, pm, views, kcs, vcs):
        idx = pm.index().to(self.buf.device)
        for (kv, vv), kc, vc in zip(views, kcs, vcs):
            kv.view(torch.uint8)[idx] = kc.to(self.buf.device).view(torch.uint8)
            vv.view(torch.uint8)[idx] = vc.to(self.buf.device).view(torch.uint8)

    def fill(self, regions, pattern, width):
        for a, b in regions:
            if width == 2:
                self.buf[a:b].view(torch.int16).fill_(pattern - (1 << 16) if pattern >= 1 << 15 else pattern)
            else:
                self.buf[a:b].fill_(pattern)

    def holds(self, regions, byte):
        """Every byte of every region is `byte` (one synchronisation)."""
        if not regions:
            return True
        return bool(torch.stack([(self.buf[a:b] == byte).all() for a, b in regions]).all())

    def neighbours(self, pm):
        """[(start, end)]: the physical page below and above every used slot that belongs to no used slot itself."""
        have = set(pm.slot.tolist())
        out = []
        for s in sorted(have):
            if s - 1 not in have:
                out.append((GUARD + s * pm.slot_bytes - pm.pb, GUARD + s * pm.slot_bytes))
            if s + 1 not in have and GUARD + (s + 1) * pm.slot_bytes + pm.pb <= TOTAL:
                out.append((GUARD + (s + 1) * pm.slot_bytes, GUARD + (s + 1) * pm.slot_bytes + pm.pb))
        return out

    def snapshot(self, regions):
        return [self.buf[a:b].clone() for a, b in regions]

    def unchanged(self, regions, snap):
        return all(torch.equal(self.buf[a:b], s) for (a, b), s in zip(regions, snap))


# ---- the address computation, exact and narrowed (numpy, offsets only) -------------------------------------------------
MUTANTS = ("bytes-int32", "bytes-uint32", "elems-int32", "in-page-low32")


def _wrap32(x, signed):
    x = np.asarray(x, dtype=np.int64) & 0xFFFFFFFF
    return np.where(x >= (1 << 31), x - (1 << 32), x) if signed else x


def address(ids, in_page, stride_bytes, elem_bytes, mutant=None):
    """Byte offset from a view's base pointer of byte `in_page` of page `ids` (int64 arrays), as the kernels form it —
    page * block_stride + offset inside the page — exactly, or with one step narrowed."""
    ids = np.asarray(ids, dtype=np.int64)
    in_page = np.asarray(in_page, dtype=np.int64)
    prod = ids * stride_bytes
    if mutant is None:
        return prod + in_page
    if mutant == "bytes-int32":
        return _wrap32(prod, True) + in_page
    if mutant == "bytes-uint32":
        return _wrap32(prod, False) + in_page
    if mutant == "elems-int32":
        return _wrap32(ids * (stride_bytes // elem_bytes), True) * elem_bytes + in_page
    assert mutant == "in-page-low32"                     # a 64-bit page base, the offset added in the low word only
    return (prod & ~np.int64(0xFFFFFFFF)) | ((prod + in_page) & 0xFFFFFFFF)


def reads(pm, ctxs):
    """Per request: (arena ids, in-page byte offsets) of the first byte of every token row below its context, through
    the relocated rows.  The same for K and V and every layer (relative to the view's base)."""
    bs, row_bytes = pm.geom.bs, pm.geom.Hkv * pm.geom.D * pm.geom.elem_bytes
    out = []
    for row, ctx in zip(pm.rows, ctxs):
        tok = np.arange(int(ctx))
        ids = pm.ids[np.asarray(row, dtype=np.int64)[tok // bs]]
        out.append((ids, (tok % bs) * row_bytes))
    return out


def inside(regions, addr, length):
    """bool per address: [addr, addr + length) lies inside one of the (sorted, disjoint after merging) regions."""
    regions = sorted(regions)
    merged = []
    for a, b in regions:
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    starts = np.array([m[0] for m in merged], dtype=np.int64)
    ends = np.array([m[1] for m in merged], dtype=np.int64)
    addr = np.asarray(addr, dtype=np.int64)
    k = np.searchsorted(starts, addr, side="right") - 1
    ok = k >= 0
    k = np.maximum(k, 0)
    return ok & (addr >= starts[k]) & (addr + length <= ends[k])


# ---- the case table: what tests/test_gpu_high_pages.py runs, and what the host proof covers ---------------------------
def _sinks(Hq, seed):
    return (torch.randn(Hq, generator=torch.Generator().manual_seed(seed)) * 2).float()


def _fp16(c):
    c.q, c.kc, c.vc = c.q.to(torch.float16), c.kc.to(torch.float16), c.vc.to(torch.float16)
    return c


def _tree(trees, ctxs, Hq, Hkv, seed, fp8=False):
    c = TO.attention_case(trees, ctxs, Hq, Hkv, 128, 16, seed, fp8=fp8)
    c.trees = trees
    return c


_MIXED = ([4, 33, 2, 9], [130, 200, 64, 97])
_SHORT = ([1, 4, 2, 3], [130, 200, 64, 97])


def _shared_prefix():
    q_lens, P = [1, 9, 3], 32
    ctxs = [P + e + q for q, e in zip(q_lens, [0, 20, 66])]
    return S.share_prefix(F.planted_case(q_lens, ctxs, 16, 4, 128, 16, seed=3), P)


def _prefix_groups():
    q_lens, req_group, group_len = [1, 4, 2, 3, 9, 1], [0, 1, -1, 0, 1, 0], [64, 96]
    ctxs = [(group_len[g] if g >= 0 else 0) + e + q for q, e, g in zip(q_lens, [0, 5, 18, 40, 0, 70], req_group)]
    return PG.share_in_groups(F.planted_case(q_lens, ctxs, 16, 4, 128, 32, seed=4), req_group, group_len)


def _tree_trees():
    return [TO.random_tree(32, np.random.default_rng(14), 0.6), TO.random_tree(6, np.random.default_rng(15), 0.8)]


# name -> (builder of the small case, call kind, keyword arguments of the call, flips, layers)
#   verify: ops.verify_attention(host_lens=, num_splits_max=);  prefix / groups: its shared-prefix forms;
#   tree: ops.verify_attention_tree;  step: ops.step_attention;  plan-run / plan-layers: VerifyAttentionPlan on two layers
READ_CASES = {
    # the bodies of verify_attention, D 128 bf16 in pages of 16
    "short-generic": (lambda: F.planted_case(*_SHORT, 8, 2, 128, 16, seed=11), "verify", dict(host_lens=False), (0,), 1),
    "short-layouts": (lambda: F.planted_case(*_SHORT, 8, 2, 128, 16, seed=11), "verify", dict(host_lens=True), (0,), 1),
    "long-draft-dma": (lambda: F.planted_case([33], [200], 8, 2, 128, 16, seed=12), "verify", dict(host_lens=True), (0, 1), 1),
    "mixed-pair": (lambda: F.planted_case(*_MIXED, 8, 2, 128, 16, seed=13), "verify", dict(host_lens=True), (0,), 1),
    "split-combine": (lambda: F.planted_case([2, 1, 3], [300, 257, 290], 16, 4, 128, 16, seed=14), "verify",
                      dict(host_lens=False, num_splits_max=3), (0,), 1),
    "split-combine-layouts": (lambda: F.planted_case([2, 1, 3], [300, 257, 290], 16, 4, 128, 16, seed=14), "verify",
                              dict(host_lens=True, num_splits_max=3), (0,), 1),
    # the cache kinds
    "f16-mixed": (lambda: _fp16(F.planted_case(*_MIXED, 8, 2, 128, 16, seed=15)), "verify", dict(host_lens=True), (0,), 1),
    "f16-generic": (lambda: _fp16(F.planted_case(*_SHORT, 8, 2, 128, 16, seed=16)), "verify", dict(host_lens=False), (0,), 1),
    "e4m3-mixed": (lambda: C.uniform_case(*_MIXED, 8, 2, 16, seed=2, dtype=torch.bfloat16), "verify", dict(host_lens=True),
                   (0,), 1),
    "e4m3-generic": (lambda: C.uniform_case(*_SHORT, 8, 2, 16, seed=7, dtype=torch.bfloat16), "verify",
                     dict(host_lens=False), (0,), 1),
    "d64-window-sinks": (lambda: F.planted_case(*_MIXED, 8, 2, 64, 16, seed=17, window=128, sinks=_sinks(8, 17)), "verify",
                         dict(host_lens=True), (0,), 1),
    "d64-window-sinks-generic": (lambda: F.planted_case(*_SHORT, 8, 2, 64, 16, seed=18, window=128, sinks=_sinks(8, 18)),
                                 "verify", dict(host_lens=False), (0,), 1),
    "pages-32": (lambda: F.planted_case(*_MIXED, 8, 2, 128, 32, seed=19), "verify", dict(host_lens=True), (0,), 1),
    "pages-48": (lambda: F.planted_case(*_MIXED, 8, 2, 128, 48, seed=20), "verify", dict(host_lens=True), (0,), 1),
    "pages-48-generic": (lambda: F.planted_case([3, 4, 2, 1], [200, 150, 97, 250], 8, 2, 128, 48, seed=21), "verify",
                         dict(host_lens=False), (0,), 1),
    "pages-48-e4m3": (lambda: C.uniform_case([3, 33, 2, 9], [200, 250, 64, 97], 8, 4, 48, seed=8, dtype=torch.bfloat16),
                      "verify", dict(host_lens=True), (0,), 1),
    # the other calls
    "shared-prefix": (_shared_prefix, "prefix", {}, (0, 1), 1),
    "prefix-groups": (_prefix_groups, "groups", {}, (0,), 1),
    "tree": (lambda: _tree(_tree_trees(), [200, 95], 8, 2, 5), "tree", {}, (0,), 1),
    "tree-e4m3": (lambda: _tree(_tree_trees(), [200, 95], 8, 2, 6, fp8=True), "tree", {}, (0,), 1),
    "step-chunk": (lambda: F.planted_case([40, 3], [100, 64], 8, 2, 128, 16, seed=22), "step", {}, (0,), 1),
    "step-chunk-window": (lambda: F.planted_case([40, 3], [200, 164], 8, 2, 64, 16, seed=23, window=128,
                                                 sinks=_sinks(8, 23)), "step", {}, (0,), 1),
    "plan-run": (lambda: F.planted_case(*_MIXED, 8, 2, 128, 16, seed=24), "plan-run", {}, (0,), 2),
    "plan-layers": (lambda: F.planted_case(*_MIXED, 8, 2, 128, 16, seed=25), "plan-layers", {}, (0,), 2),
}


def _bulk(dtype, kv, H, Dh, bs, layers, T=40):
    """A bulk write of T tokens into pages of their own (some padded, -1) behind a block table of one 'request' per 3
    pages, so that the map's rules apply to the destinations."""
    n_pages = -(-T // bs) + 6
    per = 3
    B = -(-n_pages // per)
    bt = torch.arange(B * per, dtype=torch.int32).view(B, per)
    g = torch.Generator().manual_seed(T + H + Dh)
    slots = torch.randperm(n_pages * bs, generator=g)[:T].to(torch.int64)
    slots[5] = -1
    eb = 1 if kv != "auto" else 2
    cache_dtype = torch.float8_e4m3fn if kv != "auto" else dtype
    mk = lambda: torch.randint(0, 256, (B * per, bs, H, Dh * eb), generator=g, dtype=torch.int32).to(torch.uint8) \
        .view(cache_dtype)
    return SimpleNamespace(bt=bt, ctxs=[per * bs] * B, kcs=[mk() for _ in range(layers)], vcs=[mk() for _ in range(layers)],
                           slots=slots, src_dtype=dtype, kv=kv, H=H, Dh=Dh, bs=bs, T=T, layers=layers,
                           keys=torch.randn(T, layers * H * Dh, generator=g), values=torch.randn(T, layers * H * Dh, generator=g))


# name -> (builder, layers): reshape_and_cache_flash_bulk.  16-byte path: rows and strides multiples of 16 bytes.
WRITE_CASES = {
    "bf16-copy-16-byte": (lambda: _bulk(torch.bfloat16, "auto", 2, 128, 16, 2), 2),
    "f16-copy-16-byte": (lambda: _bulk(torch.float16, "auto", 2, 64, 16, 1), 1),
    "bf16-copy-scalar": (lambda: _bulk(torch.bfloat16, "auto", 3, 20, 16, 2), 2),       # rows of 120 bytes
    "e4m3-quantise-16-byte": (lambda: _bulk(torch.bfloat16, "fp8_e4m3", 2, 128, 16, 2), 2),
    "e4m3-quantise-scalar": (lambda: _bulk(torch.float16, "fp8_e4m3", 3, 20, 16, 2), 2),   # rows of 60 bytes
    "e4m3-pages-48": (lambda: _bulk(torch.bfloat16, "fp8_e4m3", 4, 128, 48, 1, T=150), 1),
}
WRITE_SCALES = (0.75, 3.1)


def compaction_case(layers=33):
    """compact_accepted_paths: a 33-node chain geometry whose accepted path has 20 nodes (more than one pass of 16 rows)
    and crosses two page borders, a path of 7 across one border, n_path = 1 and the identity; `layers` > 32: two launches."""
    bs, Hkv, D = 16, 1, 64
    reqs = [(33, 45, [0, 2, 3, 5, 6, 8, 9, 11, 13, 14, 16, 17, 19, 21, 22, 24, 26, 28, 30, 32]),
            (21, 48, [0, 3, 4, 9, 15, 16, 20]), (9, 100, [0]), (4, 33, [0, 1, 2]), (5, 40, [0, 2, 3])]
    q_lens, ctxs = [r[0] for r in reqs], [r[1] for r in reqs]
    g = torch.Generator().manual_seed(31)
    nblk = [-(-c // bs) for c in ctxs]
    nb = sum(nblk) + 2
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(reqs), max(nblk), dtype=torch.int32)
    p = 0
    for i, k in enumerate(nblk):
        bt[i, :k] = perm[p:p + k].to(torch.int32)
        p += k
    mk = lambda: torch.randint(0, 256, (nb, bs, Hkv, D * 2), generator=g, dtype=torch.int32).to(torch.uint8) \
        .view(torch.bfloat16)
    W = max(q_lens)
    path = np.full((len(reqs), W), -1, dtype=np.int32)
    for i, r in enumerate(reqs):
        path[i, :len(r[2])] = r[2]
    return SimpleNamespace(bt=bt, ctxs=ctxs, q_lens=q_lens, kcs=[mk() for _ in range(layers)], vcs=[mk() for _ in range(layers)],
                           path=path, nacc=np.array([len(r[2]) for r in reqs], dtype=np.int32), layers=layers, bs=bs)


def round_trip_case():
    """fp8_codes' round trip (bulk write, then attention on what was written) as a case the map can move."""
    R = C.ROUND_TRIP
    bs = 16
    g = torch.Generator().manual_seed(9)
    nblk = [c // bs for c in R["ctxs"]]
    nb = sum(nblk) + 2
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(nblk), max(nblk), dtype=torch.int32)
    slots, k = [], 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[k:k + n].to(torch.int32)
        slots += [int(bt[i, t // bs]) * bs + t % bs for t in range(R["ctxs"][i])]
        k += n
    zero = lambda: torch.zeros(nb, bs, R["Hkv"], C.D, dtype=torch.uint8).view(torch.float8_e4m3fn)
    q = torch.randn(sum(R["q_lens"]), R["Hq"], C.D, generator=g).to(torch.bfloat16)
    return SimpleNamespace(bt=bt, ctxs=list(R["ctxs"]), q_lens=list(R["q_lens"]), kcs=[zero()], vcs=[zero()],
                           slots=torch.tensor(slots, dtype=torch.int64), q=q, nb=nb, bs=bs, Hq=R["Hq"], Hkv=R["Hkv"])


def all_maps():
    """(name, layout, flip, case, PageMap) for everything the GPU module relocates: the host proof's domain."""
    for name, (build, kind, kw, flips, layers) in READ_CASES.items():
        c = build()
        for layout in LAYOUTS:
            for flip in flips:
                yield f"read:{name}", layout, flip, c, relocate(c, layout, flip, layers)[1]
    for name, (build, layers) in WRITE_CASES.items():
        c = build()
        for layout in LAYOUTS:
            yield f"write:{name}", layout, 0, c, relocate(c, layout, 0, layers)[1]
    c = compaction_case()
    for layout in LAYOUTS:
        yield "compact", layout, 0, c, relocate(c, layout, 0, c.layers)[1]
    c = round_trip_case()
    for layout in LAYOUTS:
        yield "round-trip", layout, 0, c, relocate(c, layout, 0, 1)[1]
