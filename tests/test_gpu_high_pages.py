"""GPU: every paged kernel on pages that lie more than 2 GiB and more than 4 GiB behind the cache pointer, which is where a
production cache has them (one layer's K of a (2, num_blocks, block_size, Hkv, D) cache on a 288 GB card is 3.5 GiB and
up) and where no other test of the suite puts one.  tests/high_page_arena.py has the arena (a 2^32-byte guard, then a
span of 2^32 + 2^26 bytes viewed as caches in two layouts, one of them with a block stride that is not the page), the
page map and the case table; tests/test_high_page_arena_host.py proves on offsets alone that a page product narrowed to
32 bits, in any of four ways, makes every case below read or write poison — inside the allocation, so it shows as a
mismatch and not as a fault.

  reads    each body of ops.verify_attention (generic, short layouts, long-draft DMA, the mixed pair, split + combine),
           each cache kind (bf16 / fp16 / e4m3 at D 128, bf16 at D 64 with a window and sinks, pages of 16 / 32 / 48),
           shared_prefix_len, prefix_groups, verify_attention_tree, step_attention with a 40-token chunk (plain and
           windowed), VerifyAttentionPlan.run / run_layers over two layers.  The aliases of every used page hold the NaN
           pattern of the cache dtype, the output is pre-filled with NaN, and the result is checked (i) against the
           oracle on the small, unrelocated case at the project's bar, atol 1e-3 + rtol 2^-8, all finite, and (ii) for
           bit-equality with the same call on the compact cache: the addresses are all that differs.
  writes   reshape_and_cache_flash_bulk (same-type copies, e4m3 quantising, the 16-byte and the scalar path, two layers)
           and compact_accepted_paths (a 20-node path: two passes of 16 rows; 33 layers: two launches): the destination
           pages byte-exact, every alias still holding its sentinel, the pages next to the used slots unchanged.
  and one round trip: bulk write into high pages, then verify_attention on what was written.

The arena (about 8.1 GiB) is allocated once for the module; the module skips only where the device has less free memory
than the arena plus 2 GiB, which an MI355X never has.

What these tests pin — every expression that forms a cache address, as read when they were written (all wide enough):
  verify_attn.hip  436-437   generic / short / tree body: u32 page * u64 block_stride (elements) + u32 in-page elements,
                             the sum in 64 bits; 454-455, 469-472: pointer + i64 base * ES + u32 per-lane bytes
                             (__umul24(row <= 15, row_bytes < 2^24) + 16 chunk)
                   1212      long-draft DMA body (group_base): u64(u32 page) * u64 stride_bytes + u32 in-page bytes;
                             1222-1234 pointer + u64; 1194-1197 / 1224 per-lane u32 byte offset handed to the LDS-DMA load
                             beside the 64-bit scalar base (glds16s, 977)
                   355, 1035 block-table row: i64 request * max_blocks
  prefill_attn.hip 177       i64 page * i64 block_stride + i64 in-page row * kv_row + head; 187, 194-195: size_t base * ES
                             + u32 (__umul24) per-lane bytes
  prefix_attn.hip  126       the same product; 133, 138-139 the same per-lane form
  kv_bulk_write.hip 75-82    i64 slot / block_size -> i64 block * i64 block_stride + i64 in-page; 80-81 source rows i64
  kv_compact.hip   68        int page * i64 block_stride_bytes + i64 row * row_bytes + column
The in-page 32-bit offsets are deliberate (a page is far below 4 GiB); the page products are what must stay 64-bit.  With
each product narrowed to 32 bits (one build, every kernel above) all 68 tests of this module fail, none faults."""
import functools
import time

import numpy as np
import pytest
import torch

import attention_fixtures as F
import fp8_codes as C
import high_page_arena as A
import tree_oracle as TO
from oracle import spec_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = 1e-3, 2 ** -8


def _ops():
    from arcticinference_amd import ops
    return ops


@pytest.fixture(scope="module")
def arena():
    free, total = torch.cuda.mem_get_info()
    need = A.TOTAL + (2 << 30)
    if free < need:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the arena needs {need / 2 ** 30:.1f} GiB")
    t0 = time.perf_counter()
    a = A.Arena(DEV)
    torch.cuda.synchronize()
    print(f"high-page arena: {A.TOTAL / 2 ** 30:.2f} GiB allocated in {time.perf_counter() - t0:.3f} s, "
          f"{free / 2 ** 30:.1f} GiB were free of {total / 2 ** 30:.1f}")
    yield a
    del a.buf
    torch.cuda.empty_cache()


# ---- reads ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _read_case(name):
    """(small case, per-layer small caches, per-layer oracle): built and computed once, shared by layouts and flips."""
    build, kind, kw, flips, layers = A.READ_CASES[name]
    c = build()
    want = TO.case_oracle(c) if kind == "tree" else F.oracle(c)
    # a second layer: the same keys, V negated — its attention is the first layer's, negated
    caches = [(c.kc, c.vc)] + [(c.kc, -c.vc) for _ in range(layers - 1)]
    return c, caches, [want] + [-want for _ in range(layers - 1)]


def _run(kind, c, caches, kw):
    """The call of `kind` on case c (its block table names pages of `caches`, [(K, V)] per layer, on the device).
    Returns the outputs per layer checked, float32 on the CPU."""
    ops = _ops()
    q = c.q.to(DEV)
    bt = c.bt.to(DEV)
    seq = torch.tensor(c.ctxs, dtype=torch.int32, device=DEV)
    extra = {}
    if c.ks is not None:
        extra.update(k_scale=torch.tensor([c.ks], dtype=torch.float32, device=DEV),
                     v_scale=torch.tensor([c.vs], dtype=torch.float32, device=DEV))
    if getattr(c, "sinks", None) is not None:
        extra["sinks"] = c.sinks.to(DEV)
    if getattr(c, "window", 0):
        extra["sliding_window"] = c.window
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    k, v = caches[0]
    if kind == "tree":
        ops.verify_attention_tree(q, k, v, bt, seq, ops.TreeDrafts(c.trees, DEV), max(c.ctxs), c.scale, out=out, **extra)
        torch.cuda.synchronize()
        return [out.float().cpu()]
    qsl = torch.tensor(c.qsl, device=DEV)
    if kind == "step":
        ops.step_attention(q, k, v, bt, seq, qsl, max(c.ctxs), c.scale, q_lens_host=c.q_lens, out=out, **extra)
    elif kind in ("verify", "prefix", "groups"):
        if kind == "prefix":
            extra.update(shared_prefix_len=c.shared_len, prefix_block_table=c.prefix_table.to(DEV), seq_lens_host=c.ctxs)
        if kind == "groups":
            extra.update(prefix_groups=ops.PrefixGroups(c.req_group, c.group_len, c.q_lens, torch.device(DEV)),
                         seq_lens_host=c.ctxs)
        host_lens = kw.get("host_lens", True)
        ops.verify_attention(q, k, v, bt, seq, qsl, max(c.q_lens), max(c.ctxs), c.scale, out=out,
                             q_lens_host=c.q_lens if host_lens else None, num_splits_max=kw.get("num_splits_max", 64), **extra)
    else:
        rs = ops.split_requests(c.q_lens, c.Hq // c.Hkv, DEV)
        if kind == "plan-run":
            plan = ops.VerifyAttentionPlan(q, out, k, bt, seq, qsl, max(c.q_lens), max(c.ctxs), c.scale, req_split=rs)
            outs = []
            for kl, vl in caches:
                out.fill_(float("nan"))
                plan.run(kl, vl)
                torch.cuda.synchronize()
                outs.append(out.float().cpu())
            return outs
        assert kind == "plan-layers"
        from arcticinference_amd import _native as N
        L = len(caches)
        # q / out advance per layer (layer stride = one q), so every layer's result is checked ...
        qs = torch.stack([q] * L).contiguous()
        outs = torch.full_like(qs, float("nan"))
        plan = ops.VerifyAttentionPlan(qs[0], outs[0], k, bt, seq, qsl, max(c.q_lens), max(c.ctxs), c.scale, req_split=rs)
        tables = plan.layer_tables([kl for kl, _ in caches], [vl for _, vl in caches])
        a = plan._args
        N.check(N.lib().aic_verify_attention_layers(a[0], a[1], qs.stride(0), tables[0], tables[1], tables[2], *a[4:20],
                                                    a[20], a[21], outs.stride(0), *a[22:]))
        torch.cuda.synchronize()
        res = [outs[l].float().cpu() for l in range(L)]
        # ... and the public form, in which every layer writes the one out: the last layer's result stays
        outs[0].fill_(float("nan"))
        plan.run_layers(tables)
        torch.cuda.synchronize()
        assert torch.equal(outs[0].float().cpu(), res[-1])
        return res
    torch.cuda.synchronize()
    return [out.float().cpu()]


_READ = [(name, flip) for name, entry in A.READ_CASES.items() for flip in entry[3]]


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("name,flip", _READ, ids=[f"{n}-flip{f}" for n, f in _READ])
def test_attention_reads_high_pages(arena, name, flip, layout):
    build, kind, kw, flips, layers = A.READ_CASES[name]
    c, small, wants = _read_case(name)
    r, pm = A.relocate(c, layout, flip, layers)
    A.check_map(pm)
    dtype = c.kc.dtype
    views = arena.views(pm.geom, layout, dtype)
    assert views[0][0].stride(0) * pm.geom.elem_bytes == pm.stride_bytes
    arena.load(pm, views, [k for k, _ in small], [v for _, v in small])
    arena.fill(pm.poison(), A.NAN_PATTERN[dtype], pm.geom.elem_bytes)
    compact = _run(kind, c, [(k.to(DEV), v.to(DEV)) for k, v in small], kw)
    moved = _run(kind, r, views, kw)
    for l, (got, base, want) in enumerate(zip(moved, compact, wants)):
        err = (got - want).abs()
        worst = float((err / (ATOL + RTOL * want.abs())).max())
        same = torch.equal(got, base)
        print(f"{name} {layout} flip {flip} layer {l}: max abs err {float(err.max()):.4g}, worst err / bar {worst:.3f}, "
              f"bit-equal to the compact cache: {same}")
        assert torch.isfinite(got).all(), f"layer {l}: non-finite output (poison was read, or a row was not written)"
        assert worst <= 1, f"layer {l}: misses the bar against the oracle"                         # (i)
        assert same, f"layer {l}: differs from the same call on the compact cache"                 # (ii)


# ---- writes -----------------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _gather(view, pm):
    """The case's pages of a view, in small-page order, as bytes [n_small, bs, row bytes]."""
    idx = pm.index().to(DEV)
    return view.view(torch.uint8)[idx].cpu().numpy().reshape(idx.numel(), pm.geom.bs, -1)


@pytest.mark.parametrize("layout", A.LAYOUTS)
@pytest.mark.parametrize("name", list(A.WRITE_CASES))
def test_bulk_write_into_high_pages(arena, name, layout):
    build, layers = A.WRITE_CASES[name]
    c = build()
    r, pm = A.relocate(c, layout, 0, layers)
    A.check_map(pm)
    views = arena.views(pm.geom, layout, c.kcs[0].dtype)
    arena.load(pm, views, c.kcs, c.vcs)
    poison, nbr = pm.poison(), arena.neighbours(pm)
    arena.fill(poison, A.SENTINEL, 1)
    snap = arena.snapshot(nbr)
    keys, values = c.keys.to(c.src_dtype), c.values.to(c.src_dtype)
    scales = [torch.tensor(s, dtype=torch.float32, device=DEV) for s in A.WRITE_SCALES]
    n = c.H * c.Dh
    path16 = (n * keys.element_size()) % 16 == 0
    assert path16 == ("16-byte" in name or "pages-48" in name)
    _ops().reshape_and_cache_flash_bulk(keys.to(DEV), values.to(DEV), [k for k, _ in views], [v for _, v in views],
                                        pm.slots_of(c.slots).to(DEV), c.kv, [scales[0]] * layers, [scales[1]] * layers,
                                        c.H, c.Dh)
    torch.cuda.synchronize()
    slots = c.slots.numpy()
    live = slots >= 0
    assert (~live).any() and live.sum() > 30
    for l in range(layers):
        for (src, small, view, scale) in ((keys, c.kcs[l], views[l][0], A.WRITE_SCALES[0]),
                                          (values, c.vcs[l], views[l][1], A.WRITE_SCALES[1])):
            rows = src[:, l * n:(l + 1) * n]
            if c.kv == "auto":
                new = _bytes(rows).reshape(c.T, -1)
            else:
                e = C.encode(C.divide(rows.float().numpy(), scale), "e4m3fn")
                assert not e.nan.any()
                new = e.code
            want = _bytes(small).reshape(-1, new.shape[1]).copy()          # [slots of the small cache, row bytes]
            want[slots[live]] = new[live]
            got = _gather(view, pm).reshape(-1, new.shape[1])
            assert np.array_equal(got, want), (name, layout, l)            # destination rows AND the rest of their pages
    assert arena.holds(poison, A.SENTINEL), "a write landed 2^32 or 2^33 bytes below its page"
    assert arena.unchanged(nbr, snap), "a page next to a destination slot changed"


@pytest.mark.parametrize("layout", A.LAYOUTS)
def test_compaction_moves_rows_between_high_pages(arena, layout):
    ops = _ops()
    c = A.compaction_case()
    assert c.layers > 32 and int(c.nacc.max()) > 16
    r, pm = A.relocate(c, layout, 0, c.layers)
    A.check_map(pm)
    # the long path moves rows between pages of different bands
    bs = c.bs
    base = c.ctxs[0] - c.q_lens[0]
    hops = {(A.loose_band(int(pm.offset[int(c.bt[0, (base + int(p)) // bs])])),
             A.loose_band(int(pm.offset[int(c.bt[0, (base + d) // bs])]))) for d, p in enumerate(c.path[0, :c.nacc[0]])}
    assert any(a != b for a, b in hops), hops
    views = arena.views(pm.geom, layout, c.kcs[0].dtype)
    arena.load(pm, views, c.kcs, c.vcs)
    poison, nbr = pm.poison(), arena.neighbours(pm)
    arena.fill(poison, A.SENTINEL, 1)
    snap = arena.snapshot(nbr)
    td = ops.TreeDrafts([TO.chain(n - 1) for n in c.q_lens], DEV)
    assert td.max_q_len == c.path.shape[1]
    ops.compact_accepted_paths([k for k, _ in views], [v for _, v in views], r.bt.to(DEV),
                               torch.tensor(c.ctxs, dtype=torch.int32, device=DEV), td, torch.from_numpy(c.path).to(DEV),
                               torch.from_numpy(c.nacc).to(DEV))
    torch.cuda.synchronize()
    moved = 0
    for l in range(c.layers):
        for small, view in ((c.kcs[l], views[l][0]), (c.vcs[l], views[l][1])):
            before = _bytes(small).reshape(small.shape[0], bs, -1)
            want = TO.compact(before.copy(), c.bt.numpy(), c.ctxs, c.q_lens, c.path, c.nacc)
            assert np.array_equal(_gather(view, pm), want), (layout, l)
            moved += int((want != before).any(axis=-1).sum())
    assert moved == 2 * c.layers * (19 + 6 + 2)        # destination slots that differ from before, per cache
    assert arena.holds(poison, A.SENTINEL), "a row landed 2^32 or 2^33 bytes below its page"
    assert arena.unchanged(nbr, snap), "a page next to a used slot changed"


@pytest.mark.parametrize("layout", A.LAYOUTS)
def test_round_trip_bulk_write_then_attention_in_high_pages(arena, layout):
    """tests/test_gpu_fp8_codes.py's round trip with the cache in the arena: bf16 K / V through the e4m3 bulk write into
    high pages, then attention on the pages the kernel wrote; the oracle attends to decode(encode(x / scale)) * scale."""
    ops = _ops()
    c = A.round_trip_case()
    scale = C.ROUND_TRIP_SCALE
    keys, values = C.round_trip_source()
    r, pm = A.relocate(c, layout, 0, 1)
    A.check_map(pm)
    (kv, vv), = arena.views(pm.geom, layout, torch.float8_e4m3fn)
    arena.load(pm, [(kv, vv)], c.kcs, c.vcs)
    poison = pm.poison()
    arena.fill(poison, A.NAN_PATTERN[torch.float8_e4m3fn], 1)
    sc = torch.tensor(scale, dtype=torch.float32, device=DEV)
    ops.reshape_and_cache_flash_bulk(C.bf16_tensor(keys).to(DEV), C.bf16_tensor(values).to(DEV), [kv], [vv],
                                     pm.slots_of(c.slots).to(DEV), "fp8_e4m3", [sc], [sc], c.Hkv, C.D)
    torch.cuda.synchronize()
    want_codes = []
    for src, view in ((keys, kv), (values, vv)):
        e = C.encode(C.divide(src, scale), "e4m3fn")
        full = np.zeros((c.nb * c.bs, c.Hkv * C.D), dtype=np.uint8)
        full[c.slots.numpy()] = e.code
        assert not e.nan.any() and np.array_equal(_gather(view, pm).reshape(c.nb * c.bs, -1), full)
        want_codes.append(full.reshape(c.nb, c.bs, c.Hkv, C.D))
    assert arena.holds(poison, A.NAN_PATTERN[torch.float8_e4m3fn])
    qsl = np.concatenate([[0], np.cumsum(c.q_lens)]).astype(np.int32)
    k_ref, v_ref = (torch.from_numpy(C.decode(w, "e4m3fn")).float() for w in want_codes)
    want = O.verify_attention(c.q, k_ref, v_ref, c.bt, c.ctxs, qsl, C.D ** -0.5, scale, scale)
    for host_lens in (False, True):
        out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
        ops.verify_attention(c.q.to(DEV), kv, vv, r.bt.to(DEV), torch.tensor(c.ctxs, dtype=torch.int32, device=DEV),
                             torch.tensor(qsl, device=DEV), max(c.q_lens), max(c.ctxs), C.D ** -0.5, out=out,
                             q_lens_host=c.q_lens if host_lens else None, k_scale=sc.view(1), v_scale=sc.view(1))
        torch.cuda.synchronize()
        got = out.float().cpu()
        worst = float(((got - want).abs() / (ATOL + RTOL * want.abs())).max())
        print(f"round trip {layout}, host lengths {host_lens}: worst err / bar {worst:.3f}")
        assert torch.isfinite(got).all() and worst <= 1
