"""GPU: the fp8 paths at every code point (tests/fp8_codes.py has the bit-level encoder / decoder, the pattern sets and
the fixtures; tests/test_fp8_codes_host.py proves them on the CPU).

  writers   the bulk KV write on all 65 536 bf16 patterns, all 65 536 fp16 patterns and the f32 decision boundaries of the
            format, for e4m3 and e5m2 caches, four scales, the 16-byte and the scalar path: byte-equal to
            encode(f32(src) / scale) wherever the quotient is a number, a NaN code where it is not — and exactly 0x7f, the
            sign dropped, which is the kernel's rule (fp8_codes' docstring);
            aic_quantize_fp8_per_tensor on every finite bf16 pattern (amax 3.39e38: subnormals and zeros), the patterns up
            to 448 (every code), an amax whose product with the inverse scale rounds above 448, zeros (the scale floor) and
            lengths that are no multiple of 4: scale and bytes equal to the oracle's;
  readers   every finite e4m3 code through V and through K of ops.verify_attention (two sweeps of 256 rows, bf16 and fp16
            queries, with and without host-known query lengths), caches of uniformly drawn codes through every other KV8
            body, and a round trip bulk write -> attention; all at the project's bar, atol 1e-3 + rtol 2^-8 against the
            fp32 oracle, every output pre-filled with NaN."""
import numpy as np
import pytest
import torch

import attention_fixtures as F
import fp8_codes as C
import prefix_group_fixtures as PG
import shared_prefix_fixtures as S
import tree_oracle as TO
from oracle import spec_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = C.ATOL, C.RTOL


def _ops():
    from arcticinference_amd import ops
    return ops


# ---- the bulk KV write -------------------------------------------------------------------------------------------------
def _source(src, fmt):
    """(f32 values, to a torch tensor of the source dtype)"""
    if src == "bf16":
        return C.all_bf16(), C.bf16_tensor
    if src == "fp16":
        return C.all_fp16(), C.fp16_tensor
    return C.f32_boundaries(fmt), lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))


def _bulk_write(k_src, v_src, to_tensor, fmt, scales, H, Dh, seed=0):
    """Writes the patterns (one per element, padded with zeros to whole rows of H * Dh) through the op behind a shuffled
    slot mapping.  Returns per cache (K, V): (written bytes [slots, n], source values [T, n], the slot of every token)."""
    n, bs = H * Dh, 16
    T = -(-k_src.size // n)
    pad = lambda x: np.concatenate([x, np.zeros(T * n - x.size, dtype=np.float32)]).reshape(T, n)
    k_src, v_src = pad(k_src), pad(v_src)
    nb = -(-T // bs) + 2
    slots = torch.randperm(nb * bs, generator=torch.Generator().manual_seed(seed))[:T].to(torch.int64)
    kc = torch.zeros(nb, bs, H, Dh, dtype=torch.uint8, device=DEV).view(C.TORCH_DTYPE[fmt])
    vc = torch.zeros(nb, bs, H, Dh, dtype=torch.uint8, device=DEV).view(C.TORCH_DTYPE[fmt])
    sc = [torch.tensor(s, dtype=torch.float32, device=DEV) for s in scales]
    _ops().reshape_and_cache_flash_bulk(to_tensor(k_src).to(DEV), to_tensor(v_src).to(DEV), [kc], [vc], slots.to(DEV),
                                        C.KV_DTYPE[fmt], [sc[0]], [sc[1]], H, Dh)
    torch.cuda.synchronize()
    flat = lambda c: c.view(torch.uint8).cpu().numpy().reshape(nb * bs, n)
    return (flat(kc), k_src), (flat(vc), v_src), slots.numpy()


@pytest.mark.parametrize("path", ["16-byte", "scalar"])
@pytest.mark.parametrize("scales", [(1.0, 0.75), (0.125, 3.1)], ids=["k1-v0.75", "k0.125-v3.1"])
@pytest.mark.parametrize("src", ["bf16", "fp16", "f32-boundaries"])
@pytest.mark.parametrize("fmt", C.FORMATS)
def test_bulk_write_every_pattern(fmt, src, scales, path):
    x, to_tensor = _source(src, fmt)
    if path == "16-byte":
        H, Dh = (2, 64) if src == "f32-boundaries" else (8, 128)
    else:
        H, Dh = (3, 7) if src == "f32-boundaries" else (3, 20)       # rows of 84 / 120 bytes: no multiple of 16
    assert ((H * Dh * (4 if src == "f32-boundaries" else 2)) % 16 == 0) == (path == "16-byte")
    (kb, ks), (vb, vs), slots = _bulk_write(x, x[::-1].copy(), to_tensor, fmt, scales, H, Dh)
    compared = 0
    for got, source, scale, name in ((kb, ks, scales[0], "K"), (vb, vs, scales[1], "V")):
        quo = C.divide(source, scale)
        want = C.encode(quo, fmt)
        full = np.zeros_like(got)
        full[slots] = want.code
        nan = np.zeros(got.shape, dtype=bool)
        nan[slots] = want.nan
        bad = (got != full) & ~nan
        assert not bad.any(), (name, [(f"{float(source.reshape(-1)[i]):.9g}", hex(want.code.reshape(-1)[i]))
                                      for i in np.flatnonzero(bad[slots])[:8]], hex(int(got[bad][0])))
        assert C.is_nan_code(got[nan], fmt).all() and (got[nan] == C.WRITER_NAN_CODE).all(), name
        assert np.array_equal(want.nan, np.isnan(quo))
        compared += source.size
    print(f"bulk write {fmt} {src} {path}: {compared} elements compared, none skipped")
    assert compared >= 2 * x.size


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_bulk_write_answers_every_nan_with_0x7f(fmt):
    """The sign rule of the kernel (f32_to_fp8_sat): one code for every NaN, whatever its sign, payload or source type —
    where torch's conversion keeps the sign.  +-inf is no NaN: it saturates."""
    bits = np.array([0x7fc00000, 0xffc00000, 0x7f810000, 0xff810000, 0x7fffffff, 0xffffffff, 0x7fc10000, 0xffa00000],
                    dtype=np.uint32)                 # payloads in the upper mantissa bits: NaN in bf16 and fp16 too
    x = np.concatenate([bits.view(np.float32), np.float32([np.inf, -np.inf, 1.0, -1.0, 0.0, -0.0, 1e30, -1e30])])
    top = C.max_code(fmt)
    for to_tensor in (lambda v: torch.from_numpy(v.copy()), C.bf16_tensor, C.fp16_tensor):
        (kb, _), (vb, _), slots = _bulk_write(x, x, to_tensor, fmt, (0.75, 3.1), 1, 16)
        for got in (kb[slots].reshape(-1), vb[slots].reshape(-1)):
            assert (got[:8] == 0x7f).all(), [hex(b) for b in got[:8]]
            assert got[8:10].tolist() == [top, top | 0x80] and got[14:16].tolist() == [top, top | 0x80]
            assert got[12:14].tolist() == [0x00, 0x80]


# ---- per-tensor quantisation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.quant_inputs()))
def test_quantize_per_tensor_on_the_code_points(name):
    x = C.quant_inputs()[name]
    xt = C.bf16_tensor(x)
    q_ref, s_ref = O.fp8_quant_per_tensor(xt)
    codes, scale = C.quant_per_tensor(x)
    q, s = _ops().quantize_fp8_per_tensor(xt.to(DEV))
    got = q.cpu().view(torch.uint8).numpy()
    print(f"quantize {name}: {got.size} elements compared, scale {float(s):.9g}")
    assert float(s.cpu()) == float(s_ref) == float(scale)
    bad = np.flatnonzero(got != q_ref.view(torch.uint8).numpy())
    assert bad.size == 0, [(f"{float(x[i]):.9g}", hex(got[i]), hex(codes[i])) for i in bad[:8]]
    assert np.array_equal(got, codes)


# ---- attention ---------------------------------------------------------------------------------------------------------
def _dev(c):
    args = (c.q.to(DEV), c.kc.to(DEV), c.vc.to(DEV), c.bt.to(DEV), torch.tensor(c.ctxs, dtype=torch.int32, device=DEV),
            torch.tensor(c.qsl, device=DEV))
    kw = dict(k_scale=torch.tensor([c.ks], dtype=torch.float32, device=DEV),
              v_scale=torch.tensor([c.vs], dtype=torch.float32, device=DEV))
    return args, kw


def _verify(c, host_lens=True, **extra):
    args, kw = _dev(c)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    _ops().verify_attention(*args, max(c.q_lens), max(c.ctxs), c.scale, out=out,
                            q_lens_host=c.q_lens if host_lens else None, **kw, **extra)
    torch.cuda.synchronize()
    return out.float().cpu()


def _close(got, want, what):
    err = (got - want).abs()
    worst = err / (ATOL + RTOL * want.abs())
    print(f"{what}: max abs err {float(err.max()):.4g}, worst err / bar {float(worst.max()):.3f}")
    assert torch.isfinite(got).all(), f"{what}: non-finite output (a row was not written)"
    return worst


@pytest.mark.parametrize("host_lens", [False, True], ids=["plain", "q_lens_host"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("sweep", ["v", "k"])
def test_every_code_through_attention(sweep, dtype, host_lens):
    """256 rows, one per code (the two NaN codes stand in as 0x00): tests/test_fp8_codes_host.py shows that a code read as
    its neighbour moves its row by >= 14 (V) / 15 (K) times the bar."""
    c = (C.v_sweep_case if sweep == "v" else C.k_sweep_case)(dtype)
    want = F.oracle(c)
    worst = _close(_verify(c, host_lens), want, f"{sweep} sweep")
    rows = C.code_of_row()
    bad = (worst > 1).any(-1).numpy()
    assert not bad.any(), f"{sweep} sweep: the rows of codes {[hex(x) for x in sorted(set(rows[bad].tolist()))]} miss the bar"
    assert rows.size == 256 and sorted(rows.reshape(-1).tolist()) == list(range(256))


def _attend(c, call):
    args, kw = _dev(c)
    out = torch.full(c.q.shape, float("nan"), dtype=c.q.dtype, device=DEV)
    call(args, kw, out)
    torch.cuda.synchronize()
    return out.float().cpu()


def _body_case(body, dtype):
    """(case, run, oracle): the smallest shapes that reach each of the other KV8 bodies, as their own tests define them."""
    ops = _ops()
    if body == "long-draft":                 # 33 query tokens x G 4 = 132 rows, lengths known on the host
        c = C.uniform_case([33], [200], 8, 2, 16, seed=1, dtype=dtype)
        return c, lambda: _verify(c), lambda: F.oracle(c)
    if body == "mixed":                      # short and long requests in one call (16 / 132 / 8 / 36 rows)
        c = C.uniform_case([4, 33, 2, 9], [130, 200, 64, 97], 8, 2, 16, seed=2, dtype=dtype)
        return c, lambda: _verify(c), lambda: F.oracle(c)
    if body == "shared-prefix":              # one shared prefix of 32 tokens, request 0 right behind it
        q_lens, P = [1, 9, 3], 32
        ctxs = [P + e + q for q, e in zip(q_lens, [0, 20, 66])]
        c = S.share_prefix(C.uniform_case(q_lens, ctxs, 16, 4, 16, seed=3, dtype=dtype), P)
        return c, lambda: _verify(c, shared_prefix_len=P, prefix_block_table=c.prefix_table.to(DEV),
                                  seq_lens_host=c.ctxs), lambda: F.oracle(c)
    if body == "prefix-groups":              # two groups and a request in none, pages of 32
        q_lens, req_group, group_len = [1, 4, 2, 3, 9, 1], [0, 1, -1, 0, 1, 0], [64, 96]
        ctxs = [(group_len[g] if g >= 0 else 0) + e + q for q, e, g in zip(q_lens, [0, 5, 18, 40, 0, 70], req_group)]
        c = PG.share_in_groups(C.uniform_case(q_lens, ctxs, 16, 4, 32, seed=4, dtype=dtype), req_group, group_len)
        return c, lambda: _verify(c, prefix_groups=ops.PrefixGroups(req_group, group_len, q_lens, torch.device(DEV)),
                                  seq_lens_host=c.ctxs), lambda: F.oracle(c)
    if body == "tree":                       # tree-shaped drafts: a 33-token tree and a small one
        from arcticinference_amd import tree_drafts as TD
        trees = [TO.random_tree(32, np.random.default_rng(14), 0.6), TO.random_tree(6, np.random.default_rng(15), 0.8)]
        lay = TD.build_tree_layout(trees)
        c = C.uniform_case([int(x) for x in lay.q_lens], [200, 95], 8, 2, 16, seed=5, dtype=dtype)
        run = lambda: _attend(c, lambda args, kw, out: ops.verify_attention_tree(
            *args[:5], ops.TreeDrafts(trees, DEV), max(c.ctxs), c.scale, out=out, **kw))
        return c, run, lambda: TO.tree_attention(c.q, c.kc, c.vc, c.bt, c.ctxs, lay.query_start_loc, lay.masks, c.scale,
                                                 k_scale=c.ks, v_scale=c.vs)
    assert body == "step-with-a-prefill-chunk"       # a prefill chunk of 40 tokens beside a decode
    c = C.uniform_case([40, 3], [100, 64], 8, 2, 16, seed=6, dtype=dtype)
    run = lambda: _attend(c, lambda args, kw, out: ops.step_attention(*args, max(c.ctxs), c.scale, q_lens_host=c.q_lens,
                                                                      out=out, **kw))
    return c, run, lambda: F.oracle(c)


_BODIES = ["long-draft", "mixed", "shared-prefix", "prefix-groups", "tree", "step-with-a-prefill-chunk"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("body", _BODIES)
def test_uniform_codes_through_every_other_body(body, dtype):
    """K and V bytes uniform over the 254 finite codes: subnormals and the top binade in every tile.  k_scale = v_scale =
    2^-6 (fp8_codes.UNIFORM_K_SCALE): the codes' rms is 105, so the scores spread ~1.6 nats at sm_scale D^-0.5
    (tests/test_fp8_codes_host.py measures it)."""
    c, run, oracle = _body_case(body, dtype)
    assert (c.ks, c.vs) == (2.0 ** -6, 2.0 ** -6)
    want = oracle()
    worst = _close(run(), want, body)
    assert float(worst.max()) <= 1, f"{body}: {int((worst > 1).sum())} elements miss the bar"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_round_trip_bulk_write_then_attention(dtype):
    """bf16 K / V of log-uniform magnitude through the bulk write at a scale at which 1 % of them saturate (and a fifth
    fall below the smallest subnormal), then attention on the cache the kernel wrote; the oracle attends to
    decode(encode(x / scale)) * scale."""
    R, scale = C.ROUND_TRIP, C.ROUND_TRIP_SCALE
    keys, values = C.round_trip_source()
    bs, Hkv, Hq = 16, R["Hkv"], R["Hq"]
    g = torch.Generator().manual_seed(9)
    nblk = [c // bs for c in R["ctxs"]]
    perm = torch.randperm(sum(nblk) + 2, generator=g)
    bt = torch.zeros(len(nblk), max(nblk), dtype=torch.int32)
    slots, k = [], 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[k:k + n].to(torch.int32)
        slots += [int(bt[i, t // bs]) * bs + t % bs for t in range(R["ctxs"][i])]
        k += n
    slots = torch.tensor(slots, dtype=torch.int64)
    nb = sum(nblk) + 2
    kc = torch.zeros(nb, bs, Hkv, C.D, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    vc = torch.zeros(nb, bs, Hkv, C.D, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    sc = torch.tensor(scale, dtype=torch.float32, device=DEV)
    _ops().reshape_and_cache_flash_bulk(C.bf16_tensor(keys).to(DEV), C.bf16_tensor(values).to(DEV), [kc], [vc],
                                        slots.to(DEV), "fp8_e4m3", [sc], [sc], Hkv, C.D)
    want_codes = []
    for src, cache in ((keys, kc), (values, vc)):
        e = C.encode(C.divide(src, scale), "e4m3fn")
        full = np.zeros((nb * bs, Hkv * C.D), dtype=np.uint8)
        full[slots.numpy()] = e.code
        assert not e.nan.any() and np.array_equal(cache.view(torch.uint8).cpu().numpy().reshape(nb * bs, -1), full)
        want_codes.append(full.reshape(nb, bs, Hkv, C.D))
    q = torch.randn(sum(R["q_lens"]), Hq, C.D, generator=g).to(dtype)
    qsl = np.concatenate([[0], np.cumsum(R["q_lens"])]).astype(np.int32)
    k_ref, v_ref = (torch.from_numpy(C.decode(w, "e4m3fn")).float() for w in want_codes)
    want = O.verify_attention(q, k_ref, v_ref, bt, R["ctxs"], qsl, C.D ** -0.5, scale, scale)
    for host_lens in (False, True):
        out = torch.full(q.shape, float("nan"), dtype=dtype, device=DEV)
        _ops().verify_attention(q.to(DEV), kc, vc, bt.to(DEV), torch.tensor(R["ctxs"], dtype=torch.int32, device=DEV),
                                torch.tensor(qsl, device=DEV), max(R["q_lens"]), max(R["ctxs"]), C.D ** -0.5, out=out,
                                q_lens_host=R["q_lens"] if host_lens else None, k_scale=sc.view(1), v_scale=sc.view(1))
        torch.cuda.synchronize()
        worst = _close(out.float().cpu(), want, f"round trip, host lengths {host_lens}")
        assert float(worst.max()) <= 1
