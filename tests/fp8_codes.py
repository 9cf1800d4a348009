"""OCP fp8 at the level of bits, for the tests that pin every code point of the fp8 paths (bulk KV write, per-tensor
quantisation, the KV8 attention bodies).  numpy / torch on the CPU only; no torch fp8 dtype takes part in `encode` or
`decode` (tensors are viewed as float8 only to hand bytes to a kernel or to the project's oracle).

encode(x, fmt)      f32 -> codes of `e4m3fn` / `e5m2`, written from the OCP definition: round to nearest, ties to even
                    (the subnormal range included); |x| above the largest finite value, +-inf included, saturates to it
                    (+-448 / +-57344); the sign of zero is kept.  NaN is a class, not a code: it comes back as a mask.
decode(code, fmt)   the 256-entry table (f64; every fp8 value is exact in f32, bf16 below 2^8 of mantissa, and f16).
all_bf16 / all_fp16 every 16-bit pattern, as the f32 values they stand for (pattern i at index i).
f32_boundaries      the f32 values at which an encoder decides: every midpoint of two adjacent finite fp8 values and its
                    two f32 neighbours, the neighbourhoods of +-max, of the saturation threshold, of the smallest
                    subnormal and of half of it, +-0, +-inf, f32 subnormals, NaN.

NaN through the writers.  torch's conversion keeps the sign of a NaN (0x7f / 0xff); the bulk KV write
(csrc/kv_bulk_write.hip, f32_to_fp8_sat) returns 0x7f for EVERY NaN, whatever its sign or payload, in both formats
(e4m3fn: the one NaN pattern; e5m2: the all-ones NaN).  tests/test_gpu_fp8_codes.py asserts that rule on the device.

The attention fixtures (v_sweep_case, k_sweep_case, uniform_case, round_trip_source) are described at their builders;
tests/test_fp8_codes_host.py proves on references alone that the two sweeps tell every finite code from its neighbours
by at least ten times the project's attention bar (atol 1e-3 + rtol 2^-8)."""
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

FORMATS = ("e4m3fn", "e5m2")
# mantissa bits, exponent bias, code of the largest finite magnitude
_FMT = {"e4m3fn": (3, 7, 0x7e), "e5m2": (2, 15, 0x7b)}
KV_DTYPE = {"e4m3fn": "fp8_e4m3", "e5m2": "fp8_e5m2"}                   # ops.reshape_and_cache_flash_bulk's names
TORCH_DTYPE = {"e4m3fn": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
ORACLE_KIND = {"e4m3fn": "e4m3", "e5m2": "e5m2"}                        # oracle.spec_oracle.fp8_sat's names
SCALES = (1.0, 0.75, 0.125, 3.1)                                        # the writers' sweep
WRITER_NAN_CODE = 0x7f                                                  # the bulk KV write's code for every NaN
ATOL, RTOL = 1e-3, 2 ** -8                                              # the project's attention bar

Encoded = namedtuple("Encoded", "code nan")       # code uint8 (0 where nan), nan bool


def max_code(fmt):
    return _FMT[fmt][2]


def is_nan_code(code, fmt):
    """The codes a writer may answer a NaN with: magnitude bits above the format's infinity / largest-finite pattern."""
    code = np.asarray(code, dtype=np.uint8)
    return (code & 0x7f) > (0x7e if fmt == "e4m3fn" else 0x7c)


def finite_codes(fmt):
    c = np.arange(256, dtype=np.uint8)
    return c[(c & 0x7f) <= _FMT[fmt][2]]


def encode(x, fmt):
    """f32 array -> Encoded(code, nan), bit by bit (see the module docstring for the rules)."""
    M, bias, top = _FMT[fmt]
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    bits = x.view(np.uint32).astype(np.int64)
    sign = (bits >> 31) << 7
    mag = bits & 0x7fffffff
    nan = mag > 0x7f800000
    ef = np.maximum(mag >> 23, 1)                                   # f32 subnormals share the exponent of 2^-126
    sig = (mag & 0x7fffff) | np.where((mag >> 23) > 0, 1 << 23, 0)   # |x| = sig * 2^(ef - 150)
    emin = 1 - bias
    u = np.maximum(ef - 127, emin)                                  # exponent of the fp8 binade |x| falls in
    shift = np.minimum((u - M) - (ef - 150), 40)                    # |x| = (sig / 2^shift) fp8 quanta of 2^(u - M)
    q = sig >> shift
    rem = sig & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    # normal: q carries the implicit bit 2^M, so the sum lands on (u + bias) << M | fraction, a mantissa carry included;
    # subnormal (u == emin): the exponent field is 0 and q is the code, 2^M being the smallest normal
    code = ((u + bias - 1) << M) + q
    code = np.minimum(code, top)                                    # saturate: codes order like magnitudes
    code = np.where(nan, 0, code | sign)
    return Encoded(code.astype(np.uint8), nan)


def decode_table(fmt):
    """f64 [256]; nan / inf at the codes that are not finite."""
    M, bias, top = _FMT[fmt]
    out = np.zeros(256, dtype=np.float64)
    for c in range(256):
        e, m = (c & 0x7f) >> M, c & ((1 << M) - 1)
        if (c & 0x7f) > top:
            v = math.inf if (fmt == "e5m2" and m == 0) else math.nan
        elif e == 0:
            v = math.ldexp(m, 1 - bias - M)
        else:
            v = math.ldexp((1 << M) + m, e - bias - M)
        out[c] = -v if c & 0x80 else v
    return out


_TABLES = {f: decode_table(f) for f in FORMATS}


def decode(code, fmt):
    return _TABLES[fmt][np.asarray(code, dtype=np.uint8)]


def order_key(code):
    """Signed integer that orders codes like the values they stand for (-0 and +0 compare equal, as the values do)."""
    code = np.asarray(code, dtype=np.int64)
    return np.where(code & 0x80, -(code & 0x7f), code & 0x7f)


# ---- pattern sets ------------------------------------------------------------------------------------------------------
def all_bf16():
    return (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)


def all_fp16():
    return np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)


def bf16_tensor(x_f32):
    """The bf16 torch tensor of f32 values that are bf16 values (their upper 16 bits)."""
    hi = (np.ascontiguousarray(x_f32, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return torch.from_numpy(hi.view(np.int16).copy()).view(torch.bfloat16)


def fp16_tensor(x_f32):
    with np.errstate(over="ignore"):                     # beyond 65504: inf, as meant
        return torch.from_numpy(np.asarray(x_f32, dtype=np.float32).astype(np.float16))


def f32_boundaries(fmt):
    """Sorted finite values, then +-inf, then NaN (both signs, two payloads)."""
    pos = np.sort(decode(finite_codes(fmt), fmt))
    pos = pos[pos >= 0][1:]                              # +0 once (the table has -0 and +0)
    mids = (pos[:-1] + pos[1:]) / 2                      # exact in f64 and in f32 (one more mantissa bit)
    top, tiny = pos[-1], pos[1]
    sat = top + (top - pos[-2]) / 2                      # 464 / 61440: the tie between max and the first code beyond it
    pts = np.concatenate([pos, mids, [sat, tiny / 2, tiny / 4, 3 * tiny / 2, 2 * top, 3.0e38]]).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), np.concatenate([pos, mids, [sat, tiny / 2, tiny / 4, 3 * tiny / 2, 2 * top,
                                                                              np.float32(3.0e38)]]))
    inf = np.float32(np.inf)
    pts = np.concatenate([pts, np.nextafter(pts, inf), np.nextafter(pts, -inf)])
    sub = np.array([1, 2, 0x400000, 0x7fffff, 0x800000], dtype=np.uint32).view(np.float32)   # f32 subnormals, 2^-126
    pts = np.unique(np.concatenate([pts, sub]))
    pts = pts[np.isfinite(pts)]
    finite = np.concatenate([-pts[::-1], pts])
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], dtype=np.uint32).view(np.float32)
    return np.concatenate([finite, [-inf, inf], nans]).astype(np.float32)


def divide(x_f32, scale):
    """x / scale as the bulk KV write forms it: one correctly rounded f32 division."""
    with np.errstate(all="ignore"):
        return np.asarray(x_f32, dtype=np.float32) / np.float32(scale)


# ---- per-tensor quantisation (oracle.spec_oracle.fp8_quant_per_tensor, aic_quantize_fp8_per_tensor) ---------------------
def quant_per_tensor(x_f32):
    """(codes, scale f32): scale = max(amax / 448, 1 / (448 * 512)), code = encode(x * (1 / scale)), all in f32."""
    x = np.asarray(x_f32, dtype=np.float32)
    amax = np.float32(np.abs(x).max())
    scale = np.maximum(amax / np.float32(448.0), np.float32(1.0 / (448.0 * 512.0))).astype(np.float32)
    inv = np.float32(1.0) / scale
    with np.errstate(all="ignore"):
        e = encode(x * inv, "e4m3fn")
    assert not e.nan.any()
    return e.code, scale


def quant_inputs():
    """name -> f32 values that are bf16 values: the inputs of the per-tensor quantiser's sweep."""
    every = all_bf16().copy()
    every[~np.isfinite(every)] = 0.0
    small = every.copy()
    small[np.abs(small) > 448.0] = 0.0
    # an amax whose amax * (1 / (amax / 448)) rounds ABOVE 448 in f32: the clamp, not the division, has to hold the top
    over = None
    for a in every[(every > 1.0) & (every < 1e6)]:
        s = np.float32(a) / np.float32(448.0)
        if np.float32(a) * (np.float32(1.0) / s) > np.float32(448.0):
            over = np.float32(a)
            break
    assert over is not None
    g = np.random.default_rng(5)
    ramp = (over * g.uniform(-1.0, 1.0, 1021)).astype(np.float32)
    ramp = (ramp.view(np.uint32) & 0xffff0000).view(np.float32).copy()           # truncated to bf16 values
    ramp[:4] = [over, -over, 0.0, -0.0]
    return {
        "every-finite-bf16": every,                # amax 3.39e38: nearly everything lands on a subnormal or on zero
        "bf16-up-to-448": small,                   # amax 448, scale 1: every code written from its own value
        "amax-rounds-above-448": ramp,             # 1021 elements: no multiple of 4 either
        "all-zero": np.zeros(4096, dtype=np.float32),      # the scale floor 1 / (448 * 512)
        "length-65533": small[:65533],             # the tail of a 4-element group
        "length-5": np.array([448.0, -0.0, 2.0 ** -9, -2.0 ** -10, 17.0], dtype=np.float32),
    }


# ---- attention: shared geometry ----------------------------------------------------------------------------------------
D, BS = 128, 16
AMP = 40.0                                   # nats at a planted key (tests/attention_fixtures.py)
NAN_CODES = (0x7f, 0xff)                     # e4m3fn; replaced by 0x00 wherever a sweep would place them
SWEEP_HQ, SWEEP_HKV, SWEEP_B, SWEEP_QL = 4, 1, 16, 4        # 16 requests x 4 tokens x 4 heads: one row per code
V_SWEEP_K_SCALE, V_SWEEP_V_SCALE = 0.0037, 64.0             # K as the planted fixtures scale it; V: 2^-9 * 64 = 0.125, 448 * 64 = 28672
K_SWEEP_K_SCALE, K_SWEEP_V_SCALE, K_SWEEP_SM_SCALE = 2.0, 1.0, 0.125
K_SWEEP_GAIN = 2.0                           # a row's score against its key: 2 * (1 + m / 8), in [2, 4)
UNIFORM_K_SCALE, UNIFORM_V_SCALE = 2.0 ** -6, 2.0 ** -6     # uniform codes have rms 105: scores spread ~1.6 nats at sm_scale D^-0.5
ROUND_TRIP_SCALE = 2.0 ** -7                 # 448 / 128 = 3.5: 31 of the source's 3072 magnitudes saturate (1.0 %)


def fp8_tensor(codes):
    return torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn)


def _qsl(q_lens):
    return np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)


def code_of_row():
    """[T, Hq] the code a sweep's row stands for: request i, token t, head h -> 16 i + 4 t + h."""
    T = SWEEP_B * SWEEP_QL
    tok = np.arange(T)[:, None]
    return (tok // SWEEP_QL) * 16 + (tok % SWEEP_QL) * SWEEP_HQ + np.arange(SWEEP_HQ)[None, :]


def _swept(codes):
    codes = np.asarray(codes, dtype=np.uint8).copy()
    codes[np.isin(codes, NAN_CODES)] = 0
    return codes


def v_sweep_case(dtype):
    """Every code through V.  One context of 256 designated keys in 16 shared pages, key j at position j with the planted
    phase-code K of tests/attention_fixtures.py and V = code j in all 128 dimensions (the NaN codes replaced by 0x00);
    every request adds a page of its own with its 4 query tokens (V = 0).  Row (request i, token t, head h) aims 40 nats at
    key 16 i + 4 t + h and returns ~decode(code) * v_scale.  `place[c]`: where code c sits, for `discrimination`."""
    g = torch.Generator().manual_seed(77)
    M = D // 2
    scale = D ** -0.5
    theta = (torch.rand(M, generator=g, dtype=torch.float64) * (1 - 2e-6) + 1e-6) * math.pi
    phase = lambda pos: torch.cat([(pos.double()[..., None] * theta).cos(), (pos.double()[..., None] * theta).sin()], -1)
    ctx = 256 + SWEEP_QL
    n_shared = 256 // BS
    total = n_shared + SWEEP_B + 1
    perm = torch.randperm(total, generator=g)
    bt = torch.zeros(SWEEP_B, n_shared + 1, dtype=torch.int32)
    bt[:, :n_shared] = perm[:n_shared].to(torch.int32)
    bt[:, n_shared] = perm[n_shared:n_shared + SWEEP_B].to(torch.int32)
    k = np.zeros((total, BS, SWEEP_HKV, D), dtype=np.float32)
    v8 = np.zeros((total, BS, SWEEP_HKV, D), dtype=np.uint8)
    vcodes = _swept(np.arange(256))
    pos = torch.arange(256)
    place = {c: ("vc", (int(perm[c // BS]), c % BS)) for c in range(256)}
    k[perm[:n_shared].numpy()] = phase(pos).float().numpy().reshape(n_shared, BS, 1, D)
    v8[perm[:n_shared].numpy()] = np.broadcast_to(vcodes.reshape(n_shared, BS, 1, 1), (n_shared, BS, 1, D))
    own = phase(256 + torch.arange(BS)).float().numpy().reshape(BS, 1, D)          # the stale slots too
    for i in range(SWEEP_B):
        k[int(bt[i, n_shared])] = own
    k8 = encode(k / np.float32(V_SWEEP_K_SCALE), "e4m3fn").code
    target = torch.from_numpy(code_of_row())
    q = ((AMP / (M * scale)) * phase(target)).float().to(dtype)
    q_lens, ctxs = [SWEEP_QL] * SWEEP_B, [ctx] * SWEEP_B
    return SimpleNamespace(q=q, kc=fp8_tensor(k8), vc=fp8_tensor(v8), bt=bt, qsl=_qsl(q_lens), ks=V_SWEEP_K_SCALE,
                           vs=V_SWEEP_V_SCALE, q_lens=q_lens, ctxs=ctxs, Hq=SWEEP_HQ, Hkv=SWEEP_HKV, D=D, bs=BS, window=0,
                           sinks=None, scale=scale, codes=vcodes, place=place)


def k_sweep_dim(c):
    """The dimension code c sits in: 16 consecutive codes (one request) take 16 different ones, the 256 of them every
    residue of the 8-element conversion group and of the dword."""
    return (7 * int(c)) % D


def k_sweep_case(dtype):
    """Every code through K.  Request i holds its own 24 keys: 16 designated ones (key j carries code c = 16 i + j in K's
    dimension k_sweep_dim(c) and zero elsewhere; V = -1 except +1 in that dimension), 4 fillers and its 4 query tokens
    (K = 0, V = -1).  Row (i, t, h) stands for c = 16 i + 4 t + h: q is zero except in c's dimension, where it holds
    sign(c) * GAIN * 2^-e(c) / (sm_scale * k_scale) — a power of two, e(c) the exponent of the code's leading bit (2^-9 for
    the zeros) — so the row scores GAIN * (1 + m / 8) in [2, 4) nats against its key and 0 against the other 20 + t keys
    it sees: out[dim] = tanh((score - ln n) / 2), about 0.5 per nat.  A neighbour code moves the score by GAIN / 8 at least
    (a wrong sign, binade or subnormal by much more)."""
    kcodes = _swept(np.arange(256))
    place = {}
    table = decode(np.arange(256), "e4m3fn")
    pages = 2 * SWEEP_B + 1
    perm = torch.randperm(pages, generator=torch.Generator().manual_seed(78))
    bt = perm[:2 * SWEEP_B].to(torch.int32).view(SWEEP_B, 2)
    k8 = np.zeros((pages, BS, SWEEP_HKV, D), dtype=np.uint8)
    v8 = np.full((pages, BS, SWEEP_HKV, D), 0xb8, dtype=np.uint8)               # -1
    rows = code_of_row()
    q = np.zeros((SWEEP_B * SWEEP_QL, SWEEP_HQ, D), dtype=np.float32)
    for c in range(256):
        i, j, d = c // 16, c % 16, k_sweep_dim(c)
        page = int(bt[i, 0])
        k8[page, j, 0, d] = kcodes[c]
        place[c] = ("kc", (page, j, 0, d))
        v8[page, j, 0, d] = 0x38                                                  # +1
        val = table[kcodes[c]]
        e = math.floor(math.log2(abs(val))) if val != 0 else -9
        w = K_SWEEP_GAIN * 2.0 ** -e / (K_SWEEP_SM_SCALE * K_SWEEP_K_SCALE)
        tok, h = np.argwhere(rows == c)[0]
        q[tok, h, d] = -w if (c & 0x80) else w
    qt = torch.from_numpy(q).to(dtype)
    assert torch.equal(qt.float(), torch.from_numpy(q))                          # powers of two, exact in bf16 and f16
    q_lens, ctxs = [SWEEP_QL] * SWEEP_B, [16 + 4 + SWEEP_QL] * SWEEP_B
    return SimpleNamespace(q=qt, kc=fp8_tensor(k8), vc=fp8_tensor(v8), bt=bt, qsl=_qsl(q_lens), ks=K_SWEEP_K_SCALE,
                           vs=K_SWEEP_V_SCALE, q_lens=q_lens, ctxs=ctxs, Hq=SWEEP_HQ, Hkv=SWEEP_HKV, D=D, bs=BS, window=0,
                           sinks=None, scale=K_SWEEP_SM_SCALE, codes=kcodes, place=place)


def reference(c, dtype=torch.float64):
    """softmax(Q K^T) V of a case in `dtype` through the decode table (no torch fp8 dtype): [T, Hq, D]."""
    table = torch.from_numpy(decode(np.arange(256), "e4m3fn")).to(dtype)
    G = c.Hq // c.Hkv
    out = torch.zeros(int(c.qsl[-1]), c.Hq, c.D, dtype=dtype)
    kb, vb = c.kc.view(torch.uint8).long(), c.vc.view(torch.uint8).long()
    for i, ctx in enumerate(c.ctxs):
        q0, q1 = int(c.qsl[i]), int(c.qsl[i + 1])
        blocks = c.bt[i, :(ctx + c.bs - 1) // c.bs].long()
        K = table[kb[blocks]].reshape(-1, c.Hkv, c.D)[:ctx] * c.ks
        V = table[vb[blocks]].reshape(-1, c.Hkv, c.D)[:ctx] * c.vs
        s = torch.einsum("qhd,khd->hqk", c.q[q0:q1].to(dtype), K.repeat_interleave(G, dim=1)) * c.scale
        pos = torch.arange(q1 - q0).unsqueeze(1) + (ctx - (q1 - q0))
        s = s.masked_fill(~(torch.arange(ctx).unsqueeze(0) <= pos).unsqueeze(0), float("-inf"))
        out[q0:q1] = torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), V.repeat_interleave(G, dim=1))
    return out


def sweep_reference(c, dtype=torch.float64, probs=None):
    """`reference` for a sweep case (every request has the same lengths) in one batched product.  `probs`: the soft-max
    weights of an earlier call on a case with the same q and K (they do not read V).  Returns (out, probs)."""
    table = torch.from_numpy(decode(np.arange(256), "e4m3fn")).to(dtype)
    B, ql, ctx = len(c.ctxs), c.q_lens[0], c.ctxs[0]
    pages = c.bt[:, :(ctx + c.bs - 1) // c.bs].long()
    if probs is None:
        K = table[c.kc.view(torch.uint8).long()[pages]].reshape(B, -1, c.D)[:, :ctx] * c.ks     # Hkv = 1
        s = torch.einsum("bqhd,bkd->bqhk", c.q.to(dtype).view(B, ql, c.Hq, c.D), K) * c.scale
        seen = torch.arange(ctx).view(1, 1, 1, ctx) <= (torch.arange(ql) + ctx - ql).view(1, ql, 1, 1)
        probs = torch.softmax(s.masked_fill(~seen, float("-inf")), dim=-1)
    V = table[c.vc.view(torch.uint8).long()[pages]].reshape(B, -1, c.D)[:, :ctx] * c.vs
    return torch.einsum("bqhk,bkd->bqhd", probs, V).reshape(B * ql, c.Hq, c.D), probs


def neighbours(c):
    """The finite codes next to c on its own side of zero."""
    m = c & 0x7f
    return [c + d for d in (-1, 1) if 0 <= m + d <= 0x7e]


def discrimination(case):
    """For every finite code c and each of its neighbours n: the reference re-derived with c's place in the cache holding
    n instead, and the largest movement of an output element in units of the bar at that element.  {(c, n): ratio}."""
    base, probs = sweep_reference(case)
    bar = ATOL + RTOL * base.abs()
    out = {}
    for c in finite_codes("e4m3fn").tolist():
        name, index = case.place[c]
        cache = getattr(case, name)
        assert (cache.view(torch.uint8)[index] == c).all()
        for n in neighbours(c):
            moved = cache.clone()
            moved.view(torch.uint8)[index] = n
            alt = SimpleNamespace(**{**vars(case), name: moved})
            out[(c, n)] = float(((sweep_reference(alt, probs=probs if name == "vc" else None)[0] - base).abs() / bar).max())
    return out


# ---- attention: uniform codes ------------------------------------------------------------------------------------------
def uniform_case(q_lens, ctxs, Hq, Hkv, bs, seed, dtype):
    """K and V bytes drawn uniformly over the 254 finite e4m3 codes (every page, the slots past a context too), random q.
    The namespace has the fields tests/attention_fixtures.oracle and the prefix fixtures' share_* functions read."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    nblk = [(c + bs - 1) // bs for c in ctxs]
    total = sum(nblk) + 3
    perm = torch.randperm(total, generator=g)
    bt = torch.zeros(len(ctxs), max(nblk), dtype=torch.int32)
    k = 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[k:k + n].to(torch.int32)
        k += n
    finite = finite_codes("e4m3fn")
    k8 = finite[rng.integers(0, finite.size, (total, bs, Hkv, D))]
    v8 = finite[rng.integers(0, finite.size, (total, bs, Hkv, D))]
    q = torch.randn(int(sum(q_lens)), Hq, D, generator=g).to(dtype)
    return SimpleNamespace(q=q, kc=fp8_tensor(k8), vc=fp8_tensor(v8), bt=bt, qsl=_qsl(q_lens), ks=UNIFORM_K_SCALE,
                           vs=UNIFORM_V_SCALE, q_lens=list(q_lens), ctxs=list(ctxs), Hq=Hq, Hkv=Hkv, D=D, bs=bs, window=0,
                           sinks=None, scale=D ** -0.5)


def score_spread(c):
    """Standard deviation, in nats, of the visible scores of a uniform case (request 0, every head)."""
    table = torch.from_numpy(decode(np.arange(256), "e4m3fn"))
    ctx, ql = c.ctxs[0], c.q_lens[0]
    K = table[c.kc.view(torch.uint8).long()[c.bt[0, :(ctx + c.bs - 1) // c.bs].long()]].reshape(-1, c.Hkv, c.D)[:ctx] * c.ks
    s = torch.einsum("qhd,khd->hqk", c.q[:ql].double(), K.repeat_interleave(c.Hq // c.Hkv, dim=1)) * c.scale
    return float(s[..., :ctx - ql].std())


# ---- attention: round trip through the bulk write ----------------------------------------------------------------------
ROUND_TRIP = dict(q_lens=[4, 9], ctxs=[64, 32], Hq=8, Hkv=2)


def round_trip_source(seed=3):
    """(keys, values) bf16 [96, Hkv * D]: every bf16 pattern with 2^-22 <= |x| < 4 (24 binades x 128 mantissas x 2 signs =
    6144 patterns, 4 times each), shuffled — log-uniform magnitudes.  At ROUND_TRIP_SCALE the quotients span the e4m3
    range from below its smallest subnormal to past 448: zeros, subnormals, every binade and saturation all occur."""
    pats = all_bf16()
    a = np.abs(pats)
    pats = pats[np.isfinite(pats) & (a >= 2.0 ** -22) & (a < 4.0)]
    assert pats.size == 6144
    rng = np.random.default_rng(seed)
    T = sum(ROUND_TRIP["ctxs"])
    n = ROUND_TRIP["Hkv"] * D
    keys = rng.permutation(np.tile(pats, T * n // pats.size)).reshape(T, n)
    values = rng.permutation(np.tile(pats, T * n // pats.size)).reshape(T, n)
    return keys, values
