"""Planted-key attention fixtures: data on which ONE key carries a row's whole weight, so that a mask edge that is off by
one key moves the output by order 1 instead of by ~1/ctx (random Q / K / V put a single-key fault on the tolerance).

Relative-position phase code.  With M = D / 2 frequencies theta_m drawn uniformly in (0, pi) per kv head, key j is
[cos(j theta_m), sin(j theta_m)] and a query that AIMS at key t is A / (M sm_scale) [cos(t theta_m), sin(t theta_m)]:
its score against key j is A mean_m cos(theta_m (j - t)), A at j = t and a random sidelobe (sigma ~ A / sqrt(D))
elsewhere.  A = 40 nats keeps every score bounded (fp32 arithmetic is a fair reference) and leaves the target
>= 0.999 of a row's weight when it is visible.  V is randn, different per kv head: the output names the key attended.

The aim of a query token at absolute position p (window W), one of
  edge    t = p          must be seen: the output is ~V[p]
  past    t = p + 1      must not be seen; for the last token t = seq_len, planted in the stale slot after the last
                         token (the last page's free slot, or the spare page every padded block-table column names)
  win_lo  t = p - W + 1  must be seen      (windowed layers only)
  below   t = p - W      must not be seen  (windowed layers only)
  far     a random visible key: page and tile attribution in the middle of the range
The G query heads of a kv head take different aims for the same token, rotating with the token index (the kernels pack
row = token * G + head); a target that does not exist (t < 0) falls back to `edge`.

Also here: a float64 restatement of the oracle with movable mask edges (the mutated references of
tests/test_attention_fixtures_host.py), and the structured-score profiles of the lazy-maximum tests."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import spec_oracle as O

KINDS = ("edge", "past", "win_lo", "below", "far")
EDGE, PAST, WIN_LO, BELOW, FAR = range(5)
SEEN = (EDGE, WIN_LO, FAR)
AMP = 40.0                     # nats at the target
K_SCALE, V_SCALE = 0.0037, 0.021   # fp8 cache: |K| <= 1 -> |K / k_scale| <= 271 < 448 (e4m3); V as the other tests scale it
PF_SLACK_NATS = 6.0 * math.log(2.0)   # kPfSlack (csrc/prefill_attn.hip) and the verify bodies' slack: 2^6


def _phase(pos, theta):
    """pos int64 [...], theta f64 [..., M] (broadcast against pos[..., None]) -> f64 [..., 2 M]"""
    ang = pos.double().unsqueeze(-1) * theta
    return torch.cat([ang.cos(), ang.sin()], dim=-1)


def planted_case(q_lens, ctxs, Hq, Hkv, D, bs, seed, window=0, fp8=False, sinks=None, plant_below=False, amp=AMP):
    """A step of len(q_lens) requests.  Returns a namespace: q [T, Hq, D] bf16; kc / vc paged caches (bf16, or e4m3 codes
    of x / scale) behind a shuffled block table `bt` whose padded columns name a planted spare page; qsl; ks / vs (None
    for bf16); kind / target [T, Hq] (the aim of every row); stale [B] (position seq_len physically holds its planted
    key); and the arguments.  `plant_below` (windowed): every page wholly below the first row's `below` target holds keys
    the first token's rows aim at."""
    g = torch.Generator().manual_seed(seed)
    M, G, B = D // 2, Hq // Hkv, len(q_lens)
    W = int(window or 0)
    scale = D ** -0.5
    theta = (torch.rand(Hkv, M, generator=g, dtype=torch.float64) * (1 - 2e-6) + 1e-6) * math.pi
    nblk = [(c + bs - 1) // bs for c in ctxs]
    total = sum(nblk) + 3
    perm = torch.randperm(total, generator=g)
    spare = int(perm[sum(nblk)])
    bt = torch.full((B, max(nblk) + 1), spare, dtype=torch.int32)
    # unowned slots: keys of unrelated positions (never a target), V like everything else
    kc = _phase(torch.randint(20000, 30000, (total, bs, 1), generator=g), theta).float()
    vc = torch.randn(total, bs, Hkv, D, generator=g)
    # the spare page serves the last request whose context ends on a page border (else request 0): its key seq_len
    owner = max([i for i, c in enumerate(ctxs) if c % bs == 0], default=0)
    kc[spare] = _phase(torch.tensor([[ctxs[owner]]]), theta).float()
    stale = [c % bs != 0 or i == owner for i, c in enumerate(ctxs)]
    k = 0
    for i, n in enumerate(nblk):
        pages = perm[k:k + n]
        k += n
        bt[i, :n] = pages.to(torch.int32)
        pos = torch.arange(n * bs)                       # every slot of the last page: the stale ones too
        keys = _phase(pos.unsqueeze(-1), theta)          # [n bs, Hkv, D]
        if plant_below and W:
            ctx0 = ctxs[i] - q_lens[i]
            cut = max(0, (ctx0 - W) // bs * bs)          # pages wholly below the first token's `below` target
            cand = [t for t in (ctx0, ctx0 - W + 1, ctx0 + 1) if t >= 0]
            if cut:
                lure = torch.tensor([cand[j % len(cand)] for j in range(cut)])
                keys[:cut] = _phase(lure.unsqueeze(-1), theta)
        kc[pages.long()] = keys.float().view(n, bs, Hkv, D)
    # ---- aims --------------------------------------------------------------------------------------------------------
    kinds = (EDGE, PAST, WIN_LO, BELOW, FAR) if W else (EDGE, PAST, FAR)
    T = int(sum(q_lens))
    kind = torch.zeros(T, Hq, dtype=torch.int64)
    target = torch.zeros(T, Hq, dtype=torch.int64)
    gq = (torch.arange(Hq) % G).unsqueeze(0)
    r0 = 0
    for i, (ql, ctx) in enumerate(zip(q_lens, ctxs)):
        n = torch.arange(ql).unsqueeze(1)
        p = (ctx - ql) + n.expand(ql, Hq)
        kd = torch.tensor(kinds)[(n + gq + seed + i) % len(kinds)]
        lo = (p - W + 1).clamp(min=0) if W else torch.zeros_like(p)
        far = lo + (torch.rand(ql, Hq, generator=g, dtype=torch.float64) * (p - lo + 1).double()).long().clamp(max=p - lo)
        t = torch.where(kd == EDGE, p, torch.where(kd == PAST, p + 1, torch.where(kd == WIN_LO, p - W + 1,
                        torch.where(kd == BELOW, p - W, far))))
        kd = torch.where(t < 0, torch.full_like(kd, EDGE), kd)
        t = torch.where(t < 0, p, t)
        kind[r0:r0 + ql], target[r0:r0 + ql] = kd, t
        r0 += ql
    head_theta = theta[torch.arange(Hq) // G]            # [Hq, M]
    q = (amp / (M * scale)) * _phase(target, head_theta.unsqueeze(0))
    q = q.float().to(torch.bfloat16)
    ks = vs = None
    if fp8:
        ks, vs = K_SCALE, V_SCALE
        kc, vc = O.fp8_sat(kc / ks, "e4m3"), O.fp8_sat(vc / vs, "e4m3")
    else:
        kc, vc = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    return SimpleNamespace(q=q, kc=kc, vc=vc, bt=bt, qsl=qsl, ks=ks, vs=vs, kind=kind, target=target, stale=stale,
                           q_lens=list(q_lens), ctxs=list(ctxs), Hq=Hq, Hkv=Hkv, D=D, bs=bs, window=W, sinks=sinks,
                           scale=scale)


def take_heads(c, h):
    """The case restricted to kv head h (its query heads, K / V, sinks and aims): keeps the references small."""
    G = c.Hq // c.Hkv
    sl = slice(h * G, (h + 1) * G)
    d = dict(vars(c))
    d.update(q=c.q[:, sl].contiguous(), kc=c.kc[:, :, h:h + 1].contiguous(), vc=c.vc[:, :, h:h + 1].contiguous(),
             kind=c.kind[:, sl], target=c.target[:, sl], Hq=G, Hkv=1,
             sinks=None if c.sinks is None else c.sinks[sl].contiguous())
    return SimpleNamespace(**d)


def oracle(c):
    """The project's fp32 oracle on the case's own (quantised) tensors."""
    sc = dict(k_scale=c.ks, v_scale=c.vs) if c.ks is not None else {}
    return O.verify_attention(c.q, c.kc, c.vc, c.bt, c.ctxs, c.qsl, c.scale, sliding_window=c.window, sinks=c.sinks, **sc)


def reference(c, dtype=torch.float64, causal=0, win_lo=0):
    """Restatement of the oracle in `dtype` with movable mask edges: position p sees keys
    p - W + 1 + win_lo .. p + causal (causal = win_lo = 0: the oracle's attention).  causal = +1 reads position seq_len
    through the block table, as a kernel with that fault would.  Returns (out [T, Hq, D], the weight of every row's
    target [T, Hq], 0 where the target is not among the keys read).  A row that sees nothing gives zeros."""
    Hq, Hkv, D, bs, W = c.Hq, c.Hkv, c.D, c.bs, c.window
    G = Hq // Hkv
    T = int(c.qsl[-1])
    out = torch.zeros(T, Hq, D, dtype=dtype)
    wt = torch.zeros(T, Hq, dtype=dtype)
    ks, vs = (c.ks, c.vs) if c.ks is not None else (1.0, 1.0)
    for i, ctx in enumerate(c.ctxs):
        q0, q1 = int(c.qsl[i]), int(c.qsl[i + 1])
        ql = q1 - q0
        if ql == 0:
            continue
        nk = ctx + max(causal, 0)
        blocks = c.bt[i, :(nk + bs - 1) // bs].long()
        K = c.kc[blocks].reshape(-1, Hkv, D)[:nk].to(dtype) * ks
        V = c.vc[blocks].reshape(-1, Hkv, D)[:nk].to(dtype) * vs
        Q = c.q[q0:q1].to(dtype)
        s = torch.einsum("qhd,khd->hqk", Q, K.repeat_interleave(G, dim=1)) * c.scale
        pos = torch.arange(ql).unsqueeze(1) + (ctx - ql)
        key = torch.arange(nk).unsqueeze(0)
        mask = key <= pos + causal
        if W:
            mask = mask & (key > pos - W + win_lo)
        s = s.masked_fill(~mask.unsqueeze(0), float("-inf"))
        if c.sinks is not None:
            s = torch.cat([s, c.sinks.to(dtype).view(Hq, 1, 1).expand(Hq, ql, 1)], dim=-1)
        p = torch.softmax(s, dim=-1)[..., :nk]
        p = torch.nan_to_num(p, nan=0.0)                 # a row with nothing visible (and no sink)
        out[q0:q1] = torch.einsum("hqk,khd->qhd", p, V.repeat_interleave(G, dim=1))
        tg = c.target[q0:q1].t()                         # [Hq, ql]
        ok = tg < nk
        wt[q0:q1] = (p.gather(2, tg.clamp(max=nk - 1).unsqueeze(-1)).squeeze(-1) * ok).t()
    return out, wt


def rows_of(c, kinds):
    """[T, Hq] bool: the rows whose aim is one of `kinds`."""
    m = torch.zeros_like(c.kind, dtype=torch.bool)
    for k in kinds:
        m |= c.kind == k
    return m


def last_rows_without_stale_slot(c):
    """[T, Hq] bool: the last query token of every request whose position seq_len holds no planted key."""
    m = torch.zeros_like(c.kind, dtype=torch.bool)
    for i, ok in enumerate(c.stale):
        if not ok and c.qsl[i + 1] > c.qsl[i]:
            m[int(c.qsl[i + 1]) - 1] = True
    return m


def describe(c, got, want, atol, rtol, limit=12):
    """The failing rows by aim and place: request, token, query head, row of the request (token * G + head of the group:
    row % 128, % 32 and % 16 name the workgroup block, the wave and the MFMA tile), position, aim kind and target."""
    G = c.Hq // c.Hkv
    err = (got - want).abs()
    bad = (err > atol + rtol * want.abs()).any(dim=-1)
    if not bad.any():
        return "ok"
    lines = [f"{int(bad.sum())} of {bad.numel()} rows fail, max abs err {float(err.max()):.4g}; by aim: " +
             ", ".join(f"{KINDS[k]} {int((bad & (c.kind == k)).sum())}/{int((c.kind == k).sum())}" for k in range(5))]
    req = np.searchsorted(c.qsl, np.arange(int(c.qsl[-1])), side="right") - 1
    for tok, hq in bad.nonzero()[:limit].tolist():
        i = int(req[tok])
        n = tok - int(c.qsl[i])
        p = c.ctxs[i] - c.q_lens[i] + n
        lines.append(f"  req {i} (q_len {c.q_lens[i]}, ctx {c.ctxs[i]}) token {n} head {hq} row {n * G + hq % G} pos {p} "
                     f"aim {KINDS[int(c.kind[tok, hq])]} -> key {int(c.target[tok, hq])}: err {float(err[tok, hq].max()):.4g}")
    return "\n".join(lines)


# ---- structured scores: the lazy running maximum ---------------------------------------------------------------------
PROFILES = ("rising", "falling", "spikes", "plateaus")


def structured_case(profile, q_lens, ctxs, Hq, Hkv, D, bs, seed, fp8=False, window=0, sinks=None):
    """Keys = a common direction u times a per-position profile (+ a little noise), queries ~ sqrt(D) u: score(j) ~
    profile(j) nats, within [-40, 40].  rising / falling: 36 nats over the longest context (the noise adds up to ~5 %); spikes: isolated keys 30 nats
    above a flat floor; plateaus: 20 steps of 0.41 of the slack each (2^6: two steps stay below it, the third crosses it).
    V is randn.  Same namespace as planted_case (no aims)."""
    g = torch.Generator().manual_seed(seed)
    B = len(q_lens)
    nblk = [(c + bs - 1) // bs for c in ctxs]
    total = sum(nblk) + 3
    perm = torch.randperm(total, generator=g)
    bt = torch.zeros(B, max(nblk), dtype=torch.int32)
    tok = torch.zeros(total, bs)
    k = 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[k:k + n].to(torch.int32)
        tok[perm[k:k + n].long()] = torch.arange(n * bs).float().view(n, bs)
        k += n
    t = tok / float(max(ctxs))
    if profile == "rising":
        prof = 36.0 * t
    elif profile == "falling":
        prof = -36.0 * t
    elif profile == "spikes":
        prof = torch.where(torch.rand(total, bs, generator=g) < 0.01, torch.full((total, bs), 30.0), torch.zeros(total, bs))
    else:
        prof = torch.floor(t * 20.0).clamp(max=19.0) * (0.41 * PF_SLACK_NATS)
    u = torch.randn(D, generator=g)
    u = u / u.norm()
    kc = prof[..., None, None] * u + 0.05 * torch.randn(total, bs, Hkv, D, generator=g)
    vc = torch.randn(total, bs, Hkv, D, generator=g)
    T = int(sum(q_lens))
    q = ((3.0 * u + 0.05 * torch.randn(T, Hq, D, generator=g)) * (D ** 0.5 / 3.0)).to(torch.bfloat16)
    ks = vs = None
    if fp8:
        ks, vs = float(kc.abs().max()) / 448.0, float(vc.abs().max()) / 448.0
        kc, vc = O.fp8_sat(kc / ks, "e4m3"), O.fp8_sat(vc / vs, "e4m3")
    else:
        kc, vc = kc.to(torch.bfloat16), vc.to(torch.bfloat16)
    qsl = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    return SimpleNamespace(q=q, kc=kc, vc=vc, bt=bt, qsl=qsl, ks=ks, vs=vs, q_lens=list(q_lens), ctxs=list(ctxs), Hq=Hq,
                           Hkv=Hkv, D=D, bs=bs, window=int(window or 0), sinks=sinks, scale=D ** -0.5)
