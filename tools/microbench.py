#!/usr/bin/env python3
"""Per-kernel timings on the GPU box (not part of the bench contract; used while tuning)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from arcticinference_amd import ops
from arcticinference_amd import _native as N

dev = "cuda"


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def attn(B=64, ctx=4096, qlen=4, Hq=32, Hkv=8, D=128, bs=16, layers=4, split=False, kv8=False):
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    kvs = [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(layers)]
    kw = {}
    if kv8:   # e4m3 cache: random codes without the NaN patterns
        kvs = []
        for _ in range(layers):
            raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
            raw[(raw & 0x7f) == 0x7f] = 0x30
            kvs.append(raw.view(torch.float8_e4m3fn))
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    T = B * qlen
    q = torch.randn(T, Hq, D, device=dev, dtype=torch.bfloat16)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = (torch.arange(B + 1, device=dev) * qlen).to(torch.int32)
    out = torch.empty_like(q)
    # split=True: go through the request-list path (all requests short) like the engine does
    rs = (torch.arange(B, dtype=torch.int32, device=dev), B, None, 0) if split else None
    if split and qlen * (Hq // Hkv) > 16:
        rs = ops.split_requests([qlen] * B, Hq // Hkv, dev)
    i = [0]

    def f():
        kv = kvs[i[0] % layers]
        i[0] += 1
        ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, qlen, ctx, D ** -0.5, out=out, req_split=rs, **kw)
    us = timeit(f)
    gb = B * ctx * 2 * Hkv * D * (1 if kv8 else 2) / 1e9
    print(f"attn{' fp8kv' if kv8 else ''} B={B} ctx={ctx} qlen={qlen} Hq={Hq} Hkv={Hkv} D={D}: {us:8.1f} us  {gb / us * 1e6 / 1e3:6.2f} TB/s (incl. combine)")


def attn_dtypes(B=64, ctx=4096, qlen=4, Hq=32, Hkv=8, D=128, bs=16, layers=4, split=False, kv8=False, n_short=0, n_long=0,
                rounds=5, iters=20):
    """attn() / attn_mix() geometry for a bf16 and an fp16 model in ONE process, alternating: same block table, same
    request lists, fresh random q / caches of each type (an e4m3 cache is shared).  `rounds` timed windows per type,
    interleaved bf16, fp16, bf16, ...; prints each type's minimum, median and maximum and the ratio of the medians, so the
    difference between the types can be read against the run's own spread."""
    ql = [1] * n_short + [33] * n_long if (n_short or n_long) else [qlen] * B
    B = len(ql)
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    rs = ops.split_requests(ql, Hq // Hkv, dev) if (split or n_long) else None
    kw, kv_shared = {}, None
    if kv8:
        kv_shared = []
        for _ in range(layers):
            raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
            raw[(raw & 0x7f) == 0x7f] = 0x30
            kv_shared.append(raw.view(torch.float8_e4m3fn))
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    fns = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        kvs = kv_shared or [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=dt) for _ in range(layers)]
        q = torch.randn(sum(ql), Hq, D, device=dev, dtype=dt)
        out = torch.empty_like(q)

        def f(kvs=kvs, q=q, out=out, i=[0]):
            kv = kvs[i[0] % layers]
            i[0] += 1
            ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, max(ql), ctx, D ** -0.5, out=out, req_split=rs, **kw)
        fns[name] = f
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            times[name].append(timeit(f, iters=iters))
    med = {name: float(np.median(t)) for name, t in times.items()}
    shape = f"short={n_short}x1 long={n_long}x33" if (n_short or n_long) else f"B={B} qlen={qlen}"
    print(f"attn-dtypes{' fp8kv' if kv8 else ''} {shape} ctx={ctx} Hq={Hq} Hkv={Hkv} D={D}{' lists' if rs else ''}: " +
          "  ".join(f"{name} min {min(t):7.1f} med {med[name]:7.1f} max {max(t):7.1f} us" for name, t in times.items()) +
          f"  fp16 / bf16 {med['fp16'] / med['bf16']:.3f}", flush=True)


def attn_prefix(B=64, ctx=4224, P=2048, qlen=4, Hq=32, Hkv=8, D=128, bs=16, layers=4, kv8=False, rounds=5, iters=20):
    """The same call with and without its shared prefix (ops.verify_attention(..., shared_prefix_len, prefix_block_table):
    aic_verify_attention_prefix against aic_verify_attention_dt), alternating in ONE process as attn_dtypes does.  The first
    P tokens of every request sit in the same pages (the leading block-table columns are equal), so both forms compute the
    same thing; the plain one streams those pages once per request.  Prints each form's minimum / median / maximum, the
    algorithmic KV bytes of both (partials not counted) with the rate each achieves, and the measured ratio of the medians
    against the byte model (B (ctx - P) + P) / (B ctx)."""
    ql = [qlen] * B
    nblk = (ctx + bs - 1) // bs
    n_sh = P // bs
    nb = n_sh + B * (nblk - n_sh)
    perm = torch.randperm(nb, device=dev).to(torch.int32)
    bt = torch.empty(B, nblk, dtype=torch.int32, device=dev)
    bt[:, :n_sh] = perm[:n_sh]
    bt[:, n_sh:] = perm[n_sh:].view(B, nblk - n_sh)
    table = bt[0, :n_sh].contiguous()
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    kw = {}
    if kv8:
        kvs = []
        for _ in range(layers):
            raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
            raw[(raw & 0x7f) == 0x7f] = 0x30
            kvs.append(raw.view(torch.float8_e4m3fn))
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    else:
        kvs = [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(layers)]
    q = torch.randn(sum(ql), Hq, D, device=dev, dtype=torch.bfloat16)
    outs = {name: torch.empty_like(q) for name in ("plain", "prefix")}
    extra = {"plain": {}, "prefix": dict(shared_prefix_len=P, prefix_block_table=table)}
    fns = {}
    for name in outs:
        def f(name=name, i=[0]):
            kv = kvs[i[0] % layers]
            i[0] += 1
            ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, qlen, ctx, D ** -0.5, out=outs[name], req_split=rs, **kw,
                                 **extra[name])
        fns[name] = f
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            times[name].append(timeit(f, iters=iters))
    diff = float((outs["plain"].float() - outs["prefix"].float()).abs().max())
    med = {name: float(np.median(t)) for name, t in times.items()}
    per_tok = 2 * Hkv * D * (1 if kv8 else 2)
    mb = {"plain": B * ctx * per_tok / 1e6, "prefix": (B * (ctx - P) + P) * per_tok / 1e6}
    print(f"prefix{' fp8kv' if kv8 else ''} B={B} ctx={ctx} P={P} qlen={qlen} Hq={Hq} Hkv={Hkv}: " +
          "  ".join(f"{name} min {min(t):7.1f} med {med[name]:7.1f} max {max(t):7.1f} us  {mb[name]:6.1f} MB "
                    f"{mb[name] / med[name]:5.2f} TB/s" for name, t in times.items()) +
          f"  prefix / plain {med['prefix'] / med['plain']:.3f} (bytes {mb['prefix'] / mb['plain']:.3f})  max |diff| {diff:.2g}",
          flush=True)


def _alternate(fns, rounds, iters):
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            times[name].append(timeit(f, iters=iters))
    return times, {name: float(np.median(t)) for name, t in times.items()}


def _random_tree(n, rng, bushy=0.5):
    """n draft nodes in SuffixSpecResult form (tokens distinct): a node hangs under the previous one or under any earlier."""
    return ([int(x) for x in rng.permutation(30000)[:n]],
            [c - 1 if rng.random() >= bushy else int(rng.integers(-1, c)) for c in range(n)])


def attn_tree(B=64, n_draft=3, ctx=4224, Hq=32, Hkv=8, D=128, bs=16, layers=4, kv8=False, tree=False, rounds=5, iters=20):
    """aic_verify_attention_tree against the plain call on the same step, alternating in ONE process: `lists` is the
    plain call as the engine makes it (host query lengths: per-request tile choice, the long-draft body for long drafts),
    `generic` the plain call without lists (the launch form the tree call shares), `chain` the tree call with
    lower-triangular masks (computes what `generic` does, bit for bit), `tree` (with tree=True) the tree call on random
    trees of n_draft nodes.  Prints each form's minimum / median / maximum and the ratios of the medians."""
    rng = np.random.default_rng(n_draft + B)
    q_len = n_draft + 1
    ql = [q_len] * B
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    kw = {}
    if kv8:
        kvs = []
        for _ in range(layers):
            raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
            raw[(raw & 0x7f) == 0x7f] = 0x30
            kvs.append(raw.view(torch.float8_e4m3fn))
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    else:
        kvs = [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(layers)]
    q = torch.randn(sum(ql), Hq, D, device=dev, dtype=torch.bfloat16)
    chain = ops.TreeDrafts([(list(range(n_draft)), list(range(-1, n_draft - 1)))] * B, dev)
    forms = {"lists": None, "generic": None, "chain": chain}
    if tree:
        forms["tree"] = ops.TreeDrafts([_random_tree(n_draft, rng) for _ in range(B)], dev)
    outs = {name: torch.empty_like(q) for name in forms}
    fns = {}
    for name, td in forms.items():
        def f(name=name, td=td, i=[0]):
            kv = kvs[i[0] % layers]
            i[0] += 1
            if td is None:
                ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, q_len, ctx, D ** -0.5, out=outs[name],
                                     req_split=rs if name == "lists" else None, **kw)
            else:
                ops.verify_attention_tree(q, kv[0], kv[1], bt, seq, td, ctx, D ** -0.5, out=outs[name], **kw)
        fns[name] = f
    times, med = _alternate(fns, rounds, iters)
    same = bool(torch.equal(outs["generic"], outs["chain"]))
    print(f"tree-attn{' fp8kv' if kv8 else ''} B={B} q_len={q_len} ctx={ctx} Hq={Hq} Hkv={Hkv}: " +
          "  ".join(f"{name} min {min(t):7.1f} med {med[name]:7.1f} max {max(t):7.1f} us" for name, t in times.items()) +
          f"  chain / generic {med['chain'] / med['generic']:.3f}  chain / lists {med['chain'] / med['lists']:.3f}" +
          (f"  tree / chain {med['tree'] / med['chain']:.3f}" if tree else "") + f"  chain == generic: {same}", flush=True)


def tree_accept_compact(B=64, n_draft=32, V=128256, layers=32, Hkv=8, D=128, bs=16, ctx=256, kv8=False, rounds=5, iters=20):
    """The acceptance and compaction launches of a tree step: aic_rejection_tree_greedy over B trees of n_draft nodes
    against aic_rejection_greedy over B chains of the same length (same logits, row_index forms), and aic_kv_compact_paths
    over `layers` layers on the paths the acceptance took (logits planted so that every walk goes three levels deep through
    a node's LAST child: rows move).  The caches are small (ctx tokens per request): the launch touches a few rows of each."""
    rng = np.random.default_rng(B + n_draft)
    trees = [_random_tree(n_draft, rng) for _ in range(B)]
    td = ops.TreeDrafts(trees, dev)
    lay = td.layout
    T = td.num_tokens
    logits = torch.randn(T, V, device=dev, dtype=torch.bfloat16)
    for i in range(B):
        q0, n, cur = int(lay.query_start_loc[i]), int(lay.q_lens[i]), 0
        for _ in range(3):
            kids = [c for c in range(1, n) if lay.parents[q0 + c] == cur]
            if not kids:
                break
            logits[q0 + cur, int(lay.tokens[q0 + kids[-1]])] = 64.0
            cur = kids[-1]
    q_len = n_draft + 1
    draft_rows = torch.tensor(np.concatenate([np.arange(i * q_len, i * q_len + n_draft) for i in range(B)]), device=dev)
    bonus_rows = torch.tensor(np.arange(B) * q_len + n_draft, device=dev)
    drafts = td.draft_token_ids.view(B, q_len)[:, 1:].reshape(-1).contiguous()
    cu = torch.tensor(np.arange(1, B + 1) * n_draft, dtype=torch.int32, device=dev)
    res = ops.rejection_sample_tree(logits, td)
    fns = {"tree": lambda: ops.rejection_sample_tree(logits, td),
           "chain": lambda: ops.rejection_sample(logits, drafts, cu, None, n_draft, target_row_index=draft_rows,
                                                 bonus_row_index=bonus_rows)}
    times, med = _alternate(fns, rounds, iters)
    print(f"tree-accept B={B} n_draft={n_draft} V={V}: " +
          "  ".join(f"{name} min {min(t):7.1f} med {med[name]:7.1f} max {max(t):7.1f} us" for name, t in times.items()) +
          f"  tree / chain {med['tree'] / med['chain']:.3f}  mean accepted {float(res.num_accepted.float().mean()):.2f}", flush=True)
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    dt = torch.uint8 if kv8 else torch.bfloat16
    kcs = [torch.zeros(nb, bs, Hkv, D, dtype=dt, device=dev) for _ in range(layers)]
    vcs = [torch.zeros(nb, bs, Hkv, D, dtype=dt, device=dev) for _ in range(layers)]
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    moved = int(((res.path != torch.arange(res.path.size(1), device=dev)) & (res.path >= 0)).sum())
    comp = ops.KvPathCompactor(kcs, vcs)                      # pointer tables built once, as a runner would
    us = [timeit(lambda: comp(bt, seq, td, res.path, res.num_accepted), iters=iters) for _ in range(rounds)]
    ident = torch.arange(res.path.size(1), dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
    us0 = [timeit(lambda: comp(bt, seq, td, ident, res.num_accepted), iters=iters) for _ in range(rounds)]
    us1 = [timeit(lambda: ops.compact_accepted_paths(kcs, vcs, bt, seq, td, res.path, res.num_accepted), iters=iters)
           for _ in range(rounds)]
    print(f"tree-compact{' 1-byte' if kv8 else ''} B={B} layers={layers} Hkv={Hkv} D={D}: {moved} rows move per cache: min {min(us):7.1f} "
          f"med {float(np.median(us)):7.1f} max {max(us):7.1f} us; identity paths (nothing moves) med {float(np.median(us0)):7.1f} us; "
          f"through ops.compact_accepted_paths (tables rebuilt per call: host-bound) med {float(np.median(us1)):7.1f} us", flush=True)


def attn_prefix_groups(sizes, P, loners=0, ctx=4224, qlen=4, Hq=32, Hkv=8, D=128, bs=16, layers=4, kv8=False, rounds=5,
                       iters=20, single=False):
    """The same call plain and with its prefix groups (ops.verify_attention(..., prefix_groups=):
    aic_verify_attention_prefix_groups against aic_verify_attention_dt), alternating in ONE process as attn_prefix does.
    `sizes[g]` requests share their first `P[g]` tokens' pages (P: one length, or one per group), `loners` more share
    nothing; members of the groups are interleaved in batch order.  `single`: with one group of everybody, the
    single-prefix call (aic_verify_attention_prefix) takes part too.  Prints, per form, the median of `rounds` windows in
    us per call (combine included) and the run's own max - min spread, and the ratios of the medians."""
    lens = [P] * len(sizes) if isinstance(P, int) else list(P)
    B = sum(sizes) + loners
    req_group = []
    left = list(sizes)
    while any(left):                       # round-robin over the groups: A B C A B C ...
        for g in range(len(sizes)):
            if left[g]:
                req_group.append(g)
                left[g] -= 1
    req_group += [-1] * loners
    ql = [qlen] * B
    nblk = (ctx + bs - 1) // bs
    n_sh = [l // bs for l in lens]
    nb = sum(n_sh) + sum(nblk - (n_sh[g] if g >= 0 else 0) for g in req_group)
    perm = torch.randperm(nb, dtype=torch.int32)
    bt = torch.empty(B, nblk, dtype=torch.int32)
    k = 0
    shared = []
    for n in n_sh:
        shared.append(perm[k:k + n])
        k += n
    for i, g in enumerate(req_group):
        first = 0
        if g >= 0:
            first = n_sh[g]
            bt[i, :first] = shared[g]
        bt[i, first:] = perm[k:k + nblk - first]
        k += nblk - first
    bt = bt.to(dev)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    kw = {}
    if kv8:
        kvs = []
        for _ in range(layers):
            raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
            raw[(raw & 0x7f) == 0x7f] = 0x30
            kvs.append(raw.view(torch.float8_e4m3fn))
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    else:
        kvs = [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(layers)]
    q = torch.randn(sum(ql), Hq, D, device=dev, dtype=torch.bfloat16)
    groups = ops.PrefixGroups(req_group, lens, ql, dev)       # once, as a step builds it for all its layers
    extra = {"plain": {}, "groups": dict(prefix_groups=groups)}
    if single:
        assert len(sizes) == 1 and not loners
        extra["prefix"] = dict(shared_prefix_len=lens[0], prefix_block_table=bt[0, :n_sh[0]].contiguous())
    outs = {name: torch.empty_like(q) for name in extra}
    fns = {}
    for name in outs:
        def f(name=name, i=[0]):
            kv = kvs[i[0] % layers]
            i[0] += 1
            ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, qlen, ctx, D ** -0.5, out=outs[name], req_split=rs, **kw,
                                 **extra[name])
        fns[name] = f
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            times[name].append(timeit(f, iters=iters))
    diff = max(float((outs["plain"].float() - outs[name].float()).abs().max()) for name in outs)
    med = {name: float(np.median(t)) for name, t in times.items()}
    shape = " + ".join(f"{n}x P={l}" for n, l in zip(sizes, lens)) + (f" + {loners} ungrouped" if loners else "")
    print(f"prefixgroups{' fp8kv' if kv8 else ''} B={B} ({shape}) ctx={ctx} qlen={qlen} Hq={Hq} Hkv={Hkv}: " +
          "  ".join(f"{name} med {med[name]:7.1f} spread {max(t) - min(t):5.1f} us" for name, t in times.items()) +
          f"  groups / plain {med['groups'] / med['plain']:.3f}" +
          (f"  groups / prefix {med['groups'] / med['prefix']:.3f}" if single else "") + f"  max |diff| {diff:.2g}", flush=True)


def attn_mix(n_short=59, n_long=5, q_short=1, q_long=33, ctx=4224, Hq=32, Hkv=8, D=128, bs=16, layers=4, kv8=False):
    """The steady-state step of bench.py: most requests carry no draft (q_len 1), a few a long suffix draft — one call
    through the host-partitioned path (pair kernel) against its parts."""
    B = n_short + n_long
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    kvs = [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(layers)]
    kw = {}
    if kv8:
        kvs = []
        for _ in range(layers):
            raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
            raw[(raw & 0x7f) == 0x7f] = 0x30
            kvs.append(raw.view(torch.float8_e4m3fn))
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    ql = [q_short] * n_short + [q_long] * n_long
    T = sum(ql)
    q = torch.randn(T, Hq, D, device=dev, dtype=torch.bfloat16)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    out = torch.empty_like(q)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    i = [0]

    def f():
        kv = kvs[i[0] % layers]
        i[0] += 1
        ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, max(ql), ctx, D ** -0.5, out=out, req_split=rs, **kw)
    us = timeit(f)
    gb = B * ctx * 2 * Hkv * D * (1 if kv8 else 2) / 1e9
    print(f"attn-mix{' fp8kv' if kv8 else ''} short={n_short}x{q_short} long={n_long}x{q_long} ctx={ctx} Hq={Hq} Hkv={Hkv}: {us:8.1f} us  "
          f"{gb / us * 1e6 / 1e3:6.2f} TB/s (incl. combine)")


def attn_ql(ql, ctx=4224, Hq=32, Hkv=8, D=128, bs=16, layers=4, jitter=0):
    """One host-partitioned call over an arbitrary list of query lengths (contexts ctx - jitter .. ctx)."""
    B = len(ql)
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    kvs = [torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16) for _ in range(layers)]
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    q = torch.randn(sum(ql), Hq, D, device=dev, dtype=torch.bfloat16)
    rng = np.random.default_rng(0)
    ctxs = ctx - (rng.integers(0, jitter + 1, B) if jitter else np.zeros(B, np.int64))
    seq = torch.tensor(ctxs, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    out = torch.empty_like(q)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    i = [0]

    def f():
        kv = kvs[i[0] % layers]
        i[0] += 1
        ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, max(ql), ctx, D ** -0.5, out=out, req_split=rs)
    us = timeit(f)
    gb = float(ctxs.sum()) * 2 * Hkv * D * 2 / 1e9
    hist = {k: ql.count(k) for k in sorted(set(ql))}
    print(f"attn-ql {hist} ctx<={ctx} jitter={jitter} short/long={rs[1]}/{rs[3]}: {us:8.1f} us  {gb / us * 1e6 / 1e3:6.2f} TB/s (incl. combine)")


def attn_trace(n_short=59, n_long=5, q_short=1, q_long=33, ctx=4224, Hq=32, Hkv=8, D=128, bs=16):
    """Where and when the workgroups of the one-grid short + long launch run (aic_debug_attn_trace)."""
    B = n_short + n_long
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    kv = torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16)
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    ql = [q_short] * n_short + [q_long] * n_long
    q = torch.randn(sum(ql), Hq, D, device=dev, dtype=torch.bfloat16)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    out = torch.empty_like(q)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    run = lambda: ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, max(ql), ctx, D ** -0.5, out=out, req_split=rs)
    for _ in range(3):
        run()
    buf = torch.full((2048, 4), -1, dtype=torch.int64, device=dev)
    N.lib().aic_debug_attn_trace(buf.data_ptr(), 2048)
    run()
    torch.cuda.synchronize()
    N.lib().aic_debug_attn_trace(None, 0)
    t = buf.cpu().numpy()
    t = t[t[:, 3] >= 0]
    t0 = t[:, 0].min()
    start, end = (t[:, 0] - t0) / 100.0, (t[:, 1] - t0) / 100.0       # us
    hw, xcc = t[:, 2] & 0xffffffff, t[:, 2] >> 32
    cu = (xcc & 0xf) * 64 + ((hw >> 13) & 7) * 16 + ((hw >> 8) & 0xf)      # (xcc, se, cu) -> one id
    print(f"trace short={n_short}x{q_short} long={n_long}x{q_long}: {len(t)} workgroups, kernel {end.max():.1f} us")
    for kind, name in ((1, "long"), (0, "short")):
        m = t[:, 3] == kind
        if not m.any():
            continue
        print(f"  {name:5s}: n={m.sum():4d}  start min/med/max {start[m].min():7.1f} {np.median(start[m]):7.1f} {start[m].max():7.1f}   "
              f"end min/med/max {end[m].min():7.1f} {np.median(end[m]):7.1f} {end[m].max():7.1f}   duration med {np.median(end[m] - start[m]):7.1f}   "
              f"distinct CUs {len(set(cu[m]))}")
    both = set(cu[t[:, 3] == 1]) & set(cu[t[:, 3] == 0])
    per_cu = {}
    for c, k in zip(cu, t[:, 3]):
        per_cu.setdefault(int(c), []).append(int(k))
    if os.environ.get("AIC_TRACE_DETAIL"):     # which short workgroups (by launch index) share a CU with a long one, and how long they ran
        long_cus = set(cu[t[:, 3] == 1].tolist())
        idx = np.nonzero(t[:, 3] == 0)[0]
        shared = np.array([int(cu[i]) in long_cus for i in idx])
        dur = (end - start)[idx]
        n = len(idx)
        print(f"  short workgroups in launch order, 16 bins: share of each bin on a CU with a long workgroup / median duration")
        for b in range(16):
            sl = slice(b * n // 16, (b + 1) * n // 16)
            print(f"    bin {b:2d}: shared {shared[sl].mean():.2f}  dur {np.median(dur[sl]):6.1f}  (max {dur[sl].max():6.1f})")
        print(f"  shared: median dur {np.median(dur[shared]) if shared.any() else 0:.1f}; alone: {np.median(dur[~shared]) if (~shared).any() else 0:.1f}")
    mix = sorted((tuple(sorted(v)) for v in per_cu.values()))
    from collections import Counter
    print(f"  CUs used {len(per_cu)}; CUs with both kinds {len(both)}; per-CU mix {Counter(mix).most_common(6)}")


def attn_phases(n_short=32, ctx=4224, kv8=False, Hq=32, Hkv=8, D=128, bs=16):
    """Where a short-only launch's time goes per workgroup (aic_debug_attn_phase_trace): entry -> request geometry known ->
    first tile requested -> [tile loop] -> partials stored, and when the workgroups start and end within the launch."""
    B = n_short
    nblk = (ctx + bs - 1) // bs
    nb = B * nblk
    if kv8:
        raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
        raw[(raw & 0x7f) == 0x7f] = 0x30
        kv = raw.view(torch.float8_e4m3fn)
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    else:
        kv = torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16)
        kw = {}
    # (a second cache to evict the first from the last-level cache between launches)
    other = torch.randn(64 * 1024 * 1024, device=dev)
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B, nblk)
    q = torch.randn(B, Hq, D, device=dev, dtype=torch.bfloat16)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.arange(B + 1, device=dev).to(torch.int32)
    out = torch.empty_like(q)
    rs = ops.split_requests([1] * B, Hq // Hkv, dev)
    run = lambda: ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, 1, ctx, D ** -0.5, out=out, req_split=rs, **kw)
    for _ in range(3):
        run()
    other.mul_(1.0001)
    buf = torch.zeros((4096, 8), dtype=torch.int64, device=dev)
    N.lib().aic_debug_attn_phase_trace(buf.data_ptr(), 4096)
    run()
    torch.cuda.synchronize()
    N.lib().aic_debug_attn_phase_trace(None, 0)
    t = buf.cpu().numpy()
    t = t[t[:, 0] > 0]
    us = lambda a: a / 100.0
    t0 = t[:, 0].min()
    tiles = (t[:, 6] >> 32) / 32.0
    med = lambda a: float(np.median(us(a)))
    print(f"attn-phases {'fp8' if kv8 else 'bf16'} cache, {n_short} requests x {ctx} tokens: {len(t)} workgroups, "
          f"{np.median(tiles):.0f} tiles per wave; launch (first start -> last end) {us(t[:, 5].max() - t0):.1f} us")
    print(f"   workgroup start after the first: median {med(t[:, 0] - t0):.2f} max {us((t[:, 0] - t0).max()):.2f} us")
    print(f"   entry -> request geometry known (request list, lengths): median {med(t[:, 1] - t[:, 0]):.2f} us")
    print(f"   geometry -> first tile requested (Q fragments, block table, K / V loads issued): {med(t[:, 2] - t[:, 1]):.2f} us")
    print(f"   tile loop: median {med(t[:, 4] - t[:, 2]):.2f} us = {med(t[:, 4] - t[:, 2]) / np.median(tiles):.3f} us per 32-token tile "
          f"(min {us((t[:, 4] - t[:, 2]).min()):.1f}, max {us((t[:, 4] - t[:, 2]).max()):.1f})")
    print(f"   loop end -> partials stored: {med(t[:, 5] - t[:, 4]):.2f} us;  workgroup total median {med(t[:, 5] - t[:, 0]):.1f} us; "
          f"last end - median end {us(t[:, 5].max() - np.median(t[:, 5])):.1f} us")


def attn_long_phases(B=16, q_long=33, ctx=4096, Hq=32, Hkv=8, D=128, bs=16, n_short=0):
    """Shader-clock cycle accounting of the long-draft body per wave (aic_debug_attn_phase_trace on a long-only call, or —
    n_short > 0 — on the long workgroups of a mixed call, which share their CUs with short-request workgroups)."""
    nblk = (ctx + bs - 1) // bs
    nb = (B + n_short) * nblk
    kv = torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16)
    bt = torch.randperm(nb, device=dev).to(torch.int32).view(B + n_short, nblk)
    ql = [1] * n_short + [q_long] * B
    B = B + n_short
    q = torch.randn(sum(ql), Hq, D, device=dev, dtype=torch.bfloat16)
    seq = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(ql)]).astype(np.int32), device=dev)
    out = torch.empty_like(q)
    rs = ops.split_requests(ql, Hq // Hkv, dev)
    run = lambda: ops.verify_attention(q, kv[0], kv[1], bt, seq, qsl, max(ql), ctx, D ** -0.5, out=out, req_split=rs)
    us = timeit(run)
    cap = 32768
    buf = torch.zeros((cap, 8), dtype=torch.int64, device=dev)     # two rows of 8 per wave
    N.lib().aic_debug_attn_phase_trace(buf.data_ptr(), cap)
    us_tr = timeit(run)
    N.lib().aic_debug_attn_phase_trace(None, 0)
    t = buf.cpu().numpy().reshape(-1, 16)
    t = t[t[:, 7] > 0]
    n_iter, tiles = t[:, 6] >> 8, t[:, 6] & 0xff
    dur_us = (t[:, 7] - t[:, 10]) / 100.0
    ghz = float(np.median(t[:, 11] / np.maximum(dur_us, 1e-3))) / 1e3
    start = (t[:, 10] - t[:, 10].min()) / 100.0
    print(f"long-phases {n_short} short + {B - n_short} x {q_long} tokens, ctx {ctx}: call {us:.1f} us (traced build {us_tr:.1f} us); {len(t) // 4} workgroups, "
          f"{int(np.median(n_iter))} KV tiles each; shader clock {ghz:.2f} GHz; wave start after the first: median {np.median(start):.1f} "
          f"max {start.max():.1f} us; wave duration min / median / max {dur_us.min():.1f} / {np.median(dur_us):.1f} / {dur_us.max():.1f} us")
    print("   cycles per KV tile and wave, by the wave's row tiles (MFMA issue is asynchronous: a phase that needs results waits for them)")
    for k in sorted(set(tiles.tolist())):
        m = tiles == k
        it = np.maximum(n_iter[m], 1).astype(np.float64)
        f = lambda c: float(np.median(t[m, c] / it))
        print(f"   {k} row tiles ({m.sum():5d} waves): loop {f(1):6.0f} = vmcnt wait {f(8):5.0f} | barrier {f(9):5.0f} | next tile's DMA issued {f(2):5.0f} | "
              f"K reads + score MFMAs issued {f(3):5.0f} | soft-max {f(4):5.0f} | V reads + PV MFMAs issued {f(5):5.0f};  prologue {float(np.median(t[m, 0])):6.0f}")


def _prefill_case(q_lens, ctxs, Hq, Hkv, D=128, bs=16, kv8=False):
    """Paged caches + q for a step of requests with the given query lengths and contexts (random data)."""
    nblk = [(c + bs - 1) // bs for c in ctxs]
    nb = sum(nblk)
    if kv8:
        raw = torch.randint(0, 256, (2, nb, bs, Hkv, D), dtype=torch.uint8, device=dev)
        raw[(raw & 0x7f) == 0x7f] = 0x30
        kv = raw.view(torch.float8_e4m3fn)
        sc = torch.full((1,), 0.02, dtype=torch.float32, device=dev)
        kw = dict(k_scale=sc, v_scale=sc)
    else:
        kv = torch.randn(2, nb, bs, Hkv, D, device=dev, dtype=torch.bfloat16)
        kw = {}
    perm = torch.randperm(nb, device=dev).to(torch.int32)
    bt = torch.zeros(len(ctxs), max(nblk), dtype=torch.int32, device=dev)
    k = 0
    for i, n in enumerate(nblk):
        bt[i, :n] = perm[k:k + n]
        k += n
    T = sum(q_lens)
    q = torch.randn(T, Hq, D, device=dev, dtype=torch.bfloat16)
    seq = torch.tensor(ctxs, dtype=torch.int32, device=dev)
    qsl = torch.tensor(np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32), device=dev)
    return q, kv, bt, seq, qsl, kw


def _visible_keys(q_lens, ctxs, decode_too=True, window=0):
    """Keys the rows see: position p sees p + 1 keys, or min(p + 1, window) with a sliding window."""
    w = window if window > 0 else 1 << 62
    return sum(sum(min(c - n + i + 1, w) for i in range(n)) for n, c in zip(q_lens, ctxs) if decode_too or n > 33)


def prefill(q_lens, ctxs, Hq=32, Hkv=8, D=128, bs=16, kv8=False, label="", sdpa=False, window=0, sinks=False):
    """aic_step_attention_win on one step: us per call and TFLOP/s with FLOPs = 4 D Hq sum(keys inside each row's
    window).  A window layer reads O(window) keys per row whatever the context: latency-bound, its us per call is the
    figure to read."""
    q, kv, bt, seq, qsl, kw = _prefill_case(q_lens, ctxs, Hq, Hkv, D, bs, kv8)
    split = ops.StepSplit(q_lens, Hq // Hkv, dev)
    out = torch.empty_like(q)
    if window:
        kw["sliding_window"] = window
    if sinks:
        kw["sinks"] = torch.randn(Hq, device=dev, dtype=torch.float32)

    def f():
        ops.step_attention(q, kv[0], kv[1], bt, seq, qsl, max(ctxs), D ** -0.5, step_split=split, out=out, **kw)
    us = timeit(f, iters=10, warm=2)
    fl = 4.0 * D * Hq * _visible_keys(q_lens, ctxs, window=window)
    feat = (f" D={D}" if D != 128 else "") + (f" W={window}" if window else "") + (" sinks" if sinks else "")
    print(f"prefill{' fp8kv' if kv8 else ''} {label} Hq={Hq} Hkv={Hkv}{feat} bs={bs}: {us:9.1f} us  {fl / us / 1e6:7.1f} TFLOP/s")
    if sdpa:   # reference point: torch SDPA on K/V gathered into contiguous tensors (single request, bf16 only)
        (n,), (c,) = q_lens, ctxs
        nblk = (c + bs - 1) // bs
        K = kv[0][bt[0, :nblk].long()].reshape(-1, Hkv, D)[:c].transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        V = kv[1][bt[0, :nblk].long()].reshape(-1, Hkv, D)[:c].transpose(0, 1).repeat_interleave(Hq // Hkv, 0)
        Q = q.transpose(0, 1)
        mask = torch.arange(c, device=dev)[None, :] <= (torch.arange(n, device=dev)[:, None] + c - n)
        us2 = timeit(lambda: torch.nn.functional.scaled_dot_product_attention(Q, K, V, attn_mask=mask), iters=10, warm=2)
        print(f"  torch sdpa (contiguous K/V, explicit mask)  : {us2:9.1f} us  {fl / us2 / 1e6:7.1f} TFLOP/s")
    return us


def prefill_suite():
    for kv8 in (False, True):
        for n, c in ((512, 4096), (2048, 4096), (2048, 8192)):
            prefill([n], [c], kv8=kv8, label=f"llama-8b chunk {n} ctx {c}", sdpa=not kv8)
    for c in (16384, 32768):        # Llama-70B SP = 8 slice: one kv head per rank
        prefill([8192], [c], Hq=8, Hkv=1, label=f"llama-70b sp8 chunk 8192 ctx {c}")
        prefill([8192], [c], Hq=8, Hkv=1, kv8=True, label=f"llama-70b sp8 chunk 8192 ctx {c}")
    # mixed call: 63 decoding requests (q_len 1..33) at ctx ~4096 + one 2048-token chunk (the last of a 4096-token prompt)
    rng = np.random.default_rng(0)
    dq = [int(x) for x in rng.integers(1, 34, 63)]
    dc = [int(x) for x in rng.integers(3968, 4224, 63)]
    mixed = prefill(dq[:31] + [2048] + dq[31:], dc[:31] + [4096] + dc[31:], label="mixed 63 decodes + chunk 2048")
    dec = prefill(dq, dc, label="decode-only 63")
    chunk = prefill([2048], [4096], label="chunk-only 2048")
    print(f"mixed / (decode-only + chunk-only) = {mixed / (dec + chunk):.3f}")
    # gpt-oss-120b (Hq 64, Hkv 8, head size 64; layers alternate a 128-token window and full attention, sinks on all)
    prefill([2048], [4096], Hq=64, Hkv=8, D=64, sinks=True, label="gpt-oss chunk 2048 ctx 4096", sdpa=True)
    for c in (4096, 16384, 32768):
        prefill([2048], [c], Hq=64, Hkv=8, D=64, window=128, sinks=True, label=f"gpt-oss chunk 2048 ctx {c}")
    for c in (16384, 32768):        # its SP = 8 slice: 8 query heads on one kv head per rank
        prefill([8192], [c], Hq=8, Hkv=1, D=64, sinks=True, label=f"gpt-oss sp8 chunk 8192 ctx {c}")
        prefill([8192], [c], Hq=8, Hkv=1, D=64, window=128, sinks=True, label=f"gpt-oss sp8 chunk 8192 ctx {c}")
    g = dict(Hq=64, Hkv=8, D=64, window=128, sinks=True)
    mixed = prefill(dq[:31] + [2048] + dq[31:], dc[:31] + [4096] + dc[31:], label="gpt-oss mixed 63 decodes + chunk 2048", **g)
    dec = prefill(dq, dc, label="gpt-oss decode-only 63", **g)
    chunk = prefill([2048], [4096], label="gpt-oss chunk-only 2048", **g)
    print(f"gpt-oss W=128 mixed / (decode-only + chunk-only) = {mixed / (dec + chunk):.3f}")


def lstm(B, fp8=True):
    from arcticinference_amd.speculator import ArcticLSTMSpeculator, LSTMSpeculatorConfig, random_lstm_weights
    cfg = LSTMSpeculatorConfig(vocab_size=128256, input_hidden_dim=4096)
    m = ArcticLSTMSpeculator(cfg, max_num_seqs=64, device=dev, quantize_lm_head=fp8, use_graph=False)
    m.load_weights(random_lstm_weights(cfg, seed=0).items())
    hid = torch.randn(B, 4096, device=dev, dtype=torch.bfloat16)
    ids = torch.randint(0, 128256, (B,), device=dev)
    head_gb = 128256 * 4096 * (1 if (fp8 and B <= 32) else 2) / 1e9
    gate_gb = 4 * 4096 * 4096 * 2 / 1e9
    # head-by-head schedule, the fused one with the cell as three launches (r03) and as one (r04, the default), fused +
    # on-the-fly fp8 activations (aic_debug_lstm_fused / aic_debug_lstm_cell_launches)
    for name, fused, cell in (("head-by-head", 0, 1), ("fused, 3-launch cell", 1, 3), ("fused, 1-launch cell", 1, 1), ("fused+xq", 2, 1)):
        N.lib().aic_debug_lstm_fused(fused)
        N.lib().aic_debug_lstm_cell_launches(cell)
        us = timeit(lambda: m.generate_proposals(ids, hid, 3), iters=10)
        print(f"lstm B={B} fp8={fp8 and B <= 32} {name}: {us:8.1f} us per 3-head propose; "
              f"weights {3 * (head_gb + gate_gb):.2f} GB -> {3 * (head_gb + gate_gb) / us * 1e6 / 1e3:5.2f} TB/s "
              f"({3 * (head_gb + gate_gb) / us * 1e6 / 1e3 / 8:.2f} of 8 TB/s)")
    N.lib().aic_debug_lstm_fused(1)
    N.lib().aic_debug_lstm_cell_launches(1)
    for graph in (False, True):
        m.use_graph = graph
        us = timeit(lambda: m.generate_proposals(ids, hid, 3), iters=10)
        print(f"lstm B={B} fp8={fp8 and B <= 32} fused, 1-launch cell, {'HIP graph replay' if graph else 'eager launches'}: {us:8.1f} us "
              f"({3 * (head_gb + gate_gb) / us * 1e6 / 1e3 / 8:.2f} of 8 TB/s)")
    del m
    torch.cuda.empty_cache()


def lstm_wide(sizes=(64, 96, 128, 192, 256), reps=5, iters=5):
    """Batches above 64 rows (bf16 head, Llama-8B speculator shape, k = 3): one native call on the wide GEMMs against the
    equivalent sequence of <= 64-row calls (draft_chunks(B, 64): what a 64-row cap would make of the batch, every weight
    byte streamed once per call).  The two alternate in one process; median and max - min spread of the repetitions.
    A width counts as served natively only if it wins by more than twice the larger spread."""
    from arcticinference_amd.speculator import ArcticLSTMSpeculator, LSTMSpeculatorConfig, draft_chunks, random_lstm_weights
    cfg = LSTMSpeculatorConfig(vocab_size=128256, input_hidden_dim=4096)
    m = ArcticLSTMSpeculator(cfg, max_num_seqs=256, device=dev, quantize_lm_head=False, use_graph=False)
    m.load_weights(random_lstm_weights(cfg, seed=0).items())
    gb = 3 * (128256 * 4096 * 2 + 4 * 4096 * 4096 * 2) / 1e9          # algorithmic weight bytes of a k = 3 draft
    for B in sizes:
        hid = torch.randn(B, 4096, device=dev, dtype=torch.bfloat16)
        ids = torch.randint(0, 128256, (B,), device=dev).to(torch.int32)
        parts, lo = [], 0
        for n in draft_chunks(B, 64):
            parts.append((ids[lo:lo + n], hid[lo:lo + n], n))
            lo += n
        one = lambda: m._draft(ids, hid, None, B, 3)
        seq = lambda: [m._draft(i, h, None, n, 3) for i, h, n in parts]
        same = torch.equal(one(), torch.cat(seq()))
        t_one, t_seq = [], []
        for _ in range(reps):
            t_one.append(timeit(one, iters=iters))
            t_seq.append(timeit(seq, iters=iters))
        med = lambda t: sorted(t)[len(t) // 2]
        spread = max(max(t_one) - min(t_one), max(t_seq) - min(t_seq))
        gain = med(t_seq) - med(t_one)
        print(f"lstm wide B={B:3d}: one call {med(t_one):8.1f} us (spread {max(t_one) - min(t_one):6.1f}, "
              f"{gb / med(t_one) * 1e3:5.2f} TB/s on {gb:.2f} GB)   {len(parts)} calls of <= 64 rows {med(t_seq):8.1f} us "
              f"(spread {max(t_seq) - min(t_seq):6.1f})   gain {gain:8.1f} us vs bar {2 * spread:6.1f}: "
              f"{'native' if len(parts) > 1 and gain > 2 * spread else ('same path' if len(parts) == 1 else 'NOT faster')}"
              f"   same tokens: {same}", flush=True)
    del m
    torch.cuda.empty_cache()


def rejection(B=64, k=3, V=128256):
    logits = torch.randn(B * k, V, device=dev, dtype=torch.bfloat16)
    draft = torch.randint(0, V, (B * k,), device=dev, dtype=torch.int32)
    cu = (torch.arange(1, B + 1, device=dev) * k).to(torch.int32)
    bonus = torch.zeros(B, dtype=torch.int32, device=dev)
    us = timeit(lambda: ops.rejection_sample(logits, draft, cu, bonus, k))
    print(f"rejection B={B} k={k}: {us:8.1f} us  {B * k * V * 2 / 1e9 / us * 1e6 / 1e3:5.2f} TB/s")



def _torch_topk_topp_accept(logits, draft, cu, bonus, temp_rows, k_rows, p_rows, u, q, req_rows, k):
    """vLLM 0.9.2's path for the same call, restated in torch on the same GPU: x = logits / T, apply_top_k_top_p (full
    ascending sort, softmax + cumsum in the logits dtype, scatter), softmax f32, then accept (p[draft] >= u) and
    recovery (argmax(p / q), p[draft] := 0) with the first-rejection scan."""
    x = (logits.float() / temp_rows.unsqueeze(1)).to(logits.dtype)
    if k_rows is not None or p_rows is not None:
        xs, xi = x.sort(dim=-1, descending=False)
        if k_rows is not None:
            xs = xs.masked_fill(xs < xs.gather(1, (xs.size(1) - k_rows).unsqueeze(1)), -float("inf"))
        if p_rows is not None:
            m = xs.softmax(dim=-1).cumsum(dim=-1) <= (1 - p_rows.to(x.dtype)).unsqueeze(1)
            m[:, -1] = False
            xs = xs.masked_fill(m, -float("inf"))
        x = xs.scatter(-1, xi, xs)
    p = x.softmax(dim=-1, dtype=torch.float32)
    pd = p.gather(1, draft.long().unsqueeze(1)).squeeze(1)
    acc = pd.double() >= u
    p.scatter_(1, draft.long().unsqueeze(1), 0.0)
    rec = (p / q[req_rows]).argmax(dim=-1).to(torch.int32)
    tok = torch.where(acc, draft, rec).view(-1, k)
    ok = acc.view(-1, k).int().cumprod(dim=1)
    first_rej = ok.sum(dim=1)
    out = torch.full((tok.shape[0], k + 1), -1, dtype=torch.int32, device=logits.device)
    pos = torch.arange(k + 1, device=logits.device)
    out[:, :k] = torch.where(pos[:k] <= first_rej.unsqueeze(1), tok, out[:, :k])
    out[:, k] = torch.where(first_rej == k, bonus, out[:, k])
    return out


def rejection_topk_topp(B=64, k=3, V=128256, top_k=None, top_p=None):
    """aic_rejection_random_topk_topp against the torch restatement of vLLM's sort-based path (same inputs)."""
    g = torch.Generator(device=dev).manual_seed(0)
    logits = (torch.randn(B * k, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    draft = torch.randint(0, V, (B * k,), device=dev, dtype=torch.int32, generator=g)
    cu = (torch.arange(1, B + 1, device=dev) * k).to(torch.int32)
    bonus = torch.zeros(B, dtype=torch.int32, device=dev)
    temp = torch.full((B,), 0.6, device=dev)
    u = torch.rand(B * k, dtype=torch.float64, device=dev, generator=g)
    q = torch.empty(B, V, device=dev).exponential_(generator=g)
    tk = None if top_k is None else torch.full((B,), top_k, dtype=torch.int32, device=dev)
    tp = None if top_p is None else torch.full((B,), top_p, dtype=torch.float32, device=dev)
    kw = dict(temperature=temp, uniform_probs=u, exp_noise=q, top_k=tk, top_p=tp)
    hip = timeit(lambda: ops.rejection_sample(logits, draft, cu, bonus, k, **kw))
    req = torch.arange(B, device=dev).repeat_interleave(k)
    args = (logits, draft, cu, bonus, temp[req], None if tk is None else tk[req].long(), None if tp is None else tp[req],
            u, q, req, k)
    ref = timeit(lambda: _torch_topk_topp_accept(*args))
    same = torch.equal(ops.rejection_sample(logits, draft, cu, bonus, k, **kw).output_token_ids,
                       _torch_topk_topp_accept(*args))
    passes = 1 + (2 if top_k else 0) + (1 if (top_k or top_p) else 0) + (1 if top_p else 0) + 1
    print(f"rejtopp B={B} k={k} V={V} top_k={top_k} top_p={top_p}: hip {hip:8.1f} us ({passes} passes, "
          f"{passes * B * k * V * 2 / 1e9 / hip * 1e6 / 1e3:5.2f} TB/s effective)   torch {ref:8.1f} us   "
          f"x{ref / hip:5.1f}   same tokens: {same}")


def _torch_sampler(logits, row_index, temp, k_rows, p_rows, q):
    """vLLM 0.9.2's Sampler for the same call, restated in torch on the same GPU: gather the rows, f32 copy, div_ by the
    temperature, apply_top_k_top_p in f32 (the full ascending sort when top-p is set, apply_top_k_only's topk form when
    only top-k is), softmax f32, div_(q), arg-max."""
    x = logits[row_index] if row_index is not None else logits
    x = x.float().div_(temp.unsqueeze(1))
    if p_rows is None and k_rows is not None:
        no_k = k_rows == x.shape[1]
        kk = k_rows.masked_fill(no_k, 1)
        thr = x.topk(int(kk.max()), dim=1).values.gather(1, (kk - 1).unsqueeze(1))
        thr.masked_fill_(no_k.unsqueeze(1), -float("inf"))
        x.masked_fill_(x < thr, -float("inf"))
    elif p_rows is not None:
        xs, xi = x.sort(dim=-1, descending=False)
        if k_rows is not None:
            xs.masked_fill_(xs < xs.gather(1, (xs.size(1) - k_rows).unsqueeze(1)), -float("inf"))
        m = xs.softmax(dim=-1).cumsum(dim=-1) <= (1 - p_rows).unsqueeze(1)
        m[:, -1] = False
        xs.masked_fill_(m, -float("inf"))
        x = xs.scatter(-1, xi, xs)
    return x.softmax(dim=-1, dtype=torch.float32).div_(q).argmax(dim=-1).to(torch.int32)


def sample(B=64, V=128256, top_k=None, top_p=None, indexed=False, reps=3):
    """aic_sample_topk_topp (ops.sample_tokens) against the torch restatement of vLLM's sampler: same GPU, same inputs,
    the two timed alternately `reps` times.  `indexed`: the rows are read through row_index out of a [256, V] matrix
    (the bonus rows of a verify step) instead of from a gathered [B, V] one."""
    g = torch.Generator(device=dev).manual_seed(0)
    T = 256 if indexed else B
    logits = (torch.randn(T, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    idx = (torch.arange(B, device=dev) * (T // B) + (T // B - 1)).to(torch.int64) if indexed else None
    temp = torch.full((B,), 0.6, device=dev)
    q = torch.empty(B, V, device=dev).exponential_(generator=g)
    tk = None if top_k is None else torch.full((B,), top_k, dtype=torch.int32, device=dev)
    tp = None if top_p is None else torch.full((B,), top_p, dtype=torch.float32, device=dev)
    hip_fn = lambda: ops.sample_tokens(logits, temp, q, top_k=tk, top_p=tp, row_index=idx)
    ref_fn = lambda: _torch_sampler(logits, idx, temp, None if tk is None else tk.long(), tp, q)
    hip, ref = [], []
    for _ in range(reps):
        hip.append(timeit(hip_fn))
        ref.append(timeit(ref_fn))
    same = torch.equal(hip_fn(), ref_fn())
    passes = 1 + (4 if top_k else 0) + (1 if (top_k or top_p) else 0) + (3 if top_p else 0) + 1
    fmt = lambda v: " / ".join(f"{x:7.1f}" for x in v)
    print(f"sample B={B} V={V} top_k={top_k} top_p={top_p} {'row_index' if indexed else 'gathered '}: hip {fmt(hip)} us "
          f"({passes:2d} passes, {passes * B * V * 2 / 1e9 / min(hip) * 1e6 / 1e3:5.2f} TB/s effective)   torch {fmt(ref)} us   "
          f"x{min(ref) / max(hip):5.1f} (fastest torch / slowest hip)   same tokens: {same}", flush=True)


def _torch_logprobs(logits, idx, tokens, n):
    """vLLM 0.9.2's Sampler.compute_logprobs + gather_logprobs on the rows `idx` of `logits` (recalled)."""
    x = logits if idx is None else logits[idx]
    lp = x.log_softmax(dim=-1, dtype=torch.float32)
    tok = tokens.long().unsqueeze(-1)
    tlp = lp.gather(-1, tok)
    ranks = (lp >= tlp).sum(-1)
    if n == 0:
        return tok.to(torch.int32), tlp, ranks
    tv, ti = torch.topk(lp, n, dim=-1)
    return torch.cat((tok, ti), dim=1).to(torch.int32), torch.cat((tlp, tv), dim=1), ranks


def logprobs(B=64, V=128256, n=20, indexed=False, reps=3):
    """aic_token_logprobs (ops.token_logprobs) against the torch restatement of vLLM's two functions: same GPU, same
    inputs, the two timed alternately `reps` times.  `indexed`: the rows are read through row_index out of a [256, V]
    matrix (the bonus rows of a verify step) instead of from a gathered [B, V] one."""
    g = torch.Generator(device=dev).manual_seed(0)
    T = 256 if indexed else B
    logits = (torch.randn(T, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    idx = (torch.arange(B, device=dev) * (T // B) + (T // B - 1)).to(torch.int64) if indexed else None
    tokens = torch.randint(0, V, (B,), device=dev, generator=g).to(torch.int32)
    hip_fn = lambda: ops.token_logprobs(logits, n, token_ids=tokens, row_index=idx, check_token_ids=False)
    ref_fn = lambda: _torch_logprobs(logits, idx, tokens, n)
    hip, ref = [], []
    for _ in range(reps):
        hip.append(timeit(hip_fn))
        ref.append(timeit(ref_fn))
    a, b = hip_fn(), ref_fn()
    # random bf16 rows tie inside their top n: the ids of tied entries are torch.topk's choice, the values are not
    same = (torch.equal(a[0][:, 0], b[0][:, 0]) and torch.equal(a[2], b[2])
            and bool(((a[1] - b[1]).abs() <= 1e-5 + 2.0 ** -20 * b[1].abs()).all()))
    passes = 2 + (1 if n else 0)          # bf16 keys: first, digit 1 (+ sum and rank), gather
    fmt = lambda v: " / ".join(f"{x:7.1f}" for x in v)
    print(f"logprobs B={B} V={V} n={n:2d} {'row_index' if indexed else 'gathered '}: hip {fmt(hip)} us "
          f"({passes} passes, {passes * B * V * 2 / 1e9 / min(hip) * 1e6 / 1e3:5.2f} TB/s effective)   torch {fmt(ref)} us   "
          f"x{min(ref) / max(hip):5.1f} (fastest torch / slowest hip)   same values and ranks: {same}", flush=True)


def _torch_bin_counts(tokens, V):
    """get_token_bin_counts_and_mask (vllm/model_executor/layers/utils.py, recalled): an int64 [B, V + 1] scatter-add."""
    counts = torch.zeros((tokens.shape[0], V + 1), dtype=torch.long, device=tokens.device)
    counts.scatter_add_(1, tokens, torch.ones_like(tokens))
    counts = counts[:, :V]
    return counts, counts > 0


def _torch_edits(logits, mask, ban, bias, prompt, output, rep, freq, pres, min_p, temp):
    """vLLM 0.9.2's path for the same step, restated in torch on the same GPU: the f32 copy, masked_fill_ of the allowed
    mask, the index puts of bad words / min_tokens and of the bias (their index tensors are built outside the timed
    region, vLLM builds them from Python lists every step), apply_penalties with its two bin-count matrices, and
    apply_min_p on the softmax of the tempered rows (that division is the sampler's own in vLLM: it is counted here)."""
    x = logits.float()
    if mask is not None:
        x.masked_fill_(mask, -float("inf"))
    if ban is not None:
        x[ban] = -float("inf")
    if bias is not None:
        x[bias[0], bias[1]] += bias[2]
    if rep is not None:
        V = x.shape[1]
        _, prompt_mask = _torch_bin_counts(prompt, V)
        out_counts, out_mask = _torch_bin_counts(output, V)
        penalties = torch.where(prompt_mask | out_mask, rep.unsqueeze(1), 1.0)
        x *= torch.where(x > 0, 1.0 / penalties, penalties)
        x -= freq.unsqueeze(1) * out_counts
        x -= pres.unsqueeze(1) * out_mask
    if min_p is not None:
        probs = torch.softmax(x / temp.unsqueeze(1), dim=-1)
        x.masked_fill_(probs < min_p.unsqueeze(1) * probs.amax(dim=-1, keepdim=True), -float("inf"))
    return x


def edits(B=64, V=128256, case="all", n_prompt=4096, n_output=256, reps=3):
    """aic_logits_edit (ops.edit_logits) against the torch restatement of vLLM's logits edits: same GPU, same inputs, the
    two timed alternately `reps` times.  bf16 rows, histories of `n_prompt` + `n_output` tokens per row, 4 banned and 4
    biased tokens per row, a 10 % allowed-token mask, min-p 0.1 at T = 0.8."""
    g = torch.Generator(device=dev).manual_seed(0)
    logits = (torch.randn(B, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    on = lambda name: case in (name, "all")
    mask = (torch.rand(B, V, device=dev, generator=g) < 0.1) if on("mask") else None
    rows4 = torch.arange(B, device=dev).repeat_interleave(4)
    off4 = (torch.arange(B + 1, device=dev) * 4).to(torch.int32)
    ban_tok = torch.randint(0, V, (B * 4,), device=dev, generator=g)
    bias_tok = (torch.arange(B * 4, device=dev) * 7919) % V              # distinct within a row, as dict keys are
    bias_val = torch.randn(B * 4, device=dev, generator=g)
    prompt = torch.randint(0, V, (B, n_prompt), device=dev, generator=g)
    prompt[:, -64:] = V                                                   # padding
    output = torch.randint(0, V // 64, (B, n_output), device=dev, generator=g)      # repeats: counts above 1
    off = lambda n: (torch.arange(B + 1, device=dev) * n).to(torch.int32)
    f = lambda v: torch.full((B,), v, device=dev)
    rep, freq, pres = (f(1.2), f(0.3), f(0.1)) if on("penalties") else (None, None, None)
    min_p, temp = (f(0.1), f(0.8)) if on("min_p") else (None, None)
    kw = dict(allowed_mask=mask, repetition=rep, frequency=freq, presence=pres, min_p=min_p, temperature=temp)
    if on("ban"):
        kw["ban"] = (off4, ban_tok.to(torch.int32))
    if on("bias"):
        kw["bias"] = (off4, bias_tok.to(torch.int32), bias_val)
    if on("penalties"):
        kw.update(prompt=(off(n_prompt), prompt.to(torch.int32).reshape(-1)), output=(off(n_output), output.to(torch.int32).reshape(-1)))
    hip_fn = lambda: ops.edit_logits(logits, **kw)
    ref_fn = lambda: _torch_edits(logits, mask, (rows4, ban_tok) if on("ban") else None,
                                  (rows4, bias_tok, bias_val) if on("bias") else None, prompt, output, rep, freq, pres,
                                  min_p, temp)
    hip, ref = [], []
    for _ in range(reps):
        hip.append(timeit(hip_fn))
        ref.append(timeit(ref_fn))
    a, b = hip_fn(), ref_fn()
    differ = int(((a != b) & ~(a.isnan() & b.isnan())).sum())
    # HBM bytes of the HIP call: the 16-bit rows in, the f32 rows out, the mask, and min-p's second pass over the f32 rows
    nbytes = B * V * (2 + 4 + (1 if on("mask") else 0) + (4 if on("min_p") else 0))
    fmt = lambda v: " / ".join(f"{x:7.1f}" for x in v)
    print(f"edits B={B} V={V} {case:9s}: hip {fmt(hip)} us ({nbytes / 1e6:6.1f} MB, {nbytes / 1e6 / min(hip):5.2f} TB/s)   "
          f"torch {fmt(ref)} us   x{min(ref) / max(hip):5.1f} (fastest torch / slowest hip)   "
          f"differing entries: {differ} of {B * V}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["attn", "lstm", "rej"]
    if "edits" in what:
        for V in (128256, 201088):
            for case in ("mask", "ban", "bias", "penalties", "min_p", "all"):
                edits(V=V, case=case)
    if "logprobs" in what:
        for V in (128256, 201088):
            for indexed in (False, True):
                for n in (0, 1, 20):
                    logprobs(V=V, n=n, indexed=indexed)
    if "sample" in what:
        for V in (128256, 201088):
            for indexed in (False, True):
                sample(V=V, indexed=indexed)                 # temperature only
                sample(V=V, top_p=0.9, indexed=indexed)
                sample(V=V, top_k=50, indexed=indexed)
                sample(V=V, top_k=50, top_p=0.9, indexed=indexed)
    if "rejtopp" in what:
        for V in (128256, 201088):
            rejection_topk_topp(V=V)                         # temperature only (aic_rejection_random)
            rejection_topk_topp(V=V, top_p=0.9)
            rejection_topk_topp(V=V, top_k=50)
            rejection_topk_topp(V=V, top_k=50, top_p=0.9)
    if "attn" in what:
        attn(split=True)
        attn()
        attn(B=32)
        attn(B=8)
        attn(B=64, Hq=4, Hkv=1)        # SP=8 slice
        attn(B=64, qlen=8)
        attn(B=16, qlen=33, split=True)
        attn(B=4, qlen=33, split=True)
        attn(B=1, qlen=33, split=True)
        attn(B=64, Hq=64, Hkv=8, D=64)           # gpt-oss-120b heads (secondary head size: shared-tile body for all)
        attn(B=64, Hq=8, Hkv=1, D=64)            # its SP = 8 slice
    if "fp8" in what or "attn" in what:
        attn(split=True, kv8=True)
        attn(B=16, qlen=33, split=True, kv8=True)
    if "attn16" in what:     # attn's shapes for a bf16 and an fp16 model, alternating in this process (a mode of its own:
        #                      `attn` is a stage of collect_profiles.sh and keeps its length)
        attn_dtypes(split=True)
        attn_dtypes()
        attn_dtypes(B=32)
        attn_dtypes(B=8)
        attn_dtypes(B=64, Hq=4, Hkv=1)
        attn_dtypes(B=64, qlen=8)
        attn_dtypes(B=16, qlen=33, split=True)
        attn_dtypes(B=4, qlen=33, split=True)
        attn_dtypes(B=1, qlen=33, split=True)
        attn_dtypes(B=64, Hq=64, Hkv=8, D=64)
        attn_dtypes(B=64, Hq=8, Hkv=1, D=64)
        attn_dtypes(split=True, kv8=True)
        attn_dtypes(B=16, qlen=33, split=True, kv8=True)
        attn_dtypes(n_short=59, n_long=5, ctx=4224)          # attn_mix's step: the one-grid short + long launch
    if "prefix" in what:     # a step's shared prompt prefix read once (cascade) against the plain call, alternating
        for kv8 in (False, True):
            for P in (256, 1024, 2048):
                attn_prefix(B=64, P=P, kv8=kv8)
            for B in (8, 32):
                attn_prefix(B=B, P=2048, kv8=kv8)
        attn_prefix(B=64, P=2048, Hq=4, Hkv=1)           # SP = 8 slice
        attn_prefix(B=64, P=2048, qlen=1)                # a step without drafts
        for B, P in ((8, 256), (16, 256), (8, 1024)):    # towards the break-even
            attn_prefix(B=B, P=P)
    if "tree" in what:       # tree-shaped drafts: the tree call against the plain call, acceptance and compaction launches
        for kv8 in (False, True):
            for n_draft in (3, 8):
                attn_tree(B=64, n_draft=n_draft, kv8=kv8)
        for kv8 in (False, True):
            for n_draft in (16, 32):
                attn_tree(B=16, n_draft=n_draft, kv8=kv8, tree=True)
        attn_tree(B=64, n_draft=32, tree=True)
        for n_draft in (8, 32):
            tree_accept_compact(B=64, n_draft=n_draft)
        tree_accept_compact(B=64, n_draft=32, kv8=True)
    if "prefixgroups" in what:   # prefixes shared per GROUP of requests, read once per group, against the plain call
        for kv8 in (False, True):
            attn_prefix_groups([64], 2048, kv8=kv8, single=True)
            for members in (32, 16, 8, 4):
                attn_prefix_groups([members] * (64 // members), 2048, kv8=kv8)
            attn_prefix_groups([24, 24], 2048, loners=16, kv8=kv8)
            attn_prefix_groups([32, 32], [1024, 3072], kv8=kv8)
            # what decides beside the group size: the longest range left to ONE request behind its prefix, against the
            # longest context (the suffix launch lasts as long as its longest request)
            attn_prefix_groups([32, 32], [2048, 3072], kv8=kv8)
            attn_prefix_groups([32, 32], [1536, 2560], kv8=kv8)
            attn_prefix_groups([31, 31], 2048, loners=2, kv8=kv8)
    if "prefixsplits" in what:   # split count of the prefix launch, forced (aic_debug_attn_prefix_splits)
        for kv8 in (False, True):
            for sp in (0, 1, 2, 4, 8, 16):
                N.lib().aic_debug_attn_prefix_splits(sp)
                print("prefix splits %2d: " % sp, end="")
                attn_prefix(B=64, P=2048, kv8=kv8)
        N.lib().aic_debug_attn_prefix_splits(0)
    if "long" in what:
        attn(B=16, qlen=33, split=True)
        attn(B=16, qlen=17, split=True)
        attn(B=5, qlen=33, split=True)
        attn(B=1, qlen=33, split=True)
    if "layout" in what:     # the short body's layouts (heads per workgroup x cross-workgroup splits), forced one by one
        for B, combos in ((64, ((0, 0), (4, 2), (2, 1), (2, 2), (1, 1))), (32, ((0, 0), (4, 4), (2, 2), (2, 1), (1, 1), (1, 2))),
                          (16, ((0, 0), (4, 8), (2, 4), (1, 2), (1, 1)))):
            for hpw, sp in combos:
                N.lib().aic_debug_attn_layout(hpw, sp)
                print(f"layout hpw={hpw} splits={sp}: ", end="")
                attn_mix(B, 0)
        for hpw, sp in ((0, 0), (4, 2), (2, 1), (1, 1)):
            N.lib().aic_debug_attn_layout(hpw, sp)
            print(f"layout hpw={hpw} splits={sp}: ", end="")
            attn_mix(59, 5)
        for hpw in (2, 1):          # two kv heads per rank (an 8-kv-head model under SP = 4)
            N.lib().aic_debug_attn_layout(hpw, 0)
            print(f"layout hpw={hpw} splits=auto: ", end="")
            attn_mix(64, 0, Hq=8, Hkv=2)
        N.lib().aic_debug_attn_layout(0, 0)
    if "fp8layout" in what:   # the fp8 short body is issue-bound, not HBM-bound: does a second workgroup per CU pay there?
        attn_mix(64, 0, kv8=True)       # (first case of a process: clocks still ramping)
        for B, combos in ((64, ((0, 0), (4, 2), (4, 4), (4, 8))), (32, ((0, 0), (4, 4), (4, 8), (4, 16))), (16, ((0, 0), (4, 16)))):
            for hpw, sp in combos:
                N.lib().aic_debug_attn_layout(hpw, sp)
                print(f"fp8 layout hpw={hpw} splits={sp}: ", end="")
                attn_mix(B, 0, kv8=True)
        N.lib().aic_debug_attn_layout(0, 0)
    if "longdma" in what:     # who issues the tile DMA in a long-draft workgroup (aic_debug_attn_long_dma)
        for pat in (0, 1, 2, 3):
            N.lib().aic_debug_attn_long_dma(pat)
            print(f"-- long_dma pattern {pat}")
            for B, q in ((16, 33), (16, 20), (16, 24), (32, 12), (16, 6)):
                attn(B=B, ctx=4096, qlen=q, split=True)
            attn_mix(31, 1, q_long=33)
            attn_mix(28, 4, q_long=20)
        N.lib().aic_debug_attn_long_dma(1)
    if "mixphases" in what:   # the same account for the long workgroups of mixed calls (one lane of the bench)
        attn_long_phases(1, 33, 4224, n_short=31)
        attn_long_phases(1, 10, 4224, n_short=31)
        attn_long_phases(4, 20, 4224, n_short=28)
    if "longphases" in what:  # cycle accounting of the long-draft body
        attn_long_phases(16, 33)
        attn_long_phases(16, 20)
        attn_long_phases(32, 12)
    if "phases" in what:      # in-kernel phase trace of the short body: where the per-call fixed cost sits
        for kv8 in (False, True):
            for n in (32, 64):
                attn_phases(n, 4224, kv8)
            attn_phases(32, 1056, kv8)
    if "ctxsweep" in what:    # short body over the context length: slope = streaming rate, intercept = fixed cost per call
        for kv8 in (False, True):
            for n in (32, 64):
                for ctx in (544, 1056, 2112, 4224, 8448):
                    attn_mix(n, 0, 1, 33, ctx=ctx, kv8=kv8)
    if "longctx" in what:     # the long-draft body alone over the context length: fixed cost and slope per 32-token tile
        for B in (16, 1):
            for ctx in (128, 512, 1024, 2048, 4096):
                attn(B=B, ctx=ctx, qlen=33, split=True)
        for ctx in (128, 1024, 4096):
            attn(B=16, ctx=ctx, qlen=12, split=True)
    if "manylong" in what:    # a 32-request lane in which suffix decoding hit for many requests (one-grid form out of room)
        for ns, nl, qlong in ((31, 1, 33), (28, 4, 20), (25, 7, 20), (22, 10, 20), (19, 13, 20), (17, 15, 20), (17, 15, 33), (12, 20, 12),
                              (4, 28, 12), (0, 32, 12)):
            for mode, name in ((0, "one grid   "), (1, "two launches"), (-1, "library    ")):
                N.lib().aic_debug_attn_sequential(mode)
                print(name, end=" ")
                attn_mix(ns, nl, q_long=qlong)
        N.lib().aic_debug_attn_sequential(-1)
    if "fp8mix" in what:      # a 32-request lane with long drafts, fp8 cache against bf16
        attn_mix(32, 0, kv8=True)
        for kv8 in (True, False):
            for ns, nl, qlong in ((32, 0, 33), (31, 1, 33), (30, 2, 33), (30, 2, 12), (28, 4, 20), (0, 1, 33), (0, 2, 33)):
                attn_mix(ns, nl, q_long=qlong, kv8=kv8)
    if "pmc" in what:      # the cases whose kernels tools/pmc_kernels.py tells apart by name (few iterations: counters, not time)
        _t = timeit
        timeit = lambda fn, iters=4, warm=1: _t(fn, iters=4, warm=1)
        attn(split=True)                               # verify_attn_kernel<1, true, false, 4>: the bf16 short body (baseline)
        attn(split=True, kv8=True)                     # <1, true, true, 4>: fp8 short body
        attn(B=64, Hq=4, Hkv=1, split=True)            # <1, false, false, 4>: SP = 8 slice, waves = token ranges
        attn(B=16, qlen=33, split=True)                # verify_attn_long4_kernel<false, 128>: long drafts alone
        attn(B=16, qlen=33, split=True, kv8=True)      # verify_attn_long4_kernel<true, 128>
        attn(B=64, Hq=64, Hkv=8, D=64)                 # verify_attn_long4_kernel<false, 64>: head size 64
        timeit = _t
    if "mid" in what:      # suffix drafts of 4-7 tokens (17-32 query rows): two row tiles of the short body since r02
        attn_mix(64, 0)
        attn_mix(59, 5, q_long=8)
        attn_mix(59, 5, q_long=5)
        attn_mix(59, 5, q_long=9)
        attn_mix(59, 5, q_long=33)
        attn_mix(57, 7, q_long=8)
        attn_mix(30, 2, q_long=8)
        attn_mix(30, 2, q_long=33)
        attn_mix(59, 5, q_long=8, Hq=4, Hkv=1)
        attn_mix(59, 5, q_long=33, Hq=4, Hkv=1)
        attn_mix(64, 0, q_short=8)         # every request at two row tiles
        attn_mix(64, 0, q_short=4)
    if "light" in what:    # weight of the short-body splits that share CUs with long-draft workgroups (percent; 100 = equal)
        for pct in (100, 96, 92, 88, 84):
            N.lib().aic_debug_attn_light(pct)
            print("light", pct)
            attn_ql([1] * 31 + [33], jitter=256)
            attn_ql([1] * 30 + [20, 33], jitter=256)
            attn_ql([1] * 29 + [10, 20, 33], jitter=256)
            attn_ql([1] * 63 + [33], jitter=256)
            attn_ql([1] * 62 + [20] * 2, jitter=256)
            attn_ql([1] * 59 + [33] * 5, jitter=256)
            attn_ql([1] * 59 + [12] * 3 + [33] * 2, Hq=4, Hkv=1, jitter=256)
        N.lib().aic_debug_attn_light(0)
    if "ql" in what:
        for jit in (0, 256):
            attn_ql([1] * 64, jitter=jit)
            attn_ql([1] * 59 + [6] * 3 + [20] * 2, jitter=jit)
            attn_ql([1] * 59 + [8] * 3 + [33] * 2, jitter=jit)
            attn_ql([1] * 61 + [6] * 3, jitter=jit)
            attn_ql([1] * 62 + [20] * 2, jitter=jit)
            attn_ql([1] * 63 + [33], jitter=jit)
            attn_ql([1] * 58 + [5, 7, 8, 10, 20, 33], jitter=jit)
    if "trace32" in what:      # one lane of the bench: 32 requests, a few long drafts
        attn_trace(31, 1)
        attn_trace(28, 4, q_long=20)
        attn_trace(27, 5)
    if "trace" in what:
        attn_trace(59, 5)
        attn_trace(56, 8)
        attn_trace(62, 2)
        attn_trace(63, 1)
        attn_trace(30, 2)
        attn_trace(31, 1)
    if "sptrace" in what:        # the SP = 8 slice: which workgroups end the one-grid launch, by long split count
        for sp in (24, 32):
            N.lib().aic_debug_attn_long_splits(sp)
            print("long splits", sp)
            attn_trace(63, 1, Hq=4, Hkv=1)
            attn_trace(31, 1, Hq=4, Hkv=1)
        N.lib().aic_debug_attn_long_splits(0)
        attn_mix(64, 0, Hq=4, Hkv=1)
        attn_mix(32, 0, Hq=4, Hkv=1)
    if "mix" in what:
        attn_mix(64, 0)
        attn_mix(59, 5)
        attn_mix(59, 0)
        attn_mix(0, 5)
        attn_mix(56, 8)
        attn_mix(59, 5, q_long=17)
        attn_mix(59, 5, q_short=4)
        attn_mix(59, 5, kv8=True)
        attn_mix(8, 1, Hq=4, Hkv=1)      # SP = 8 slice
        attn_mix(59, 5, Hq=4, Hkv=1)
    if "mixdma" in what:        # DMA duty pattern of the long part of mixed calls
        for pat in (0, 1, 2):
            N.lib().aic_debug_attn_long_dma(pat)
            print(f"-- long_dma pattern {pat}")
            for ns, nl, ql in ((31, 1, 10), (30, 2, 10), (31, 1, 20), (31, 1, 33), (30, 2, 33), (28, 4, 20), (27, 5, 33)):
                attn_mix(ns, nl, q_long=ql)
        N.lib().aic_debug_attn_long_dma(1)
    if "mixes" in what:         # the bench's common lane mixes under the library's own rules
        attn(B=32, ctx=4224, qlen=1, split=True)
        for ns, nl, ql in ((31, 1, 10), (30, 2, 10), (31, 1, 20), (30, 2, 20), (31, 1, 33), (30, 2, 33), (28, 4, 20), (27, 5, 33), (25, 7, 20)):
            attn_mix(ns, nl, q_long=ql)
    if "longsplits8" in what:   # the same at full width (8 kv heads: one GPU), after the r04 long-body changes
        L = N.lib()
        for ns, nl, ql in ((31, 1, 10), (30, 2, 10), (31, 1, 20), (30, 2, 20), (31, 1, 33), (30, 2, 33), (28, 4, 20), (27, 5, 33), (25, 7, 20)):
            for sp in (0, 2, 3, 4, 5, 6, 8, 10):
                L.aic_debug_attn_long_splits(sp)
                print("long splits %2d: " % sp, end="")
                attn_mix(ns, nl, q_long=ql)
        L.aic_debug_attn_long_splits(0)
    if "longsplits" in what:
        # long-draft split count of a mixed call on the slices a rank sees under SP (kv heads per rank 8 / 4 / 2 / 1)
        L = N.lib()
        for Hkv in (4, 2, 1):
            for ns, nl in ((63, 1), (61, 3), (59, 5), (31, 1), (30, 2), (15, 1)):
                for sp in (0, 12, 16, 20, 24, 32):
                    L.aic_debug_attn_long_splits(sp)
                    print("long splits %2d: " % sp, end="")
                    attn_mix(ns, nl, Hq=4 * Hkv, Hkv=Hkv)
        L.aic_debug_attn_long_splits(0)
    if "splight" in what:       # lighter trailing splits on SP slices, where the long workgroups are many and short
        for Hkv in (1, 2, 4):
            for ns, nl in ((63, 1), (61, 3), (59, 5), (31, 1), (29, 3)):
                for pct in (100, 94, 0):
                    N.lib().aic_debug_attn_light(pct)
                    print("light %3d: " % pct, end="")
                    attn_mix(ns, nl, Hq=4 * Hkv, Hkv=Hkv)
        N.lib().aic_debug_attn_light(0)
    if "spsplits" in what:      # short-part split count on SP slices (aic_debug_attn_layout: heads per workgroup, splits)
        for Hkv, hpws in ((1, (1,)), (2, (2, 1)), (4, (4, 2))):
            for ns, nl in ((64, 0), (63, 1), (32, 0), (31, 1)):
                for hpw in hpws:
                    for sp in (0, 2, 3, 4, 6, 8, 12, 16):
                        N.lib().aic_debug_attn_layout(hpw if sp else 0, sp)
                        print("hpw %d splits %2d: " % (hpw, sp), end="")
                        attn_mix(ns, nl, Hq=4 * Hkv, Hkv=Hkv)
        N.lib().aic_debug_attn_layout(0, 0)
    if "prefill" in what:       # aic_step_attention: prefill chunks, the SP = 8 slice, a mixed step
        prefill_suite()
    if "lstm" in what:
        lstm(64)
        lstm(32)
        lstm(8)
    if "lstm" in what or "lstm_wide" in what:
        lstm_wide()
    if "rej" in what:
        rejection()
