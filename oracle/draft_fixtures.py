"""ORACLE — test infrastructure only (never imported by the product package).

Margin-planted draft-model fixtures.  Random draft checkpoints put nearly every (row, head) of a large vocabulary at a
near-tie, so a test can only demand "the kernel's token, or one within a bf16 step of the top".  Here the LM-head rows
at chosen target tokens are overwritten so that each target wins by a wide margin on the oracle's own states, and a test
can demand the oracle's tokens exactly (`torch.equal`).

build_fixture(family, ck, ids, hidden, k, ...):
  1. chooses targets t[b, h], distinct over every (row, head) pair that reads the same LM-head matrix (`head.0` for the
     LSTM and tied MLP / sum_rnn models, `head.{h}` per head for untied ones), index edges included: 0 and V - 1, both
     sides of 64-row block boundaries, rows of a partly valid last block and, with `tp` > 1, the first and last real row
     of every vocab shard;
  2. runs the oracle teacher-forced with the expected tokens and takes the state every head's LM head reads;
  3. plants the target rows: row j of the dual basis (pseudo-inverse) of that matrix's states, scaled, so a planted row
     scores high on its own state and ~0 on the others (the background rows stay random);
  4. re-runs the oracle free and asserts that it returns exactly the expected tokens, every one at least
     `margin_steps` bf16 steps (of the larger magnitude) above the runner-up.  With `fp8` this is the oracle's own fp8
     path (planting moves the per-tensor weight scale); the fp8 states (dequantised activations) are what is planted on.

Variants:
  * "exact"     : the above;
  * "negative"  : every real logit of every (row, head) is below zero (a shared direction u with u . s = 1 on every
                  state is subtracted from every real row); the target is the least negative by the same margin, so a
                  zero-filled padded column would win if a kernel failed to mask it;
  * "exact_tie" : for chosen (b, h) the target row is copied bit for bit to a second index (another 64-row block, or
                  the same block at 1 / 4 / 16 rows for the GEMM epilogue's levels, or the neighbouring vocab shard with
                  `tp` > 1), above or below the target; the expected token is the lower index and the margin is taken to
                  the third-best;
  * "bf16_tie"  : (bf16 head) a companion row at a higher index whose pre-rounding logit is LARGER than the target's
                  while both round to the same bf16 value, each at least 1/8 bf16 step clear of the rounding edges: the
                  expected token is the target; a kernel that compares before rounding returns the companion.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from oracle import spec_oracle as O

BLOCK = 64            # rows per workgroup of the head GEMM (kRowsPerBlock)
VARIANTS = ("exact", "negative", "exact_tie", "bf16_tie")


def bf16_step(x: float) -> float:
    """Distance between adjacent bf16 values at magnitude |x| (8 significant bits)."""
    a = abs(float(x))
    if a == 0.0:
        return 2.0 ** -133
    _, e = math.frexp(a)            # a = m 2^e, m in [0.5, 1)
    return math.ldexp(1.0, e - 8)


def shard_bounds(V: int, tp: int) -> List[Tuple[int, int]]:
    """[start, end) of the real rows of every vocab shard (speculator.py: padded to 64, split evenly)."""
    padded = (V + BLOCK - 1) // BLOCK * BLOCK
    size = padded // tp
    return [(r * size, min(V, (r + 1) * size)) for r in range(tp)]


def edge_targets(V: int, tp: int = 1) -> List[int]:
    """Index edges of the head GEMM and of the vocab shards, most important first."""
    e = [0, V - 1, BLOCK - 1, BLOCK]
    last = (V - 1) // BLOCK * BLOCK                  # first row of the last (maybe partly valid) block
    e += [last - 1, last, V - 2]
    mid = V // 2 // BLOCK * BLOCK
    e += [mid - 1, mid]
    for s, t in shard_bounds(V, tp):
        e += [s, t - 1]
    out = []
    for x in e:
        if 0 <= x < V and x not in out:
            out.append(x)
    return out


@dataclass
class DraftFixture:
    ckpt: Dict[str, torch.Tensor]          # the checkpoint, planted (same names as the input)
    tokens: torch.Tensor                   # [B, k] int64: what the free oracle returns
    logits: List[torch.Tensor]             # per head [B, V] bf16: the free oracle's logits
    head_keys: List[str]                   # LM-head matrix read by head h
    edges: List[int] = field(default_factory=list)
    ties: List[Tuple[int, int, int, int]] = field(default_factory=list)      # (b, h, lower, upper): bitwise twin rows
    bf16_pairs: List[Tuple[int, int, int, int, float, float]] = field(default_factory=list)
    # ^ (b, h, target, companion, f64 logit of the target, f64 logit of the companion), companion > target
    states: List[torch.Tensor] = field(default_factory=list)      # per head [B, Ds] f64: what the head's GEMM reads

    def value(self, b: int, h: int) -> float:
        return float(self.logits[h][b, int(self.tokens[b, h])])


def run_oracle(family: str, ck, ids, hidden, k: int, *, fp8: bool, n_predict: int, scale_input: bool, tie: bool = True,
               stacks=(0, 0, 0), forced=None, states: bool = False):
    """(tokens, logits[, states]) of the op-sequence oracle on a checkpoint with the reference's names."""
    if family == "lstm":
        return O.lstm_generate_proposals(O.merge_lstm_checkpoint(ck), ids, hidden, k, n_predict, scale_input, fp8_head=fp8,
                                         return_logits=True, forced_tokens=forced, return_states=states)
    Ds = ck["ln.0.weight"].numel()
    return O.mlp_generate_proposals(ck, ids, hidden, k, n_predict, Ds, tie, scale_input, fp8_head=fp8, return_logits=True,
                                    forced_tokens=forced, stacks=tuple(stacks), return_states=states)


def head_keys(family: str, k: int, tie: bool) -> List[str]:
    if family == "lstm" or tie:
        return ["head.0.weight"] * k
    return [f"head.{h}.weight" for h in range(k)]


def _tie_offsets(V: int, tp: int) -> List[int]:
    """Row distances between tie partners: other blocks (neighbouring lane, other wave and same thread of the arg-max
    reductions over the per-block partials), then inside one block (same lane, lane shuffle, other wave of the epilogue)."""
    n_full = V // BLOCK
    out = [BLOCK, BLOCK * BLOCK, 1, BLOCK * 256, 4, BLOCK * 3, 16, BLOCK * 2]
    return [d for d in out if d < n_full * BLOCK - BLOCK] or [1]


def _plan(V: int, B: int, k: int, keys: List[str], variant: str, tp: int, g: torch.Generator):
    """expected[B, k], twin[(b, h)] -> (other index, side), edges used.  The expected token of a tie pair is its lower
    index; the companion of a bf16 pair sits above its target."""
    expected = torch.full((B, k), -1, dtype=torch.int64)
    pairs: Dict[Tuple[int, int], int] = {}
    used_edges: List[int] = []
    full_rows = V // BLOCK * BLOCK                   # tie partners stay inside full blocks
    bounds = shard_bounds(V, tp)
    for key in dict.fromkeys(keys):
        slots = [(b, h) for h in range(k) if keys[h] == key for b in range(B)]
        taken = set()

        def free(*xs):
            return all(0 <= x < V and x not in taken for x in xs)

        # 1. tie / companion pairs: every other (row, head) of the matrix, cycling through the placements
        if variant in ("exact_tie", "bf16_tie"):
            chosen = [s for i, s in enumerate(slots) if (s[0] + s[1]) % 2 == 0]
            cross = [(bounds[r][1] - 1, bounds[r + 1][0]) for r in range(tp - 1)]       # straddling two shards
            offs = _tie_offsets(V, tp)
            for n, (b, h) in enumerate(chosen):
                if n < len(cross):
                    lo, hi = cross[n]
                    side = "above"
                else:
                    d = offs[n % len(offs)]
                    side = "above" if n % 2 == 0 else "below"
                    for _ in range(1000):
                        t = int(torch.randint(0, full_rows, (1,), generator=g))
                        lo, hi = (t, t + d) if side == "above" else (t - d, t)
                        if hi < full_rows and free(lo, hi):
                            break
                    else:
                        raise RuntimeError("no room for a tie pair")
                if not free(lo, hi):
                    continue
                taken.update((lo, hi))
                expected[b, h] = lo                     # exact_tie: the lower twin; bf16_tie: the target
                pairs[(b, h)] = hi                      # its twin, or the companion above it
        # 2. index edges, then random rows
        rest = [s for s in slots if int(expected[s]) < 0]
        perm = torch.randperm(len(rest), generator=g).tolist()
        rest = [rest[i] for i in perm]
        edges = [e for e in edge_targets(V, tp) if e not in taken]
        for (b, h), e in zip(rest, edges):
            expected[b, h] = e
            taken.add(e)
            used_edges.append(e)
        for b, h in rest[len(edges):]:
            while True:
                t = int(torch.randint(0, V, (1,), generator=g))
                if t not in taken:
                    break
            expected[b, h] = t
            taken.add(t)
    return expected, pairs, used_edges


def _head_input(state: torch.Tensor, fp8: bool) -> torch.Tensor:
    """What the LM-head GEMM multiplies: the bf16 state, or its dequantised per-tensor e4m3 image."""
    if not fp8:
        return state.double()
    q, s = O.fp8_quant_per_tensor(state)
    return q.double() * float(s)


def _scaled_row(p: torch.Tensor, s: torch.Tensor, goal: float, tol: float) -> torch.Tensor:
    """bf16 row ~ goal * p whose exact logit against s is within `tol` of `goal`: bf16(goal * p), then single-ulp nudges of
    the element that brings the logit closest to the goal (small elements give fine steps) until it is within `tol`."""
    r = (goal * p).to(torch.bfloat16)
    sd = s.double()
    for _ in range(256):
        d = goal - float(r.double() @ sd)
        if abs(d) <= tol:
            return r
        bits = r.view(torch.int16)
        cand = []
        for step in (1, -1):
            nb = (bits + step).view(torch.bfloat16)
            ok = (r != 0) & torch.isfinite(nb) & (torch.sign(nb) == torch.sign(r))
            cand.append(torch.where(ok, (nb.double() - r.double()) * sd, torch.full_like(sd, math.inf)))
        c = torch.stack(cand)
        flat = int(torch.argmin((c - d).abs()))
        step, k = (1, -1)[flat // r.numel()], flat % r.numel()
        r = r.clone()
        r.view(torch.int16)[k] += step
    raise RuntimeError(f"could not place a logit within {tol} of {goal}")


def build_fixture(family: str, ck: Dict[str, torch.Tensor], ids: torch.Tensor, hidden: torch.Tensor, k: int, *,
                  fp8: bool = False, variant: str = "exact", tp: int = 1, n_predict: Optional[int] = None,
                  scale_input: bool = True, tie: bool = True, stacks=(0, 0, 0), seed: int = 0,
                  margin_steps: int = 16) -> DraftFixture:
    """`family` "lstm" (checkpoint names of random_lstm_weights) or "mlp" (random_mlp_weights' flat names, sum_rnn stacks
    included via `stacks`).  `tp` only steers the edge targets and the shard-straddling tie pairs; the oracle is the
    single-rank one.  Returns the planted checkpoint (the input is not modified), the expected tokens and the free
    oracle's logits; raises AssertionError if the free oracle does not reproduce the plan with the margin."""
    assert variant in VARIANTS, variant
    assert not (variant == "bf16_tie" and fp8), "bf16_tie is built for the bf16 head"
    n_predict = k if n_predict is None else n_predict
    keys = head_keys(family, k, tie)
    V, Ds = ck[keys[0]].shape
    B = ids.numel()
    g = torch.Generator().manual_seed(seed)
    kw = dict(fp8=fp8, n_predict=n_predict, scale_input=scale_input, tie=tie, stacks=stacks)
    expected, pairs, used_edges = _plan(V, B, k, keys, variant, tp, g)

    # 2. the states every head reads, teacher-forced on the expected tokens
    _, _, states = run_oracle(family, ck, ids, hidden, k, forced=expected, states=True, **kw)
    X = [_head_input(s, fp8) for s in states]

    # 3. plant
    out = dict(ck)
    bf16_pairs = []
    for key in dict.fromkeys(keys):
        W = ck[key].clone()
        slots = [(b, h) for h in range(k) if keys[h] == key for b in range(B)]
        S = torch.stack([X[h][b] for b, h in slots])                          # [n, Ds] f64
        P = torch.linalg.pinv(S)                                              # [Ds, n]: S @ P = I
        bg = (S.float() @ W.float().t())                                      # background logits
        bg_max = float(bg.abs().max())
        c = 1.5 * 2.0 ** math.ceil(math.log2(max(2.0 * bg_max, 1e-3)))       # mid-binade: no step change nearby
        for j, (b, h) in enumerate(slots):
            t = int(expected[b, h])
            if variant == "bf16_tie" and (b, h) in pairs:
                u = pairs[(b, h)]
                st = bf16_step(c)
                W[t] = _scaled_row(P[:, j], S[j], c - st / 4, st / 32)        # both inside the bucket around c,
                W[u] = _scaled_row(P[:, j], S[j], c + st / 4, st / 32)        # >= 1/8 step from either edge
                bf16_pairs.append((b, h, t, u))
                continue
            W[t] = (c * P[:, j]).to(torch.bfloat16)
            if variant == "exact_tie" and (b, h) in pairs:
                W[pairs[(b, h)]] = W[t]
        if variant == "negative":
            u = P.sum(dim=1)                                                  # u . s_j = 1 for every state
            top = (S.float() @ W.float().t())
            mask = torch.ones_like(top, dtype=torch.bool)
            for j, (b, h) in enumerate(slots):
                mask[j, int(expected[b, h])] = False
            runner = float(top[mask].max())                                   # best non-target logit over all states
            beta = c + (c - runner) / 4
            W = (W.double() - beta * u[None, :]).to(torch.bfloat16)
        out[key] = W

    # 4. verify on the free oracle
    toks, logits = run_oracle(family, out, ids, hidden, k, **kw)
    assert torch.equal(toks, expected), f"free oracle parted from the plan at {(toks != expected).nonzero().tolist()[:8]}"
    ties = []
    for (b, h), other in pairs.items():
        lo, hi = int(expected[b, h]), other
        if variant == "exact_tie":
            ties.append((b, h, lo, hi))
            assert torch.equal(logits[h][b, lo].view(torch.int16), logits[h][b, hi].view(torch.int16)), \
                ("tie logits differ", b, h, lo, hi, float(logits[h][b, lo]), float(logits[h][b, hi]))
    for n, (b, h, t, u) in enumerate(bf16_pairs):
        ft, fu = float(X[h][b] @ out[keys[h]][t].double()), float(X[h][b] @ out[keys[h]][u].double())
        bf16_pairs[n] = (b, h, t, u, ft, fu)
    for b in range(B):
        for h in range(k):
            lg = logits[h][b].float().clone()
            t = int(expected[b, h])
            top = float(lg[t])
            lg[t] = -math.inf
            if (b, h) in pairs:
                lg[pairs[(b, h)]] = -math.inf                                 # margin to the third-best
            second = float(lg.max())
            if variant == "negative":
                assert top < 0 and second < 0, (b, h, top, second)
            gap = top - second
            need = margin_steps * bf16_step(max(abs(top), abs(second)))
            assert gap >= need, f"margin at row {b} head {h}: {top} - {second} < {margin_steps} bf16 steps"
    return DraftFixture(ckpt=out, tokens=toks, logits=logits, head_keys=keys, edges=used_edges, ties=ties,
                        bf16_pairs=bf16_pairs, states=X)


def add_sum_rnn_stacks(ck: Dict[str, torch.Tensor], stacks, tie: bool, Ds: int, k: int, g: torch.Generator) -> None:
    """Random extra stages of a stacked sum_rnn checkpoint (flat names of mlp_generate_proposals' `stacks`), in place."""
    lin = lambda: (torch.randn(Ds, Ds, generator=g) * 0.06).to(torch.bfloat16)
    lnw = lambda: (1.0 + 0.1 * torch.randn(Ds, generator=g)).to(torch.bfloat16)
    lnb = lambda: (0.1 * torch.randn(Ds, generator=g)).to(torch.bfloat16)
    stages = lambda kind: (range(2) if kind == "proj" else range(1)) if tie else range(k)
    for kind, n in (("emb", stacks[0]), ("proj", stacks[1])):
        for i in stages(kind):
            for j in range(1, n + 1):
                ck[f"{kind}.{i}.{3 * j - 2}.weight"], ck[f"{kind}.{i}.{3 * j - 2}.bias"] = lnw(), lnb()
                ck[f"{kind}.{i}.{3 * j}.weight"] = lin()
    for i in stages("ln"):
        for j in range(1, stacks[2] + 1):
            ck[f"ln.{i}.{3 * j - 1}.weight"] = lin()
            ck[f"ln.{i}.{3 * j}.weight"], ck[f"ln.{i}.{3 * j}.bias"] = lnw(), lnb()


def lstm_fixture(V: int, Ds: int, H: int, B: int, *, fp8: bool = False, variant: str = "exact", tp: int = 1, k: int = 3,
                 seed: int = 0, std: float = 0.05, ck=None):
    """A sum_lstm speculator (n_predict = k, scale_input) with random weights, ids and hidden states, planted.
    Returns (config, fixture, ids, hidden)."""
    from arcticinference_amd.speculator import LSTMSpeculatorConfig, random_lstm_weights
    cfg = LSTMSpeculatorConfig(vocab_size=V, input_hidden_dim=H, inner_dim=str(Ds), emb_dim=str(Ds), proj_dim=str(Ds),
                               n_predict=k, num_lookahead_tokens=k)
    if ck is None:
        ck = random_lstm_weights(cfg, seed=seed, std=std)
    g = torch.Generator().manual_seed(1000 + seed * 131 + B)
    hidden = torch.randn(B, H, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, V, (B,), generator=g)
    fx = build_fixture("lstm", ck, ids, hidden, k, fp8=fp8, variant=variant, tp=tp, n_predict=k, scale_input=True,
                       seed=seed + B)
    return cfg, fx, ids, hidden
