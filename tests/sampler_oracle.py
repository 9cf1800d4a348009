"""CPU restatement of vLLM 0.9.2's Sampler for temperature / top-k / top-p (v1/sample/sampler.py and
v1/sample/ops/topk_topp_sampler.py: forward_native, random_sample; vLLM is not importable here, the rules are recalled),
and a fixture builder for aic_sample_topk_topp on top of sampling_oracle.build_row.

The sampler differs from the rejection sampler's compute_probs in one thing: it converts the logits to f32 FIRST and
divides by the temperature in f32, so x = f32(l) / T is never rounded to the logits dtype:
  greedy rows (T <= 0): arg-max of the raw row;
  x = logits.to(float32).div_(T); apply_top_k_top_p on the f32 rows (apply_top_k_only's topk form when only top-k is
  set); probs = softmax(x, f32); q ~ Exp(1); token = argmax(probs / q)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

import sampling_oracle as S

CUMSUM_MARGIN = 5e-3    # every ascending cumulative sum (f64, on the f32 x) stays this far from 1 - p
WINNER_MARGIN = 1e-4    # the f64 winner of p / q leads the runner-up by this, relative


def scaled_f32(logits: torch.Tensor, temperature: float) -> np.ndarray:
    """x = f32(logits) / T, the f32 quotient, as f64."""
    return (logits.float() / torch.tensor(float(temperature), dtype=torch.float32)).double().numpy()


def sample_literal(logits: torch.Tensor, temperature: Sequence[float], top_k: Optional[Sequence[int]],
                   top_p: Optional[Sequence[float]], q: torch.Tensor) -> torch.Tensor:
    """int32 [rows]: the sampler restated.  logits [rows, V] in any dtype, q f32 [rows, V]."""
    V = logits.shape[1]
    temp = torch.as_tensor(temperature, dtype=torch.float32)
    greedy = logits.float().argmax(dim=-1)
    t = torch.where(temp > 0, temp, torch.ones_like(temp))
    x = logits.to(torch.float32).div_(t.unsqueeze(1))
    k = None if top_k is None else S._norm_k(torch.as_tensor(top_k), V)
    p = None if top_p is None else torch.as_tensor(top_p, dtype=torch.float32)
    x = S.apply_top_k_top_p(x, k, p)
    probs = x.softmax(dim=-1, dtype=torch.float32)
    rand = probs.div_(q.float()).argmax(dim=-1)
    return torch.where(temp > 0, rand, greedy).to(torch.int32)


def probs_f64(logits_row: torch.Tensor, temperature: float, k: int, p: float) -> np.ndarray:
    """Independent evaluation of one random row: the f64 contract's kept set on the f32 x, then an f64 softmax."""
    x = scaled_f32(logits_row, temperature)
    keep = S.kept_f64(x, k, p)
    e = np.where(keep, np.exp(x - x[keep].max()), 0.0)
    return e / e.sum()


def winner_margin(pr: np.ndarray, q_row: torch.Tensor) -> tuple:
    """(token, relative lead of the f64 winner of p / q over the runner-up)."""
    r = pr / q_row.double().numpy()
    top = np.argsort(-r, kind="stable")[:2]
    lead = (r[top[0]] - r[top[1]]) / r[top[0]] if r[top[0]] > 0 else 0.0
    return int(top[0]), float(lead)


def sample_f64(logits: torch.Tensor, temperature, top_k, top_p, q: torch.Tensor):
    """(tokens int32 [rows], smallest winner margin over the random rows) by the independent f64 evaluation."""
    V = logits.shape[1]
    toks, worst = [], float("inf")
    for r in range(logits.shape[0]):
        T = float(temperature[r])
        if T <= 0:
            toks.append(int(logits[r].float().argmax()))
            continue
        k = V if top_k is None else int(top_k[r])
        p = 1.0 if top_p is None else float(top_p[r])
        tok, lead = winner_margin(probs_f64(logits[r], T, k, p), q[r])
        toks.append(tok)
        worst = min(worst, lead)
    return torch.tensor(toks, dtype=torch.int32), worst


class SamplerBatch:
    __slots__ = ("logits", "temps", "ks", "ps", "q", "rebuilt", "redrawn")

    def __init__(self, logits, temps, ks, ps, q, rebuilt, redrawn):
        self.logits, self.temps, self.ks, self.ps, self.q = logits, temps, ks, ps, q
        self.rebuilt, self.redrawn = rebuilt, redrawn


def cumsums_clear(x32: np.ndarray, k: int, p: float, margin: float = CUMSUM_MARGIN) -> bool:
    if p >= 1.0:
        return True
    _, c = S.ascending_cumsums(x32, k)
    return bool(np.abs(c - (1.0 - p)).min() >= margin)


def build_sampler_batch(V: int, dtype: torch.dtype, B: int, seed: int, modes: Sequence[str], tie_cut: bool = False) -> SamplerBatch:
    """B rows; row i takes modes[i % len(modes)]: "k" / "p" / "kp" (filters), "t" (temperature only), "g" (greedy, with
    filters that must be ignored), T in (1, 0.8, 1.25) by row.  sampling_oracle.build_row places p using x rounded to the
    logits dtype; each row is re-checked on the sampler's f32 x: a row with an ascending cumulative sum within
    CUMSUM_MARGIN of 1 - p is rebuilt, a row of q whose f64 winner leads by less than WINNER_MARGIN is redrawn.
    `rebuilt` / `redrawn` count the rows that needed either."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    rows, temps, ks, ps, qs = [], [], [], [], []
    rebuilt = redrawn = 0
    for i in range(B):
        mode = modes[i % len(modes)]
        T = (1.0, 0.8, 1.25)[i % 3]
        again = False
        for _ in range(50):
            if mode in ("g", "t"):
                row, k, p = S.build_row(V, dtype, rng, T, "k")
                k, p = (0, 1.0) if mode == "t" else (int(rng.integers(1, 9)), 0.5)
            else:
                row, k, p = S.build_row(V, dtype, rng, T, mode, tie_cut=tie_cut and "p" in mode)
            if mode == "g" or cumsums_clear(scaled_f32(row, T), k, p):
                break
            again = True
        else:
            raise RuntimeError("no row clear of 1 - p on the f32 x")
        rebuilt += again
        again = False
        for _ in range(50):
            q = torch.empty(V, dtype=torch.float32).exponential_(generator=g)
            if mode == "g" or winner_margin(probs_f64(row, T, k, p), q)[1] >= WINNER_MARGIN:
                break
            again = True
        else:
            raise RuntimeError("no noise row with a clear winner")
        redrawn += again
        rows.append(row)
        temps.append(-1.0 if mode == "g" else T)
        ks.append(k)
        ps.append(p)
        qs.append(q)
    return SamplerBatch(torch.stack(rows), temps, ks, ps, torch.stack(qs), rebuilt, redrawn)


def rounding_split_rows(T: float = 0.7):
    """bf16 rows for T = 0.7 in which f32(l) / T and its bf16 rounding keep different sets.  The bf16 neighbours
    a = 1.515625 and b = 1.5234375 give 2.16518 and 2.17634 in f32 and both round to 2.171875.
      row 0 (top-k): a larger maximum, then b and a, k = 2: f32 keeps {max, b}; rounded, a ties with b and stays;
      row 1 (top-p): the pair sits at the cut, b at the LOWER index: in f32 a's cumulative sum is below 1 - p and b's
      above, so a is dropped and b kept; rounded, the two tie, ties go from the lowest index up, and b is dropped instead.
    Returns (logits bf16 [2, V], temps, ks, ps)."""
    V = 1000
    a, b = 1.515625, 1.5234375
    lo = torch.full((2, V), -20.0)
    # top-k row: token 7 is the maximum, 100 holds a, 200 holds b
    lo[0, 7], lo[0, 100], lo[0, 200] = 4.0, a, b
    # top-p row: token 50 (b) and 300 (a) share nearly all the mass with token 9, slightly larger
    lo[1, 9], lo[1, 50], lo[1, 300] = 1.75, b, a
    logits = lo.to(torch.bfloat16)
    assert float(logits[0, 100]) == a and float(logits[0, 200]) == b
    x = scaled_f32(logits[1], T)
    order, c = S.ascending_cumsums(x, V)
    # 1 - p midway between the cumulative sums of a (token 300) and b (token 50): a dropped, b kept
    ca = float(c[list(order).index(300)])
    cb = float(c[list(order).index(50)])
    assert ca < cb
    p = 1.0 - (ca + cb) / 2
    return logits, [T, T], [2, V], [1.0, p]


# the batches of tests/test_gpu_sampler.py (tests/test_sampler_host.py checks the builder on the same seeds)
SMALL_MODES = (("k",), ("p",), ("kp",), ("kp", "g", "p", "t", "k"))
FULL_MODES = ("kp", "p", "k", "t", "g", "p")


def small_case(dtype: torch.dtype, V: int, modes: Sequence[str]) -> SamplerBatch:
    return build_sampler_batch(V, dtype, 8, seed=V + len(modes) * 7 + len(str(dtype)), modes=modes)


def full_case(V: int) -> SamplerBatch:
    return build_sampler_batch(V, torch.bfloat16, 64, seed=V, modes=FULL_MODES)


def tie_case(dtype: torch.dtype) -> SamplerBatch:
    return build_sampler_batch(32007, dtype, 12, seed=5, modes=("p", "kp"), tie_cut=True)
