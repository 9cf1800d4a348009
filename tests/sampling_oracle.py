"""CPU restatement of vLLM 0.9.2's top-k / top-p probabilities for the rejection sampler (draft_probs = None), and a
fixture builder whose rows keep every top-p cumulative sum clear of 1 - p.

vLLM is not importable here; the rules are restated from vllm/v1/sample/rejection_sampler.py (compute_probs) and
vllm/v1/sample/ops/topk_topp_sampler.py (apply_top_k_top_p, apply_top_k_only), dtypes and sort order included:
  x = logits.div_(T) in the logits dtype (greedy rows: T = 1);
  top-k only: mask x < (k-th largest value), k == vocab meaning no top-k (k <= 0 is treated the same way here);
  top-p: stable ascending sort, the top-k rule on the sorted row, softmax and cumsum in the logits dtype, mask every
  position whose cumsum is <= 1 - p except the last, scatter back;
  p = softmax(masked x, dtype=float32)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch


def _norm_k(k: Optional[torch.Tensor], vocab: int) -> Optional[torch.Tensor]:
    if k is None:
        return None
    k = k.to(torch.long).clone()
    k[(k <= 0) | (k > vocab)] = vocab
    return k


def apply_top_k_only(x: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    V = x.shape[1]
    no_top_k = k == V
    k = k.masked_fill(no_top_k, 1)
    thr = x.topk(int(k.max()), dim=1).values.gather(1, (k - 1).unsqueeze(1))
    thr.masked_fill_(no_top_k.unsqueeze(1), -float("inf"))
    return x.masked_fill(x < thr, -float("inf"))


def apply_top_k_top_p(x: torch.Tensor, k: Optional[torch.Tensor], p: Optional[torch.Tensor]) -> torch.Tensor:
    """x [R, V] in the logits dtype; k int [R] (normalised: vocab = none), p float [R]."""
    if p is None:
        return x if k is None else apply_top_k_only(x, k)
    x_sort, x_idx = x.sort(dim=-1, descending=False, stable=True)
    if k is not None:
        thr = x_sort.gather(1, (x_sort.size(1) - k).unsqueeze(1))
        x_sort = x_sort.masked_fill(x_sort < thr, -float("inf"))
    probs_sum = x_sort.softmax(dim=-1).cumsum(dim=-1)
    mask = probs_sum <= (1 - p.to(x.dtype)).unsqueeze(1)
    mask[:, -1] = False
    x_sort = x_sort.masked_fill(mask, -float("inf"))
    return x_sort.scatter(dim=-1, index=x_idx, src=x_sort)


def compute_probs(logits: torch.Tensor, temperature: torch.Tensor, top_k=None, top_p=None) -> torch.Tensor:
    """Per-row f32 probabilities; rows with temperature <= 0 use T = 1 (vLLM decides them by arg-max)."""
    t = torch.where(temperature > 0, temperature, torch.ones_like(temperature)).to(torch.float32)
    x = (logits.float() / t.unsqueeze(1)).to(logits.dtype)
    x = apply_top_k_top_p(x, _norm_k(top_k, x.shape[1]), None if top_p is None else top_p.float())
    return x.softmax(dim=-1, dtype=torch.float32)


def rejection_topk_topp(target_logits: torch.Tensor, draft_token_ids: Sequence[int], num_draft_tokens: Sequence[int],
                        bonus_token_ids: Sequence[int], max_spec_len: int, temperature: Sequence[float],
                        uniform: np.ndarray, exp_noise: torch.Tensor, top_k: Optional[Sequence[int]] = None,
                        top_p: Optional[Sequence[float]] = None) -> np.ndarray:
    """oracle.spec_oracle.rejection_random with vLLM's top-k / top-p applied to the random rows (per-request values
    expanded to the request's draft rows).  A draft id >= vocab has p = 0."""
    B = len(num_draft_tokens)
    out = np.full((B, max_spec_len + 1), -1, dtype=np.int32)
    rows = int(sum(num_draft_tokens))
    if rows == 0:
        for i in range(B):
            out[i, 0] = int(bonus_token_ids[i])
        return out
    V = target_logits.shape[1]
    req = np.repeat(np.arange(B), np.asarray(num_draft_tokens, dtype=np.int64))
    temp = torch.tensor([float(temperature[r]) for r in req], dtype=torch.float32)
    tk = None if top_k is None else torch.tensor([int(top_k[r]) for r in req])
    tp = None if top_p is None else torch.tensor([float(top_p[r]) for r in req], dtype=torch.float32)
    probs = compute_probs(target_logits[:rows], temp, tk, tp)
    start = 0
    for i, n in enumerate(num_draft_tokens):
        rejected = False
        T = float(temperature[i])
        for pos in range(n):
            row = start + pos
            draft = int(draft_token_ids[row])
            if T <= 0:
                tok = int(torch.argmax(target_logits[row].float()))
                out[i, pos] = tok
                rejected = draft != tok
            else:
                p = probs[row].clone()
                pd = float(p[draft]) if 0 <= draft < V else 0.0
                if pd >= float(uniform[row]):
                    out[i, pos] = draft
                else:
                    if 0 <= draft < V:
                        p[draft] = 0.0
                    out[i, pos] = int(torch.argmax(p / exp_noise[i].float()))
                    rejected = True
            if rejected:
                break
        if not rejected:
            out[i, n] = int(bonus_token_ids[i])
        start += n
    return out


# ------------------------------------------------------------------------------------------------------------------
# kept sets in f64 (the kernel's contract) and the fixture builder
# ------------------------------------------------------------------------------------------------------------------
def scaled(logits: torch.Tensor, temperature: float) -> np.ndarray:
    """x = logits / T rounded to the logits dtype, as f64."""
    return (logits.float() / float(temperature)).to(logits.dtype).double().numpy()


def kept_f64(x: np.ndarray, k: int, p: float) -> np.ndarray:
    """The contract: top-k {x >= tau_k}; top-p over the survivors ordered ascending by (x, index), dropping every token
    whose ascending cumulative probability is <= 1 - p, the largest survivor always kept."""
    V = x.shape[0]
    keep = np.ones(V, dtype=bool)
    if 0 < k < V:
        keep &= x >= np.sort(x)[V - k]
    if p < 1.0:
        idx = np.nonzero(keep)[0]
        order = idx[np.lexsort((idx, x[idx]))]
        e = np.exp(x[order] - x[order].max())
        c = np.cumsum(e / e.sum())
        drop = c <= 1.0 - p
        drop[-1] = False
        keep[order[drop]] = False
    return keep


def ascending_cumsums(x: np.ndarray, k: int) -> tuple:
    V = x.shape[0]
    idx = np.arange(V) if not (0 < k < V) else np.nonzero(x >= np.sort(x)[V - k])[0]
    order = idx[np.lexsort((idx, x[idx]))]
    e = np.exp(x[order] - x[order].max())
    return order, np.cumsum(e / e.sum())


def build_row(V: int, dtype: torch.dtype, rng: np.random.Generator, temperature: float, mode: str,
              margin: float = 1e-2, tie_cut: bool = False):
    """(logits [V] in `dtype`, k, p) for mode "k" (top-k only), "p" (top-p only) or "kp" (both).  A peaked head of
    planted values in [12, 18] (with repeats: boundary ties) over a body N(-8, 1) clipped to [-12, -4].  p is placed midway in a gap of the ascending
    cumulative sums so that no cumulative sum lies within `margin` of 1 - p; with `tie_cut` the gap is taken inside a
    group of tied values, so that the cut-off falls between ties."""
    for _ in range(200):
        body = np.clip(rng.standard_normal(V), -4, 4) - 8.0   # the body holds < 1e-3 of the mass
        n_head = int(rng.integers(8, 24))
        vals = rng.choice(np.arange(12.0, 18.01, 0.5), size=n_head)
        reps = rng.integers(1, 5, size=n_head)
        head = np.repeat(vals, reps)[:max(2, V // 4)]
        pos = rng.choice(V, size=head.size, replace=False)
        body[pos] = head
        row = torch.from_numpy(body.astype(np.float32)).to(dtype)
        x = scaled(row, temperature)
        k = V
        if "k" in mode:
            k = int(rng.integers(1, min(head.size + 6, V)))
        if "p" not in mode:
            return row, k, 1.0
        order, c = ascending_cumsums(x, k)
        gaps = []
        for j in range(-1, len(c) - 1):
            lo = c[j] if j >= 0 else 0.0
            hi = c[j + 1]
            if hi - lo <= 2.5 * margin or lo + margin >= 1.0 - margin:
                continue
            if tie_cut and not (j >= 0 and x[order[j]] == x[order[j + 1]]):
                continue
            gaps.append((lo + hi) / 2)
        if gaps:
            return row, k, float(1.0 - gaps[int(rng.integers(len(gaps)))])
    raise RuntimeError("no row with a clear top-p gap")


def literal_kept(row: torch.Tensor, temperature: float, k: int, p: float) -> np.ndarray:
    """Kept set of the literal restatement (masked to -inf) for one row."""
    x = (row.float() / temperature).to(row.dtype).unsqueeze(0)
    m = apply_top_k_top_p(x, _norm_k(torch.tensor([k]), row.shape[0]), torch.tensor([p]) if p < 1.0 else None)
    return (m[0] != -float("inf")).numpy()
