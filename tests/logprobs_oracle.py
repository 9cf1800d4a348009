"""CPU oracles and fixtures for aic_token_logprobs (ops.token_logprobs).

vLLM 0.9.2 reports the logprobs of a sampler call with Sampler.compute_logprobs and Sampler.gather_logprobs
(v1/sample/sampler.py; vLLM is not importable here, both are recalled):
  compute_logprobs  logits.log_softmax(dim=-1, dtype=torch.float32) of the RAW logits;
  gather_logprobs   topk(logprobs, n), the sampled token's logprob gathered, its rank (logprobs >= its logprob).sum(-1),
                    and the token in column 0 in front of the top n.
`vllm_literal` restates the two in torch.  `f64_oracle` is the independent evaluation the kernel is held to: the f64
log-softmax of the stored values, the top n by (value descending, index ascending), the rank counted on the raw values.

Random bf16 logits at V = 128 256 tie throughout their top 20 (about 40 representable values span that range), and
torch.topk leaves the order of ties unspecified, so unplanted rows cannot pin an order: `build_row` plants n + 2 strictly
distinct, dtype-representable values above everything else at chosen indices."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

CAP = 32                 # aic_logprobs_max()
ATOL, RTOL = 1e-5, 2.0 ** -22
# The bar on a logprob against f64_oracle: ATOL + RTOL * |lp|.  x - m is exact for 16-bit storage (and one f32 rounding,
# inside the relative term, for f32).  s = sum exp(x - m) >= 1 carries at most about 2^-22 relative error from exp plus
# V * 2^-41 from the 2^-40 fixed-point quantisation (1e-7 at V = 201 088): below 4e-7 in log s.  The two f32 roundings of
# the result, (x - m) - log s, add 2^-23 |lp|.  The bar leaves an order of magnitude over that.


class LogprobsLists(NamedTuple):
    logprob_token_ids: list
    logprobs: list
    sampled_token_ranks: list


class LogprobsTensors(NamedTuple):
    """vLLM 0.9.2's v1/outputs.LogprobsTensors (recalled): what the stand-in's module lacks."""
    logprob_token_ids: torch.Tensor
    logprobs: torch.Tensor
    selected_token_ranks: torch.Tensor

    def tolists(self) -> LogprobsLists:
        return LogprobsLists(self.logprob_token_ids.tolist(), self.logprobs.tolist(), self.selected_token_ranks.tolist())


def vllm_literal(logits: torch.Tensor, token_ids: torch.Tensor, n: int):
    """(ids int32 [rows, 1+n], logprobs f32 [rows, 1+n], ranks int64 [rows]): compute_logprobs + gather_logprobs."""
    logprobs = logits.log_softmax(dim=-1, dtype=torch.float32)
    tok = token_ids.to(torch.int64).unsqueeze(-1)
    token_logprobs = logprobs.gather(-1, tok)
    ranks = (logprobs >= token_logprobs).sum(-1)
    ids, vals = tok, token_logprobs
    if n > 0:
        topk_logprobs, topk_indices = torch.topk(logprobs, n, dim=-1)
        ids = torch.cat((tok, topk_indices), dim=1)
        vals = torch.cat((token_logprobs, topk_logprobs), dim=1)
    return ids.to(torch.int32), vals, ranks


def f64_oracle(logits: torch.Tensor, token_ids: Optional[Sequence[int]], n: int):
    """(ids int64 [rows, 1+n], logprobs f64 [rows, 1+n], ranks int64 [rows]) evaluated in numpy f64 on the stored
    values; token_ids None: the arg-max, ties to the lowest index."""
    x = logits.double().numpy()
    rows, V = x.shape
    ids = np.zeros((rows, 1 + n), dtype=np.int64)
    lps = np.zeros((rows, 1 + n), dtype=np.float64)
    ranks = np.zeros(rows, dtype=np.int64)
    idx = np.arange(V)
    for r in range(rows):
        m = x[r].max()
        with np.errstate(divide="ignore"):
            lp = (x[r] - m) - np.log(np.exp(x[r] - m).sum())
        tok = int(np.argmax(x[r])) if token_ids is None else int(token_ids[r])
        top = np.lexsort((idx, -x[r]))[:n]
        ids[r, 0], ids[r, 1:] = tok, top
        lps[r, 0], lps[r, 1:] = lp[tok], lp[top]
        ranks[r] = int((x[r] >= x[r, tok]).sum())
    return ids, lps, ranks


def within_bar(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Elementwise: |got - want| <= ATOL + RTOL |want|; -inf must be met by -inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isneginf(want)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - want) <= ATOL + RTOL * np.abs(want)
    return np.where(inf, np.isneginf(got), ok)


def max_excess(got: np.ndarray, want: np.ndarray) -> float:
    """Largest |got - want| / (ATOL + RTOL |want|) over the finite entries: below 1 inside the bar."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / (ATOL + RTOL * np.abs(want[fin]))).max())


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------------------------
def planted_values(count: int, dtype: torch.dtype) -> torch.Tensor:
    """`count` strictly descending values in [15.5, 24.25], exact in bf16 / fp16 (steps of 0.25 at 0.125 spacing) and,
    for f32, moved by a few ulps each so that the low digits of the 32-bit keys differ too."""
    v = 24.25 - 0.25 * torch.arange(count, dtype=torch.float64)
    if dtype == torch.float32:
        v = v - 3e-6 * torch.arange(count, dtype=torch.float64)
    out = v.to(dtype)
    assert bool((out[:-1].double() > out[1:].double()).all())
    return out


def background(V: int, dtype: torch.dtype, g: torch.Generator) -> torch.Tensor:
    return (torch.randn(V, generator=g) * 2.0).clamp_(-9.0, 9.0).to(dtype)


def planted_indices(V: int, count: int, layout: str, g: torch.Generator) -> List[int]:
    """Where the planted values go, largest first: "stretch" all in one 256-element stretch, "segments" spread evenly
    over the row (one per 2048-element segment where the row has that many), "ends" index 0 and V - 1 among them."""
    if layout == "stretch":
        start = min(V // 3, V - 256)
        pos = (torch.randperm(256, generator=g)[:count] + start).tolist()
    elif layout == "segments":
        base = [(j * V) // count + 7 for j in range(count)]
        pos = [base[i] for i in torch.randperm(count, generator=g).tolist()]
    elif layout == "ends":
        mid = (torch.randperm(V - 2, generator=g)[:count - 2] + 1).tolist()
        pos = [V - 1] + mid[:count // 2 - 1] + [0] + mid[count // 2 - 1:]
        pos = pos[:count]
    else:
        raise ValueError(layout)
    assert len(set(pos)) == count and all(0 <= p < V for p in pos)
    return [int(p) for p in pos]


def build_row(V: int, dtype: torch.dtype, n: int, layout: str, token: str, g: torch.Generator):
    """(row [V], token id, planted indices largest first).  `token`: "top" rank 1; "mid" the middle of the top n;
    "outside" just outside it (rank n + 1); "min" the unique row minimum (rank V); "tied7" one of seven entries that
    share a value between the planted ones and the rest (rank n + 2 + 7)."""
    row = background(V, dtype, g)
    count = n + 2
    pos = planted_indices(V, count, layout, g)
    row[pos] = planted_values(count, dtype)
    free = [i for i in (torch.randperm(V, generator=g)[:count + 8]).tolist() if i not in set(pos)]
    if token == "top":
        tok = pos[0]
    elif token == "mid":
        tok = pos[n // 2]
    elif token == "outside":
        tok = pos[n]
    elif token == "min":
        tok = free[0]
        row[tok] = -30.0
    elif token == "tied7":
        row[free[:7]] = 11.0
        tok = free[3]
    else:
        raise ValueError(token)
    return row, int(tok), pos


class Case(NamedTuple):
    name: str
    logits: torch.Tensor                 # [T, V], possibly a strided view
    row_index: Optional[List[int]]
    token_ids: Optional[List[int]]       # None: the arg-max form
    n: int
    planted: Optional[List[List[int]]]   # per served row: the indices columns 1..n must hold, in order (None: unpinned)

    def served(self) -> torch.Tensor:
        """The rows of the call, gathered, contiguous."""
        lg = self.logits if self.row_index is None else self.logits[torch.tensor(self.row_index)]
        return lg.contiguous()


LAYOUTS = ("stretch", "segments", "ends")
TOKENS = ("top", "mid", "outside", "min", "tied7")
_NAMES = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def planted_case(V: int, dtype: torch.dtype, rows: int, n: int, seed: int = 0, pad: int = 0,
                 row_index: Optional[List[int]] = None, total_rows: Optional[int] = None) -> Case:
    """`rows` planted rows, layouts and token kinds rotating with the row.  With `row_index` the rows live in a
    [total_rows, V] view of a [total_rows, V + pad] tensor and are served through the index (repeats allowed)."""
    g = torch.Generator().manual_seed(1000 * n + V % 997 + seed)
    T = total_rows or rows
    store = torch.zeros((T, V + pad), dtype=dtype)
    toks, plants = [], []
    for r in range(T):
        row, tok, pos = build_row(V, dtype, n, LAYOUTS[(r + seed) % 3], TOKENS[(r + 2 * seed) % 5], g)
        store[r, :V] = row
        toks.append(tok)
        plants.append(pos[:n])
    logits = store[:, :V]
    name = f"{_NAMES[dtype]}-V{V}-n{n}" + (f"-pad{pad}" if pad else "") + ("-indexed" if row_index else "")
    if row_index is None:
        return Case(name, logits, None, toks, n, plants)
    return Case(name, logits, list(row_index), [toks[i] for i in row_index], n, [plants[i] for i in row_index])


def tie_case(V: int, dtype: torch.dtype, n: int = 5) -> Case:
    """Row 0: the cut value occurs four times, two of them inside the cut: the two lowest indices must win.  Row 1: a
    tied pair inside the list, ordered by index, and the selected token is the pair's second (rank counts both).  Row 2:
    the maximum itself is tied (for the arg-max form)."""
    g = torch.Generator().manual_seed(V + n)
    vals = planted_values(n + 2, dtype)
    rows, toks, plants = [], [], []
    # row 0: n - 2 distinct values, then the cut value at four indices given in descending index order
    row = background(V, dtype, g)
    pos = planted_indices(V, n + 2, "segments", g)
    top, four = pos[:n - 2], sorted(pos[n - 2:n + 2], reverse=True)
    row[top] = vals[:n - 2]
    row[four] = vals[n - 2]
    rows.append(row)
    toks.append(four[0])                       # the highest tied index: outside the list, rank n + 2
    plants.append(top + sorted(four)[:2])
    # row 1: values 1 and 2 of the list are equal; the larger index was planted first
    row = background(V, dtype, g)
    pos = planted_indices(V, n + 2, "stretch", g)
    v = vals.clone()
    v[2] = v[1]
    row[pos] = v
    a, b = sorted(pos[1:3])
    rows.append(row)
    toks.append(b)
    plants.append(([pos[0], a, b] + pos[3:])[:n])
    # row 2: the two largest values are equal
    row = background(V, dtype, g)
    pos = planted_indices(V, n + 2, "ends", g)
    v = vals.clone()
    v[1] = v[0]
    row[pos] = v
    a, b = sorted(pos[0:2])
    rows.append(row)
    toks.append(a)
    plants.append(([a, b] + pos[2:])[:n])
    return Case(f"{_NAMES[dtype]}-V{V}-n{n}-ties", torch.stack(rows), None, toks, n, plants)


def masked_case(V: int, dtype: torch.dtype) -> Case:
    """-inf everywhere except 5 entries, n = 8: the five in order, then the three lowest masked indices at -inf."""
    g = torch.Generator().manual_seed(V)
    rows, toks, plants = [], [], []
    for r in range(2):
        row = torch.full((V,), -float("inf"), dtype=dtype)
        pos = planted_indices(V, 5, ("segments", "ends")[r], g)
        row[pos] = planted_values(5, dtype) - (20.0 if r else 0.0)
        masked = [i for i in range(8) if i not in pos][:3]
        rows.append(row)
        toks.append(pos[2] if r == 0 else masked[1])     # row 1 selects a masked token: logprob -inf, rank V
        plants.append(pos + masked)
    return Case(f"{_NAMES[dtype]}-V{V}-masked", torch.stack(rows), None, toks, 8, plants)


def all_cases() -> List[Case]:
    """Every fixture of tests/test_gpu_logprobs.py (tests/test_logprobs_host.py holds the two oracles against each
    other on the same list)."""
    f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
    cases = []
    for k, dtype in enumerate((f32, bf16, f16)):
        for n in (0, 1, 5, 20, 32):
            cases.append(planted_case(1000, dtype, 5, n, seed=k))
    cases += [planted_case(128256, bf16, 3, 20), planted_case(128256, f16, 3, 5, seed=1),
              planted_case(128256, f32, 3, 32, seed=2), planted_case(201088, bf16, 3, 32, seed=1),
              planted_case(201088, f32, 3, 1), planted_case(201088, f16, 3, 20, seed=2)]
    idx = [5, 2, 5, 11, 0]
    cases += [planted_case(1000, bf16, 5, 5, pad=3, row_index=idx, total_rows=16),       # odd stride: scalar loads
              planted_case(1000, f32, 5, 20, pad=24, row_index=idx, total_rows=16),
              planted_case(128256, bf16, 3, 20, pad=8, row_index=[9, 4, 9], total_rows=16),
              planted_case(201088, f16, 3, 5, pad=8, row_index=[15, 15, 0], total_rows=16)]
    for dtype in (f32, bf16, f16):
        cases += [tie_case(1000, dtype), masked_case(1000, dtype)]
    cases += [tie_case(128256, bf16, n=20), tie_case(201088, f32), masked_case(128256, bf16), masked_case(201088, f32)]
    return cases
