"""CPU restatement, in torch f32, of the logits edits of vLLM 0.9.2's Sampler.forward (v1/sample/sampler.py:
apply_allowed_token_ids, apply_bad_words, apply_logits_bias, apply_penalties -> apply_min_token_penalties +
apply_all_penalties, apply_min_p; model_executor/layers/utils.py: get_token_bin_counts_and_mask, apply_penalties; vLLM
is not importable here, the rules are recalled), in the operation order aic_logits_edit documents, and the fixtures of
tests/test_gpu_logits_edit.py (tests/test_logits_edit_host.py checks their properties on the CPU).

Per-request inputs are plain Python here — lists of banned tokens, bias dicts, token lists — so that nothing of the
packing under test is shared with the expectation."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

NEG_INF = float("-inf")
MIN_P_MARGIN = 1e-3      # no token of a min-p fixture lies this close to the threshold (f64, in units of (x - m) / T)
CASES = ("mask", "ban", "bias", "penalties", "min_p", "all")


def bin_counts_and_mask(tokens: Sequence[Sequence[int]], vocab: int):
    """get_token_bin_counts_and_mask: int64 counts [rows, vocab] (ids >= vocab land in a column that is cut off) and
    counts > 0."""
    rows = len(tokens)
    counts = torch.zeros((rows, vocab + 1), dtype=torch.long)
    for r, toks in enumerate(tokens):
        t = torch.as_tensor([int(v) if 0 <= int(v) < vocab else vocab for v in toks], dtype=torch.long)
        if t.numel():
            counts[r].scatter_add_(0, t, torch.ones_like(t))
    counts = counts[:, :vocab]
    return counts, counts > 0


def edit(logits: torch.Tensor, *, allowed_mask: Optional[torch.Tensor] = None, bans: Optional[List[List[int]]] = None,
         bias: Optional[List[Dict[int, float]]] = None, prompts: Optional[List[List[int]]] = None,
         outputs: Optional[List[List[int]]] = None, repetition: Optional[Sequence[float]] = None,
         frequency: Optional[Sequence[float]] = None, presence: Optional[Sequence[float]] = None) -> torch.Tensor:
    """f32 [rows, V]: steps 1 - 7 (everything but min-p).  `bans` are the tokens that apply_bad_words and
    apply_min_token_penalties set to -inf this step."""
    x = logits.to(torch.float32).clone()
    rows, V = x.shape
    if allowed_mask is not None:
        x.masked_fill_(allowed_mask.bool(), NEG_INF)
    for r, toks in enumerate(bans or ()):
        for t in toks:
            if 0 <= t < V:
                x[r, t] = NEG_INF
    for r, d in enumerate(bias or ()):
        for t, b in (d or {}).items():
            if 0 <= t < V:
                x[r, t] += torch.tensor(b, dtype=torch.float32)
    if repetition is not None or frequency is not None or presence is not None:
        _, prompt_mask = bin_counts_and_mask(prompts or [[]] * rows, V)
        out_counts, out_mask = bin_counts_and_mask(outputs or [[]] * rows, V)
        rep = torch.as_tensor(repetition if repetition is not None else [1.0] * rows, dtype=torch.float32)
        freq = torch.as_tensor(frequency if frequency is not None else [0.0] * rows, dtype=torch.float32)
        pres = torch.as_tensor(presence if presence is not None else [0.0] * rows, dtype=torch.float32)
        penalties = torch.where(prompt_mask | out_mask, rep.unsqueeze(1), torch.ones((), dtype=torch.float32))
        scaling = torch.where(x > 0, 1.0 / penalties, penalties)
        x *= scaling
        x -= freq.unsqueeze(1) * out_counts
        x -= pres.unsqueeze(1) * out_mask
    return x


def min_p_distance(x: torch.Tensor, min_p: Sequence[float], temperature: Sequence[float]) -> np.ndarray:
    """f64 [rows, V]: (x_v - m) / T - ln(min_p) on the f32 edited rows, >= 0 for the kept tokens; +inf on the rows min-p
    does not touch (T <= 0 or min_p == 0) and for nothing else (a -inf logit is -inf)."""
    xd = x.double().numpy()
    d = np.full(xd.shape, np.inf)
    for r in range(xd.shape[0]):
        if temperature[r] > 0 and min_p[r] > 0:
            T = float(np.float32(temperature[r]))
            d[r] = (xd[r] - xd[r].max()) / T - math.log(float(np.float32(min_p[r])))
    return d


def apply_min_p(x: torch.Tensor, min_p: Sequence[float], temperature: Sequence[float]) -> torch.Tensor:
    """The edited rows after min-p, evaluated in f32 as the kernel documents it: keep iff (x - m) / T >= ln(min_p)."""
    out = x.clone()
    for r in range(x.shape[0]):
        if temperature[r] > 0 and min_p[r] > 0:
            T = torch.tensor(temperature[r], dtype=torch.float32)
            cut = torch.log(torch.tensor(min_p[r], dtype=torch.float32))
            keep = (x[r] - x[r].max()) / T >= cut
            out[r] = torch.where(keep, x[r], torch.full_like(x[r], NEG_INF))
    return out


# ---------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------
class Fixture:
    """Raw logits [rows, V] (f32 values on the 1/8 grid in [-32, 32]: exact in bf16 and fp16 too, so one expectation
    serves the three dtypes) and the per-request edit inputs."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def oracle_kwargs(self, case: str) -> dict:
        kw = {}
        if case in ("mask", "all"):
            kw["allowed_mask"] = self.mask
        if case in ("ban", "all"):
            kw["bans"] = self.bans
        if case in ("bias", "all"):
            kw["bias"] = self.bias
        if case in ("penalties", "all"):
            kw.update(prompts=self.prompts, outputs=self.outputs, repetition=self.repetition, frequency=self.frequency,
                      presence=self.presence)
        return kw

    def expected(self, case: str) -> torch.Tensor:
        x = edit(self.logits, **self.oracle_kwargs(case))
        return apply_min_p(x, self.min_p, self.temperature) if case in ("min_p", "all") else x


REPETITION = [1.3, 0.8, 1.0, 1.5, 0.9]
FREQUENCY = [0.5, -0.3, 0.0, -0.1, 0.2]
PRESENCE = [0.25, -0.2, 0.0, 0.4, -0.6]
MIN_P = [0.1, 0.0, 0.05, 0.2, 0.3]
TEMPERATURE = [1.0, 0.7, -1.0, 0.5, 1.3]      # row 1 has min_p = 0, row 2 is greedy: min-p touches neither
REPEATS = 300                                 # occurrences of token 7 in row 0's output: a count above 255


def build_fixture(V: int, rows: int, segment: int, seed: int = 0) -> Fixture:
    """Histories and logits planted as tests/test_gpu_logits_edit.py's docstring lists them.  Raw logits that would put
    a token within 2 * MIN_P_MARGIN of the min-p threshold (in the "min_p" or the "all" case) are moved to -30."""
    assert 1 <= rows <= 5 and V > 64
    rng = np.random.default_rng(seed + V + rows)
    edges = sorted({t for t in (0, segment - 1, segment, V - 1) if 0 <= t < V})
    logits = torch.from_numpy(rng.integers(-48, 49, size=(rows, V)).astype(np.float32) / 8.0)
    for r in range(rows):
        logits[r, 0], logits[r, 1], logits[r, 2], logits[r, 3] = 2.5, -1.25, 0.0, NEG_INF     # positive, negative, zero, -inf
        logits[r, 20 + r] = 9.0                                                                 # a clear maximum
        logits[r, 40] = 8.5
    prompts, outputs = [], []
    for r in range(rows):
        if r == 0:
            # token 11 in the prompt only; 7 repeated; the segment edges and the planted logits (0 .. 3) in the output
            prompts.append([11, 12, 0] + rng.integers(0, V, 30).tolist() + [V] * 9)
            outputs.append([7] * REPEATS + edges + [1, 2, 3, 40] + rng.integers(0, V, 50).tolist())
        elif r == 1:
            prompts.append([11, 3, 2, V - 1] + rng.integers(0, V, 20).tolist() + [V] * 19)
            outputs.append([])                                                                  # an empty output
        elif r == 2:
            prompts.append([V] * 43)                                                            # padding only
            outputs.append(rng.integers(0, V, 17).tolist())
        else:
            prompts.append(rng.integers(0, V, 43).tolist())
            outputs.append(rng.integers(0, V, 40).tolist() + edges + [20 + r])
    bans = [[5, segment - 1, 40], [], [22], [V - 1, 0, V, -1], [2]][:rows]   # 22: row 2's raw maximum; V and -1 are ignored
    bans[0] = [t for t in bans[0] if t < V]
    bias = [{9: 1.5, segment: -2.0, 3: 4.0}, {}, None, {V - 1: 3.0, 1: -0.75}, {segment - 1: 0.375}][:rows]
    bias = [None if b is None else {t: v for t, v in b.items() if t < V} for b in bias]
    mask = torch.from_numpy(rng.random((rows, V)) < 0.1)
    mask[:, 20:25] = False                                                                      # the maxima stay allowed
    mask[:, 40] = False
    fx = Fixture(V=V, rows=rows, segment=segment, logits=logits, prompts=prompts, outputs=outputs, bans=bans, bias=bias,
                 mask=mask, repetition=REPETITION[:rows], frequency=FREQUENCY[:rows], presence=PRESENCE[:rows],
                 min_p=MIN_P[:rows], temperature=TEMPERATURE[:rows], moved=0)
    for _ in range(20):
        close = np.zeros((rows, V), dtype=bool)
        for case in ("min_p", "all"):
            d = min_p_distance(edit(fx.logits, **fx.oracle_kwargs(case)), fx.min_p, fx.temperature)
            close |= np.abs(d) < 2 * MIN_P_MARGIN
        if not close.any():
            return fx
        fx.moved += int(close.sum())
        fx.logits[torch.from_numpy(close)] = -30.0
    raise RuntimeError("no fixture clear of the min-p threshold")


def segment_size() -> int:
    """aic_logits_edit_segment() (the library loads without a GPU)."""
    from arcticinference_amd import _native
    return int(_native.lib().aic_logits_edit_segment())


def shapes(segment: int):
    """(V, rows) of the GPU tests: one ragged segment; three segments with a ragged last one, a multiple of 4 but not
    of 8 (16-byte stores, a 4-token scalar tail)."""
    return [(1000, 1), (1000, 5), (2 * segment + 1004, 1), (2 * segment + 1004, 5)]
