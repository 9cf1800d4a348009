"""GPU: aic_token_logprobs (ops.token_logprobs) against the f64 oracle of tests/logprobs_oracle.py.

Token ids, their order and the ranks are compared with ==.  Logprobs are held to 1e-5 + 2^-22 |lp| against the f64
log-softmax of the stored values.  Derivation: x - m is exact for 16-bit storage; s = sum exp(x - m) >= 1 carries at most
about 2^-22 relative error from exp plus V * 2^-41 from the 2^-40 fixed-point quantisation, below 4e-7 in log s; the two
f32 roundings of (x - m) - log s add 2^-23 |lp|; the bar leaves an order of magnitude over that.  Every test prints the
largest error it saw as a fraction of the bar before it asserts."""
import numpy as np
import pytest
import torch

import logprobs_oracle as LO

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = LO.all_cases()


def _ops():
    from arcticinference_amd import ops
    return ops


def _call(case, token_ids="case"):
    lg = case.logits.to(DEV) if case.logits.is_contiguous() else _strided_copy(case.logits)
    toks = case.token_ids if token_ids == "case" else token_ids
    ids, lps, ranks = _ops().token_logprobs(
        lg, case.n, token_ids=None if toks is None else torch.tensor(toks, dtype=torch.int32, device=DEV),
        row_index=None if case.row_index is None else torch.tensor(case.row_index, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    return ids.cpu(), lps.cpu(), ranks.cpu()


def _strided_copy(view: torch.Tensor) -> torch.Tensor:
    """The same [T, V] view of a wider [T, V + pad] tensor on the device (row_stride > V)."""
    T, V = view.shape
    wide = torch.zeros((T, view.stride(0)), dtype=view.dtype, device=DEV)
    wide[:, :V] = view.to(DEV)
    out = wide[:, :V]
    assert out.stride(0) == view.stride(0) > V
    return out


def _check(got, want, n, what=""):
    ids, lps, ranks = got
    ids64, lp64, rank64 = want
    assert ids.dtype == torch.int32 and lps.dtype == torch.float32 and ranks.dtype == torch.int64
    assert tuple(ids.shape) == tuple(lps.shape) == (ids64.shape[0], 1 + n) and tuple(ranks.shape) == (ids64.shape[0],)
    print(f"{what} max error / bar = {LO.max_excess(lps.numpy(), lp64):.3f}")
    assert ids.tolist() == ids64.tolist()
    assert ranks.tolist() == rank64.tolist()
    assert LO.within_bar(lps.numpy(), lp64).all(), LO.max_excess(lps.numpy(), lp64)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fixture_matches_the_f64_oracle(case):
    want = LO.f64_oracle(case.served(), case.token_ids, case.n)
    assert want[0][:, 1:].tolist() == case.planted          # the oracle returns the planted order
    got = _call(case)
    _check(got, want, case.n, case.name)
    again = _call(case)                                     # deterministic, bit for bit
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(got, again))


@pytest.mark.parametrize("case", [c for c in CASES if "ties" in c.name or c.name in ("bf16-V128256-n20", "f32-V1000-n5")],
                         ids=lambda c: c.name)
def test_arg_max_form_equals_the_call_given_the_arg_max(case):
    lg = case.served()
    argmax = lg.float().argmax(dim=-1).tolist()             # torch returns the first maximum of a row
    want = LO.f64_oracle(lg, None, case.n)
    assert want[0][:, 0].tolist() == argmax and want[2].min() >= 1
    implicit = _call(case, token_ids=None)
    explicit = _call(case, token_ids=argmax)
    _check(implicit, want, case.n, case.name)
    for a, b in zip(implicit, explicit):
        assert torch.equal(a, b)
    if "ties" in case.name:
        assert implicit[2].tolist()[2] == 2                 # the tied maximum: rank counts both, the lower index is taken


def test_unplanted_rows_values_and_ranks():
    """Random rows tie throughout their top n: ids are unpinned by vLLM, values and the contract's order are not."""
    g = torch.Generator().manual_seed(3)
    V, n = 128256, 20
    lg = (torch.randn(4, V, generator=g) * 3).to(torch.bfloat16)
    toks = torch.randint(0, V, (4,), generator=g).tolist()
    case = LO.Case("random", lg, None, toks, n, None)
    want = LO.f64_oracle(lg, toks, n)
    got = _call(case)
    _check(got, want, n, "random bf16 rows")
    lit = LO.vllm_literal(lg, torch.tensor(toks), n)
    assert LO.within_bar(got[1].numpy(), lit[1].double().numpy()).all()     # topk's values, whatever ids it chose
    assert got[2].tolist() == lit[2].tolist()


def test_the_call_is_capturable_and_replays_over_new_inputs():
    V, n, rows = 32007, 5, 5
    cases = [LO.planted_case(V, torch.bfloat16, rows, n, seed=s) for s in range(3)]
    lg = torch.empty(rows, V, dtype=torch.bfloat16, device=DEV)
    tok = torch.empty(rows, dtype=torch.int32, device=DEV)

    def load(c):
        lg.copy_(c.logits)
        tok.copy_(torch.tensor(c.token_ids, dtype=torch.int32))

    load(cases[0])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _ops().token_logprobs(lg, n, token_ids=tok)             # warm-up: the workspace of this stream exists
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                # straight-line: no parallel branches
        out = _ops().token_logprobs(lg, n, token_ids=tok)
    for i in (1, 2, 0):
        load(cases[i])
        graph.replay()
        torch.cuda.synchronize()
        _check(tuple(o.cpu() for o in out), LO.f64_oracle(cases[i].logits, cases[i].token_ids, n), n, f"replay {i}")


def test_error_returns_and_empty_calls():
    from arcticinference_amd._native import NativeError
    ops = _ops()
    V = 1000
    lg = torch.zeros(3, V, dtype=torch.bfloat16, device=DEV)
    with pytest.raises((ValueError, NativeError)):
        ops.token_logprobs(lg, LO.CAP + 1)
    with pytest.raises((ValueError, NativeError)):
        ops.token_logprobs(lg, 2, token_ids=torch.tensor([0, V, 1], dtype=torch.int32, device=DEV))
    with pytest.raises((ValueError, NativeError)):
        ops.token_logprobs(lg, 2, token_ids=torch.tensor([0, -1, 1], dtype=torch.int32, device=DEV))
    ids, lps, ranks = ops.token_logprobs(lg, 3, row_index=torch.zeros(0, dtype=torch.int64, device=DEV))
    assert tuple(ids.shape) == tuple(lps.shape) == (0, 4) and tuple(ranks.shape) == (0,)
    # unchecked ids (a caller that vouches for them) never index out of the row: NaN and rank 0, the rest right
    ids, lps, ranks = ops.token_logprobs(lg, 2, token_ids=torch.tensor([0, V, 1], dtype=torch.int32, device=DEV),
                                         check_token_ids=False)
    torch.cuda.synchronize()
    assert np.isnan(float(lps[1, 0])) and int(ranks[1]) == 0 and ranks.tolist()[::2] == [V, V]
    assert ids[:, 1:].tolist() == [[0, 1]] * 3          # an all-equal row: the lowest indices
    assert torch.allclose(lps[:, 1:].cpu(), torch.full((3, 2), -float(np.log(V))), atol=1e-5)
