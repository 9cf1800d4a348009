"""GPU: aic_sample_topk_topp (ops.sample_tokens) against the CPU restatement of vLLM's Sampler
(tests/sampler_oracle.py) on the same logits and Exp(1) noise.  The fixture rows keep every top-p cumulative sum 5e-3
clear of 1 - p and every winner of p / q 1e-4 clear of the runner-up (properties of the fixtures, checked on the CPU in
tests/test_sampler_host.py), so the tokens must match exactly, with no row left out."""
import numpy as np
import pytest
import torch

import sampler_oracle as O
import sampling_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from arcticinference_amd import ops
    return ops


def _sample(b_logits, temps, ks, ps, q, use_k=True, use_p=True, row_index=None):
    return _ops().sample_tokens(
        b_logits.to(DEV), torch.tensor(temps, dtype=torch.float32, device=DEV), q.to(DEV),
        top_k=torch.tensor(ks, dtype=torch.int32, device=DEV) if use_k else None,
        top_p=torch.tensor(ps, dtype=torch.float32, device=DEV) if use_p else None, row_index=row_index).cpu()


def _check(b, use_k=True, use_p=True):
    got = _sample(b.logits, b.temps, b.ks, b.ps, b.q, use_k, use_p)
    want = O.sample_literal(b.logits, b.temps, b.ks if use_k else None, b.ps if use_p else None, b.q)
    assert got.dtype == torch.int32 and torch.equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [1000, 32007])
@pytest.mark.parametrize("modes", O.SMALL_MODES)
def test_sampler_matches_the_oracle(dtype, V, modes):
    b = O.small_case(dtype, V, modes)
    # a batch that sets one filter only passes only that filter (the other pointer is NULL)
    _check(b, use_k=any("k" in m for m in modes), use_p=any("p" in m for m in modes))


@pytest.mark.parametrize("V", [128256, 201088])
def test_sampler_at_full_vocab_b64(V):
    _check(O.full_case(V))


def _redraw_until_clear(b, ks, ps):
    """Noise for a batch whose filters were replaced: the winner margin is a property of (row, filters, q)."""
    g = torch.Generator().manual_seed(77)
    q = b.q.clone()
    for r in range(q.shape[0]):
        if b.temps[r] <= 0:
            continue
        for _ in range(50):
            if O.winner_margin(O.probs_f64(b.logits[r], b.temps[r], ks[r], ps[r]), q[r])[1] >= O.WINNER_MARGIN:
                break
            q[r] = torch.empty(q.shape[1]).exponential_(generator=g)
        else:
            raise RuntimeError("no noise row with a clear winner")
    return q


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_boundary_ties_k1_tiny_p_and_disabled_filters(dtype):
    b = O.tie_case(dtype)
    B, V = b.logits.shape
    _check(b)
    for ks, ps in (([1] * B, [1.0] * B),              # k = 1: the maximum (and its ties)
                   ([0] * B, [1e-6] * B),             # p so small that only the largest survivor stays
                   ([V] * B, b.ps), ([V + 5] * B, b.ps),          # k >= V: no top-k
                   (b.ks, [1.0] * B),                 # p = 1: no top-p
                   ([0] * B, [1.0] * B)):             # neither
        q = _redraw_until_clear(b, ks, ps)
        got = _sample(b.logits, b.temps, ks, ps, q)
        assert torch.equal(got, O.sample_literal(b.logits, b.temps, ks, ps, q)), (ks[0], ps[0])


def test_all_greedy_rows_one_row_and_no_rows():
    b = O.small_case(torch.bfloat16, 32007, ("kp", "g", "p", "t", "k"))
    B, V = b.logits.shape
    greedy = b.logits.float().argmax(dim=-1).to(torch.int32)
    got = _sample(b.logits, [-1.0] * B, b.ks, b.ps, b.q)
    assert torch.equal(got, greedy)
    got = _sample(b.logits, [0.0] * B, b.ks, b.ps, b.q, use_k=False, use_p=False)
    assert torch.equal(got, greedy)
    # no noise: every row is greedy whatever its temperature
    got = _ops().sample_tokens(b.logits.to(DEV), torch.ones(B, device=DEV), None).cpu()
    assert torch.equal(got, greedy)
    # ties of the maximum go to the lowest index
    tied = b.logits.clone()
    tied[:, 17] = tied[:, 31000] = 30.0
    assert _sample(tied, [-1.0] * B, b.ks, b.ps, b.q).tolist() == [17] * B
    one = _sample(b.logits[:1], b.temps[:1], b.ks[:1], b.ps[:1], b.q[:1])
    assert torch.equal(one, O.sample_literal(b.logits[:1], b.temps[:1], b.ks[:1], b.ps[:1], b.q[:1]))
    none = _ops().sample_tokens(torch.empty(0, V, dtype=torch.bfloat16, device=DEV), torch.empty(0, device=DEV),
                                torch.empty(0, V, device=DEV), top_k=torch.empty(0, dtype=torch.int32, device=DEV))
    assert none.shape == (0,) and none.dtype == torch.int32
    idx = torch.empty(0, dtype=torch.int64, device=DEV)
    none = _ops().sample_tokens(b.logits.to(DEV), torch.empty(0, device=DEV), torch.empty(0, V, device=DEV), row_index=idx)
    assert none.shape == (0,)


def test_x_stays_in_f32_and_is_not_rounded_to_the_logits_dtype():
    lg, T, ks, ps = O.rounding_split_rows()
    V = lg.shape[1]
    # the rejection oracle's arithmetic (x rounded to bf16) keeps other sets on these rows
    for r in range(2):
        k32 = S.kept_f64(O.scaled_f32(lg[r], T[r]), ks[r], ps[r])
        k16 = S.kept_f64(S.scaled(lg[r], T[r]), ks[r], ps[r])
        assert (k32 != k16).any()
    # noise that makes the token the 16-bit keys would wrongly keep the winner if it is kept at all
    q = torch.ones(2, V)
    q[0, 100] = 1e-3          # row 0: a (token 100) is outside the top-2 in f32; rounded, it ties with b and stays
    q[1, 300] = 1e-3          # row 1: a (token 300) is cut by top-p in f32; rounded, b (token 50) is cut instead
    got = _sample(lg, T, ks, ps, q)
    assert torch.equal(got, O.sample_literal(lg, T, ks, ps, q))
    assert got.tolist() == [7, 9]
    # and the token the f32 arithmetic keeps wins where the rounded arithmetic would have dropped it
    q = torch.ones(2, V)
    q[0, 200] = 1e-3
    q[1, 50] = 1e-3
    got = _sample(lg, T, ks, ps, q)
    assert torch.equal(got, O.sample_literal(lg, T, ks, ps, q))
    assert got.tolist() == [200, 50]


def test_row_index_form_repeats_and_unfiltered_rows():
    b = O.small_case(torch.bfloat16, 32007, ("kp", "g", "p", "t", "k"))
    B, V = b.logits.shape
    want = O.sample_literal(b.logits, b.temps, b.ks, b.ps, b.q)
    full = torch.randn(3 * B + 5, V, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    idx = torch.randperm(full.shape[0], generator=torch.Generator().manual_seed(2))[:B]
    full[idx] = b.logits
    gathered = _sample(b.logits, b.temps, b.ks, b.ps, b.q)
    indexed = _sample(full, b.temps, b.ks, b.ps, b.q, row_index=idx.to(DEV))
    assert torch.equal(gathered, want) and torch.equal(indexed, gathered)
    # an unaligned view (odd row stride, offset base) takes the scalar loads
    odd = torch.zeros(B, V + 3, dtype=torch.bfloat16)
    odd[:, 1:V + 1] = b.logits
    got = _ops().sample_tokens(odd.to(DEV)[:, 1:V + 1], torch.tensor(b.temps, device=DEV), b.q.to(DEV),
                               top_k=torch.tensor(b.ks, dtype=torch.int32, device=DEV),
                               top_p=torch.tensor(b.ps, device=DEV)).cpu()
    assert torch.equal(got, want)
    for _ in range(3):
        assert torch.equal(_sample(b.logits, b.temps, b.ks, b.ps, b.q), gathered)
    # rows without filters: argmax(softmax(f32(l) / T) / q)
    t = torch.tensor([0.6, 0.8, 1.0, 1.25] * (B // 4))
    plain = _ops().sample_tokens(b.logits.to(DEV), t.to(DEV), b.q.to(DEV)).cpu()
    ref = (torch.softmax(b.logits.float() / t[:, None], dim=-1) / b.q).argmax(dim=-1).to(torch.int32)
    assert torch.equal(plain, ref)
    off = _sample(b.logits, t.tolist(), [0, V] * (B // 2), [1.0] * B, b.q)
    assert torch.equal(off, plain)


def test_the_call_is_capturable_and_replays_over_new_inputs():
    V = 32007
    batches = [O.build_sampler_batch(V, torch.bfloat16, 8, seed=100 + i, modes=("kp", "g", "p", "t", "k")) for i in range(3)]
    B = 8
    lg = torch.empty(B, V, dtype=torch.bfloat16, device=DEV)
    temp = torch.empty(B, device=DEV)
    q = torch.empty(B, V, device=DEV)
    tk = torch.empty(B, dtype=torch.int32, device=DEV)
    tp = torch.empty(B, device=DEV)

    def load(b):
        lg.copy_(b.logits)
        temp.copy_(torch.tensor(b.temps))
        q.copy_(b.q)
        tk.copy_(torch.tensor(b.ks, dtype=torch.int32))
        tp.copy_(torch.tensor(b.ps))

    load(batches[0])
    eager = [_sample(b.logits, b.temps, b.ks, b.ps, b.q) for b in batches]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _ops().sample_tokens(lg, temp, q, top_k=tk, top_p=tp)        # warm-up: the workspace of this stream exists
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = _ops().sample_tokens(lg, temp, q, top_k=tk, top_p=tp)
    for i in (1, 2, 0):
        load(batches[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), eager[i]), i
        assert torch.equal(eager[i], O.sample_literal(batches[i].logits, batches[i].temps, batches[i].ks, batches[i].ps, batches[i].q))
