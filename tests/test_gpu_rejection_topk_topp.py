"""GPU: aic_rejection_random_topk_topp (ops.rejection_sample with top_k / top_p) against the CPU restatement of vLLM's
compute_probs + apply_top_k_top_p (tests/sampling_oracle.py), fed the same uniforms and Exp(1) noise.  Rows come from
the margin-planting fixture builder: no top-p cumulative sum lies within 1e-2 of 1 - p, so the kept sets are those of
the contract, and the emitted tokens must match bit for bit."""
import numpy as np
import pytest
import torch

import sampling_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from arcticinference_amd import ops
    return ops


def _batch(V, dtype, B, n, seed, modes, tie_cut=False, oob_draft=False):
    """B requests with n draft rows each; request i takes modes[i % len(modes)]: "k" / "p" / "kp" (filters), "t"
    (temperature only), "g" (greedy).  A request's rows are permutations of one built row (same cumulative sums)."""
    rng = np.random.default_rng(seed)
    rows, drafts, temps, ks, ps = [], [], [], [], []
    for i in range(B):
        mode = modes[i % len(modes)]
        T = (1.0, 0.8, 1.25)[i % 3]
        if mode in ("g", "t"):
            row, k, p = S.build_row(V, dtype, rng, T, "k")
            k, p = (0, 1.0) if mode == "t" else (int(rng.integers(1, 9)), 0.5)   # greedy rows ignore their filters
            T = -1.0 if mode == "g" else T
        else:
            row, k, p = S.build_row(V, dtype, rng, T, mode, tie_cut=tie_cut and "p" in mode)
        x = S.scaled(row, abs(T))
        keep = S.kept_f64(x, k if mode != "g" else V, p if mode != "g" else 1.0)
        for j in range(n):
            perm = torch.from_numpy(rng.permutation(V)) if j else torch.arange(V)
            rows.append(row[perm])
            kj = keep[perm.numpy()]
            kept_ids = np.nonzero(kj)[0]
            r = rng.random()
            if oob_draft and j == n - 1 and i % 4 == 1:
                drafts.append(V + int(rng.integers(0, 3)))
            elif r < 0.4:                                     # the most likely token: often accepted
                drafts.append(int(np.argmax(x[perm.numpy()])))
            elif r < 0.7:
                drafts.append(int(rng.choice(kept_ids)))
            else:
                drafts.append(int(rng.integers(0, V)))
        temps.append(T)
        ks.append(k)
        ps.append(p)
    return torch.stack(rows), drafts, temps, ks, ps


def _fields(r):
    return (r.output_token_ids, r.num_accepted, r.last_token, r.hidden_index)


def _run(lg, drafts, n_draft, temps, ks, ps, seed, use_k=True, use_p=True, row_index=None, full=None):
    B = len(n_draft)
    V = lg.shape[1]
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(len(drafts), dtype=torch.float64, generator=g)
    q = torch.empty(B, V).exponential_(generator=g)
    bonus = torch.randint(0, V, (B,), generator=g, dtype=torch.int32)
    cu = torch.tensor(np.cumsum(n_draft), dtype=torch.int32, device=DEV)
    res = _ops().rejection_sample(
        (full if full is not None else lg).to(DEV), torch.tensor(drafts, dtype=torch.int32, device=DEV), cu,
        bonus.to(DEV), max(n_draft), temperature=torch.tensor(temps, device=DEV), uniform_probs=u.to(DEV),
        exp_noise=q.to(DEV), target_row_index=row_index,
        top_k=torch.tensor(ks, dtype=torch.int32, device=DEV) if use_k else None,
        top_p=torch.tensor(ps, dtype=torch.float32, device=DEV) if use_p else None)
    want = S.rejection_topk_topp(lg, drafts, n_draft, bonus.tolist(), max(n_draft), temps, u.numpy(), q,
                                 ks if use_k else None, ps if use_p else None)
    return res, want


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [1000, 32007])
@pytest.mark.parametrize("modes", [("k",), ("p",), ("kp",), ("kp", "g", "p", "t", "k")])
def test_topk_topp_matches_the_oracle(dtype, V, modes):
    B, n = 8, 3
    lg, drafts, temps, ks, ps = _batch(V, dtype, B, n, seed=V + len(modes) * 7 + len(str(dtype)), modes=modes)
    res, want = _run(lg, drafts, [n] * B, temps, ks, ps, seed=1)
    assert np.array_equal(res.output_token_ids.cpu().numpy(), want)


@pytest.mark.parametrize("V", [128256, 201088])
def test_topk_topp_at_full_vocab_b64_k3(V):
    B, n = 64, 3
    lg, drafts, temps, ks, ps = _batch(V, torch.bfloat16, B, n, seed=V, modes=("kp", "p", "k", "t", "g", "p"))
    res, want = _run(lg, drafts, [n] * B, temps, ks, ps, seed=2)
    got = res.output_token_ids.cpu().numpy()
    assert np.array_equal(got, want)
    acc = sum(int((got[i] == np.asarray(drafts[i * n:(i + 1) * n] + [-2])).sum()) for i in range(B))
    assert 5 < acc < B * n                                    # both accepted and recovered positions are exercised


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_boundary_ties_k1_tiny_p_and_out_of_vocab_drafts(dtype):
    V, B, n = 32007, 12, 4
    lg, drafts, temps, ks, ps = _batch(V, dtype, B, n, seed=5, modes=("p", "kp"), tie_cut=True, oob_draft=True)
    res, want = _run(lg, drafts, [n] * B, temps, ks, ps, seed=3)
    assert np.array_equal(res.output_token_ids.cpu().numpy(), want)
    # k = 1 everywhere; then p so small that only the largest survivor stays
    ks1 = [1] * B
    res, want = _run(lg, drafts, [n] * B, temps, ks1, ps, seed=4, use_p=False)
    assert np.array_equal(res.output_token_ids.cpu().numpy(), want)
    res, want = _run(lg, drafts, [n] * B, temps, ks, [1e-6] * B, seed=5, use_k=False)
    assert np.array_equal(res.output_token_ids.cpu().numpy(), want)


def test_target_row_index_form():
    V, B, n = 32007, 6, 3
    lg, drafts, temps, ks, ps = _batch(V, torch.bfloat16, B, n, seed=9, modes=("kp", "t", "p"))
    full = torch.randn(B * (n + 1) + 5, V).to(torch.bfloat16)
    idx = torch.randperm(full.shape[0])[:B * n]
    full[idx] = lg
    res, want = _run(lg, drafts, [n] * B, temps, ks, ps, seed=6, row_index=idx.to(DEV), full=full)
    assert np.array_equal(res.output_token_ids.cpu().numpy(), want)


def test_disabled_filters_are_bit_identical_to_aic_rejection_random_and_calls_repeat_exactly():
    V, B, n = 32007, 16, 3
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn(B * n, V, generator=g) * 2).to(torch.bfloat16).to(DEV)
    drafts = torch.randint(0, V, (B * n,), generator=g, dtype=torch.int32).to(DEV)
    drafts[::2] = lg[::2].float().argmax(dim=-1).to(torch.int32)
    cu = torch.arange(1, B + 1, dtype=torch.int32, device=DEV) * n
    temp = torch.tensor([(-1.0 if i % 5 == 0 else 0.5 + 0.1 * i) for i in range(B)], device=DEV)
    u = torch.rand(B * n, dtype=torch.float64, generator=g).to(DEV)
    q = torch.empty(B, V).exponential_(generator=g).to(DEV)
    bonus = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).to(DEV)
    kw = dict(temperature=temp, uniform_probs=u, exp_noise=q)
    ref = _ops().rejection_sample(lg, drafts, cu, bonus, n, **kw)
    off_k = torch.tensor([0 if i % 2 else V for i in range(B)], dtype=torch.int32, device=DEV)
    for extra in (dict(top_k=off_k), dict(top_p=torch.ones(B, device=DEV)), dict(top_k=off_k, top_p=torch.ones(B, device=DEV))):
        got = _ops().rejection_sample(lg, drafts, cu, bonus, n, **kw, **extra)
        for a, b in zip(_fields(ref), _fields(got)):
            assert torch.equal(a, b), extra
    tk = torch.tensor([20 + i for i in range(B)], dtype=torch.int32, device=DEV)
    tp = torch.tensor([0.3 + 0.04 * i for i in range(B)], device=DEV)
    first = _ops().rejection_sample(lg, drafts, cu, bonus, n, **kw, top_k=tk, top_p=tp)
    again = _ops().rejection_sample(lg, drafts, cu, bonus, n, **kw, top_k=tk, top_p=tp)
    for a, b in zip(_fields(first), _fields(again)):
        assert torch.equal(a, b)


def test_torch_sort_of_a_full_vocab_bf16_row_with_ties_is_stable_on_the_gpu():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(4, 128256, generator=g) * 2).to(torch.bfloat16).to(DEV)   # ~ 64k distinct values over 128k: ties
    v1, i1 = torch.sort(x, dim=-1)
    v2, i2 = torch.sort(x, dim=-1, stable=True)
    assert torch.equal(v1, v2) and torch.equal(i1, i2)
