"""CPU: the planted-key fixtures of tests/attention_fixtures.py are sharp enough that tests/test_gpu_attention_planted.py
would fail on a kernel whose mask is off by one key.  References only, never the code under test.  For every (head size,
cache dtype, window) combination the GPU module uses, at reduced head counts (two kv heads of G = 4):

(a) the float64 restatement agrees with the fp32 oracle (oracle.spec_oracle.verify_attention) to <= 1e-4, a tenth of
    the GPU tests' atol: bounded scores make fp32 a fair reference;
(b) on every `edge`, `win_lo` and `far` row the target key holds >= 0.999 of the row's weight;
(c) four mutated references (causal edge +1 / -1, window lower edge +1 / -1) differ from the true one by >= 0.1
    (100 x atol) in max-abs on EVERY row whose aim the mutation concerns (`past`, `edge`, `win_lo`, `below`), except
    the `past` aim of a request's last query row when position seq_len holds no planted key.

Measured margins (A = 40 nats; requests of 300 / 33 / 4 / 129 / 34 / 500 query tokens at contexts 4096 / 8192 / 4100 /
129 / 1034 / 2100, sinks ~ N(0, 2)): largest fp32 / float64 gap, smallest target weight, smallest mutation distance
    D 128 bf16  W 0 / 33 / 128:  2.9e-6 / 1.7e-6 / 2.3e-6,  1.000000,  2.04 / 2.41 / 2.07
    D 128 fp8   W 0 / 33 / 128:  6.6e-6 / 3.9e-6 / 4.8e-6,  1.000000,  1.95 / 1.98 / 2.02
    D  64 bf16  W 0 / 33 / 128:  5.3e-6 / 1.7e-6 / 1.9e-6,  1.000000,  1.64 / 1.71 / 1.85"""
import pytest
import torch

import attention_fixtures as F

Q_LENS = [300, 33, 4, 129, 34, 500]
CTXS = [4096, 8192, 4100, 129, 1034, 2100]      # 4096: a page border without a planted successor (the exception of (c))
COMBOS = [(D, fp8, W) for D, fp8 in ((128, False), (128, True), (64, False)) for W in (0, 33, 128)]


def _sinks(Hq, seed):
    return (torch.randn(Hq, generator=torch.Generator().manual_seed(seed)) * 2).float()


def margins(D, fp8, W, plant_below=False):
    """(largest |float64 - fp32 oracle|, smallest target weight on seen rows, smallest mutation distance on concerned
    rows, number of concerned rows)."""
    c = F.planted_case(Q_LENS, CTXS, 8, 2, D, 16, seed=D + W + fp8, window=W, fp8=fp8, sinks=_sinks(8, W),
                       plant_below=plant_below)
    assert c.stale == [False, True, True, True, True, True]
    true, wt = F.reference(c)
    gap = float((true.float() - F.oracle(c)).abs().max())
    weight = float(wt[F.rows_of(c, F.SEEN)].min())
    muts = [(dict(causal=+1), F.PAST), (dict(causal=-1), F.EDGE)]
    if W:
        muts += [(dict(win_lo=+1), F.WIN_LO), (dict(win_lo=-1), F.BELOW)]
    dist, n = float("inf"), 0
    for kw, kind in muts:
        rows = F.rows_of(c, (kind,))
        if kind == F.PAST:
            rows &= ~F.last_rows_without_stale_slot(c)
        assert int(rows.sum()) >= 100, (kw, int(rows.sum()))
        d = (F.reference(c, **kw)[0] - true).abs().amax(dim=-1)
        dist = min(dist, float(d[rows].min()))
        n += int(rows.sum())
    return gap, weight, dist, n


@pytest.mark.parametrize("D,fp8,W", COMBOS, ids=[f"D{D}-{'fp8' if f else 'bf16'}-W{W}" for D, f, W in COMBOS])
def test_planted_fixtures_are_fair_and_sharp(D, fp8, W):
    gap, weight, dist, n = margins(D, fp8, W)
    print(f"D {D} fp8 {fp8} W {W}: fp32/float64 gap {gap:.3g}, min target weight {weight:.6f}, "
          f"min mutation distance {dist:.3g} over {n} rows")
    assert gap <= 1e-4
    assert weight >= 0.999
    assert dist >= 0.1


def test_planted_pages_below_the_window_keep_the_fixture_sharp():
    """The lure keys below every window (plant_below) are masked in the true reference: the same three conditions hold."""
    gap, weight, dist, _ = margins(64, False, 128, plant_below=True)
    assert gap <= 1e-4 and weight >= 0.999 and dist >= 0.1


def test_aims_cover_every_kind_on_block_wave_and_tile_borders():
    """Every aim occurs on first rows of 128-row blocks, 32-row waves and 16-row MFMA tiles, and the heads of one token
    differ in their aims."""
    c = F.planted_case([2048], [4096], 8, 2, 128, 16, seed=1, window=128)
    G = 4
    row = torch.arange(2048).unsqueeze(1) * G + (torch.arange(8) % G).unsqueeze(0)
    for m in (128, 32, 16):
        assert {int(k) for k in c.kind[row % m == 0]} == set(range(5)), m
    assert all(len({int(k) for k in c.kind[t, :G]}) == G for t in range(200, 300))
    # different frequency sets and V per kv head
    assert not torch.equal(c.q[:, :G], c.q[:, G:]) and not torch.equal(c.kc[:, :, 0], c.kc[:, :, 1])


def test_structured_profiles_stay_within_40_nats():
    for prof in F.PROFILES:
        for fp8 in (False, True):
            c = F.structured_case(prof, [64], [8192], 8, 1, 128, 16, seed=2, fp8=fp8)
            ks = c.ks if fp8 else 1.0
            K = c.kc[c.bt[0].long()].reshape(-1, 128).float() * ks
            s = (c.q[:, 0].float() @ K.t()) * c.scale
            assert float(s.abs().max()) <= 40.0, (prof, fp8, float(s.abs().max()))
            assert float(s.max() - s.min()) > 2 * F.PF_SLACK_NATS      # the running maximum has to move
