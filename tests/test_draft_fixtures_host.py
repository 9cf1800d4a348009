"""The contract of the margin-planted draft fixtures (oracle/draft_fixtures.py), checked on the CPU oracle alone: the
free oracle reproduces the planned tokens with >= 16 bf16 steps to the runner-up at every (row, head), the index edges
are among the targets, and each variant holds what its GPU tests rely on (test_gpu_draft_exact.py)."""
import math

import pytest
import torch

from oracle import draft_fixtures as F


def _rerun(fx, family, ids, hidden, k, **kw):
    return F.run_oracle(family, fx.ckpt, ids, hidden, k, **kw)


def _check_contract(fx, family, ids, hidden, k, fp8, margin=16, **kw):
    toks, logits = _rerun(fx, family, ids, hidden, k, fp8=fp8, **kw)
    assert torch.equal(toks, fx.tokens)
    skip = {(b, h): hi for b, h, _, hi in fx.ties}
    skip.update({(b, h): u for b, h, _, u, *_ in fx.bf16_pairs})
    B = ids.numel()
    for h in range(k):
        assert torch.equal(logits[h], fx.logits[h])
        for b in range(B):
            lg = logits[h][b].float().clone()
            t = int(toks[b, h])
            top = float(lg[t])
            lg[t] = -math.inf
            if (b, h) in skip:
                lg[skip[(b, h)]] = -math.inf
            second = float(lg.max())
            assert top - second >= margin * F.bf16_step(max(abs(top), abs(second))), (b, h, top, second)
    # distinct targets over the pairs that share an LM-head matrix
    for key in set(fx.head_keys):
        ts = [int(fx.tokens[b, h]) for h in range(k) if fx.head_keys[h] == key for b in range(B)]
        assert len(set(ts)) == len(ts)
    return logits


def _lstm(V, B, **kw):
    return F.lstm_fixture(V, 512, 768, B, **kw)


LSTM_KW = dict(n_predict=3, scale_input=True)


@pytest.mark.parametrize("V,B,fp8", [(3001, 1, False), (3001, 17, False), (50000, 33, False), (3001, 5, True),
                                     (50000, 32, True)])
def test_planted_free_oracle_and_margin(V, B, fp8):
    from arcticinference_amd.speculator import random_lstm_weights
    cfg, fx, ids, hidden = _lstm(V, B, fp8=fp8, seed=3)
    _check_contract(fx, "lstm", ids, hidden, 3, fp8, **LSTM_KW)
    # only the target rows moved; the background and every other tensor are the seeded random checkpoint's
    ck = random_lstm_weights(cfg, seed=3, std=0.05)
    moved = (fx.ckpt["head.0.weight"] != ck["head.0.weight"]).any(dim=1).nonzero().flatten().tolist()
    assert set(moved) == set(fx.tokens.flatten().tolist())
    assert all(torch.equal(fx.ckpt[n], ck[n]) for n in ck if n != "head.0.weight")


def test_edges_are_targets():
    cfg, fx, ids, hidden = _lstm(3001, 16, seed=5, tp=4)
    targets = set(fx.tokens.flatten().tolist())
    want = {0, 3000, 63, 64, 2943, 2944}                          # 3001 = 46 full blocks + 57 rows
    for s, e in F.shard_bounds(3001, 4):
        want |= {s, e - 1}
    assert want <= targets, want - targets
    assert set(fx.edges) <= targets
    # the full vocabulary: 2004 whole blocks
    assert {0, 128255, 63, 64, 128191, 128192} <= set(F.edge_targets(128256))


@pytest.mark.parametrize("tp", [1, 2, 4])
def test_negative_every_real_logit_below_zero(tp):
    cfg, fx, ids, hidden = _lstm(3001, 12, variant="negative", tp=tp, seed=6)
    logits = _check_contract(fx, "lstm", ids, hidden, 3, False, **LSTM_KW)
    for lg in logits:
        assert float(lg.float().max()) < 0
    # a zero column would have won every (row, head)
    assert all(float(fx.logits[h][b, int(fx.tokens[b, h])]) < 0 for h in range(3) for b in range(12))


@pytest.mark.parametrize("V,B,fp8,tp", [(50000, 20, False, 1), (50000, 7, True, 1), (3001, 10, False, 2),
                                        (3001, 10, False, 4)])
def test_exact_tie_bitwise_equal_lower_index(V, B, fp8, tp):
    cfg, fx, ids, hidden = _lstm(V, B, fp8=fp8, variant="exact_tie", tp=tp, seed=8)
    logits = _check_contract(fx, "lstm", ids, hidden, 3, fp8, **LSTM_KW)
    assert fx.ties and {h for _, h, _, _ in fx.ties} == {0, 1, 2}
    W = fx.ckpt["head.0.weight"]
    gaps = set()
    for b, h, lo, hi in fx.ties:
        assert lo < hi and int(fx.tokens[b, h]) == lo
        assert torch.equal(W[lo].view(torch.int16), W[hi].view(torch.int16))
        assert torch.equal(logits[h][b, lo].view(torch.int16), logits[h][b, hi].view(torch.int16))
        gaps.add(hi // F.BLOCK - lo // F.BLOCK)
    assert 0 in gaps and 1 in gaps and max(gaps) >= 3      # same block (epilogue), neighbouring and farther blocks
    if V > 256 * F.BLOCK * 2:
        assert {64, 256} <= gaps                            # other wave / same thread of the per-block arg-max
    if tp > 1:
        bounds = F.shard_bounds(V, tp)
        straddle = {(e - 1, e) for _, e in bounds[:-1]}
        assert straddle <= {(lo, hi) for _, _, lo, hi in fx.ties}


@pytest.mark.parametrize("V,B,tp", [(50000, 20, 1), (3001, 10, 2), (3001, 10, 4)])
def test_bf16_tie_rounds_equal_f32_ordered(V, B, tp):
    cfg, fx, ids, hidden = _lstm(V, B, variant="bf16_tie", tp=tp, seed=9)
    logits = _check_contract(fx, "lstm", ids, hidden, 3, False, **LSTM_KW)
    assert fx.bf16_pairs and {p[1] for p in fx.bf16_pairs} == {0, 1, 2}
    for b, h, t, u, ft, fu in fx.bf16_pairs:
        assert t < u and int(fx.tokens[b, h]) == t
        assert fu > ft                                          # the companion is larger before rounding
        assert torch.equal(logits[h][b, t].view(torch.int16), logits[h][b, u].view(torch.int16))
        m = float(logits[h][b, t])
        assert torch.tensor(ft).to(torch.bfloat16) == torch.tensor(fu).to(torch.bfloat16) == m
        st = F.bf16_step(m)
        for f in (ft, fu):                                      # >= 1/8 step from both rounding edges
            assert abs(f - m) <= st / 2 - st / 8, (f, m, st)
        # what a comparison before rounding would pick
        x = fx.states[h][b]
        W = fx.ckpt["head.0.weight"]
        assert float(x @ W[u].double()) > float(x @ W[t].double())


@pytest.mark.parametrize("kind", ["mlp_tied", "mlp_untied", "sum_rnn_stacked"])
@pytest.mark.parametrize("fp8", [False, True])
def test_other_families(kind, fp8):
    from arcticinference_amd.speculator import MLPSpeculatorConfig, random_mlp_weights
    V, H, Ds, k, B = 5003, 768, 512, 3, 12
    tie = kind != "mlp_untied"
    stacks = (1, 1, 1) if kind == "sum_rnn_stacked" else (0, 0, 0)
    mcfg = MLPSpeculatorConfig(vocab_size=V, emb_dim=H, inner_dim=Ds, n_predict=k, num_lookahead_tokens=k, tie_weights=tie,
                               scale_input=True)
    ck = random_mlp_weights(mcfg, seed=12, std=0.05)
    g = torch.Generator().manual_seed(13)
    F.add_sum_rnn_stacks(ck, stacks, tie, Ds, k, g)
    hidden = torch.randn(B, H, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, V, (B,), generator=g)
    kw = dict(n_predict=k, scale_input=True, tie=tie, stacks=stacks)
    fx = F.build_fixture("mlp", ck, ids, hidden, k, fp8=fp8, seed=14, **kw)
    assert fx.head_keys == (["head.0.weight"] * k if tie else [f"head.{h}.weight" for h in range(k)])
    _check_contract(fx, "mlp", ids, hidden, k, fp8, **kw)
    if not tie:                   # untied heads: targets distinct per matrix only, each matrix planted on its own head
        for h in range(k):
            assert not torch.equal(fx.ckpt[f"head.{h}.weight"], ck[f"head.{h}.weight"])


def test_fp8_fixture_is_measured_on_the_fp8_oracle():
    """Planting moves the per-tensor weight scale: the fixture holds on the fp8 path it was built for."""
    from arcticinference_amd.speculator import random_lstm_weights
    from oracle import spec_oracle as O
    cfg, fx, ids, hidden = _lstm(3001, 24, fp8=True, seed=15)
    _, s_before = O.fp8_quant_per_tensor(random_lstm_weights(cfg, seed=15, std=0.05)["head.0.weight"])
    _, s_after = O.fp8_quant_per_tensor(fx.ckpt["head.0.weight"])
    assert float(s_after) != float(s_before)
    _check_contract(fx, "lstm", ids, hidden, 3, True, **LSTM_KW)


# ---------------------------------------------------------------------------------------------------------------------
# full size: V 128256, Ds 4096, hidden 4096
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_ckpt():
    from arcticinference_amd.speculator import LSTMSpeculatorConfig, random_lstm_weights
    yield random_lstm_weights(LSTMSpeculatorConfig(vocab_size=128256, input_hidden_dim=4096), seed=4, std=0.02)


@pytest.mark.parametrize("B,fp8", [(64, False), (32, True)])
def test_full_size(full_ckpt, B, fp8):
    cfg, fx, ids, hidden = F.lstm_fixture(128256, 4096, 4096, B, fp8=fp8, ck=full_ckpt, seed=4)
    _check_contract(fx, "lstm", ids, hidden, 3, fp8, **LSTM_KW)
    assert {0, 128255, 63, 64} <= set(fx.tokens.flatten().tolist())


def test_oracle_embedding_add_keeps_the_fp32_alpha():
    """The oracle's `states + alpha * z` (torch.add / add_ with alpha in the reference) is ATen's GPU arithmetic: an fp32
    alpha in one fma, one bf16 rounding — what the kernels compute (r(fmaf(alpha, z, r(s)))).  torch on the CPU would
    round alpha to bf16 first (8.15719 -> 8.1875 at n_predict = 3, Ds = 512), moving ~40 % of the elements by a step."""
    from oracle import spec_oracle as O
    sw = 0.5 ** (0.5 / 3)
    alpha = math.sqrt((1 - sw ** 2) * (512 / 2)) / sw
    g = torch.Generator().manual_seed(0)
    a = torch.randn(4096, generator=g).to(torch.bfloat16)
    z = (torch.randn(4096, generator=g) * 0.05).to(torch.bfloat16)
    got = O.add_scaled(a, z, alpha)
    a32 = torch.tensor(alpha, dtype=torch.float32)
    assert float(a32) != float(a32.to(torch.bfloat16))
    # z * alpha32 is exact in f64 and a is a bf16 value: the f64 sum rounded to fp32 is the fma, then one bf16 rounding
    want = (a.double() + z.double() * float(a32)).to(torch.float32).to(torch.bfloat16)
    assert torch.equal(got, want)
    assert torch.equal(O.add_scaled(torch.zeros_like(z), z, alpha), (z.float() * a32).to(torch.bfloat16))
    assert not torch.equal(got, (a.double() + z.double() * float(a32.to(torch.bfloat16))).float().to(torch.bfloat16))


def test_oracle_norm_rsqrt_is_correctly_rounded():
    """MLPSpeculatorLayerNorm's rsqrt of the bf16 mean square, as ATen's fp32 opmath gives it on the GPU (and the kernels
    compute): the correctly rounded bf16 value.  torch's CPU rsqrt of a small bf16 tensor can be one or two steps off
    (rsqrt(1.1015625) -> 0.95703125 instead of 0.953125), scaling a whole row by up to 0.8 %."""
    from oracle import spec_oracle as O
    g = torch.Generator().manual_seed(31)
    x = (torch.randn(64, 1, 768, generator=g) * (0.8 + 0.4 * torch.rand(64, 1, 1, generator=g))).to(torch.bfloat16)
    ms = x.pow(2).mean(-1, keepdim=True) + 1e-6
    rs = (1.0 / ms.double().sqrt()).to(torch.bfloat16)                  # correctly rounded
    assert torch.equal(O._l2norm(x), x * rs)
