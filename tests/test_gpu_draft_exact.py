"""Draft-model tokens pinned EXACTLY (A8-A11) on margin-planted LM-head fixtures (oracle/draft_fixtures.py).

Every case requires the kernel's tokens to equal the CPU op-sequence oracle's on every head of every row
(`torch.equal`, no teacher forcing), and the bf16-rounded maximum logit returned beside each token to be within
1 bf16 step (bf16 head) / 4 steps (fp8 head) of the oracle's logit at that token.  The fixtures plant the target rows so
that each target wins by >= 16 bf16 steps; the exact-tie fixtures copy a target row bit for bit to a second index (the
lowest index must win at every level of the arg-max); the bf16-tie fixtures put a companion row whose logit is larger
before rounding and equal after it above the target (the comparison is on bf16-ROUNDED logits); the negative fixtures make
every real logit negative, so an unmasked zero-filled padded column would win.  The random-weight tests in
test_gpu_kernels.py stay as the near-tie probe."""
import pytest
import torch

from oracle import draft_fixtures as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _native():
    from arcticinference_amd import _native as N
    return N


def _check_values(vals, fx, fp8, tag):
    """The returned maximum logit against the oracle's logit at the expected token: 1 bf16 step (bf16 head), 4 (fp8 head:
    one bf16 ulp in an activation can flip its e4m3 code)."""
    ulps = 4 if fp8 else 1
    B, k = fx.tokens.shape
    for b in range(B):
        for h in range(k):
            ref = fx.value(b, h)
            assert abs(float(vals[b, h]) - ref) <= max(abs(ref), 1e-3) * 2 ** -7 * ulps, (tag, b, h, float(vals[b, h]), ref)


def _propose(m, hidden_d, ids, B, k, index=None):
    """aic_lstm_propose, the engine's whole-draft entry point: (tokens, bf16-rounded maximum logits)."""
    N = _native()
    toks = torch.full((B, k), -1, dtype=torch.int64, device=DEV)
    vals = torch.full((B, k), float("nan"), dtype=torch.float32, device=DEV)
    ids_d = ids.to(torch.int32).to(DEV)
    N.check(N.lib().aic_lstm_propose(m._h, hidden_d.data_ptr(), None if index is None else index.data_ptr(),
                                     ids_d.data_ptr(), B, k, toks.data_ptr(), vals.data_ptr(), N.current_stream_ptr()))
    torch.cuda.synchronize()
    return toks.cpu(), vals.cpu()


def _lstm_model(cfg, fx, max_num_seqs, fp8, **kw):
    from arcticinference_amd.speculator import ArcticLSTMSpeculator
    m = ArcticLSTMSpeculator(cfg, max_num_seqs=max_num_seqs, device=DEV, quantize_lm_head=fp8, **kw)
    m.load_weights(fx.ckpt.items())
    return m


def _exact(m, fx, ids, hidden, fp8, tag):
    """generate_proposals and aic_lstm_propose: tokens equal to the oracle's, values within the head's steps."""
    B, k = fx.tokens.shape
    hid_d = hidden.to(DEV)
    got = m.generate_proposals(ids.to(DEV), hid_d, k).cpu()
    assert torch.equal(got, fx.tokens), (tag, (got != fx.tokens).nonzero().tolist()[:8])
    toks, vals = _propose(m, hid_d, ids, B, k)
    assert torch.equal(toks, fx.tokens), (tag, "propose")
    _check_values(vals, fx, fp8, tag)


# ---------------------------------------------------------------------------------------------------------------------
# LSTM at the 8B speculator's size (V 128256, Ds = hidden = 4096)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_ckpt():
    from arcticinference_amd.speculator import LSTMSpeculatorConfig, random_lstm_weights
    yield random_lstm_weights(LSTMSpeculatorConfig(vocab_size=128256, input_hidden_dim=4096), seed=4, std=0.02)


@pytest.mark.parametrize("B,fp8,with_index", [(8, False, False), (64, False, False), (8, True, True), (32, True, False)])
def test_lstm_full_size_exact(full_ckpt, B, fp8, with_index):
    """bf16 head at 8 and 64 rows, fp8 e4m3 head at 8 and 32 rows (the widest batch that takes it); the 8-row fp8 case
    also through aic_lstm_propose with a hidden-state row index (the engine's call form)."""
    cfg, fx, ids, hidden = F.lstm_fixture(128256, 4096, 4096, B, fp8=fp8, ck=full_ckpt, seed=4)
    m = _lstm_model(cfg, fx, B, fp8)
    assert (m.quantize_lm_head and fp8) or not fp8
    _exact(m, fx, ids, hidden, fp8, f"full size B={B} fp8={fp8}")
    if with_index:
        g = torch.Generator().manual_seed(B)
        idx = torch.randperm(3 * B, generator=g)[:B]
        pool = torch.randn(3 * B, 4096, generator=g).to(torch.bfloat16)
        pool[idx] = hidden
        toks, vals = _propose(m, pool.to(DEV), ids, B, 3, index=idx.to(torch.int32).to(DEV))
        assert torch.equal(toks, fx.tokens)
        _check_values(vals, fx, fp8, "hidden_index")


# ---------------------------------------------------------------------------------------------------------------------
# odd small shapes: partly valid last block (3001), many blocks (50000), the padded-batch edges at 16 / 32 / 64
# ---------------------------------------------------------------------------------------------------------------------
_SMALL = [(V, B, False) for V in (3001, 50000) for B in (1, 5, 16, 17, 33, 64)] + \
         [(3001, 5, True), (50000, 17, True), (3001, 32, True), (3001, 33, True), (50000, 33, True)]


@pytest.mark.parametrize("V,B,quantize", _SMALL)
def test_lstm_small_shapes_exact(V, B, quantize):
    """`quantize` = quantize_lm_head: the fp8 head serves padded batches up to 32 rows; B = 33 (64 padded) must take the
    bf16 arithmetic (head_fp8_max_batch = 32, speculator.py): its values are held to the bf16 oracle's within 1 step."""
    fp8 = quantize and B <= 32
    cfg, fx, ids, hidden = F.lstm_fixture(V, 512, 768, B, fp8=fp8, seed=7)
    m = _lstm_model(cfg, fx, 64, quantize)
    _exact(m, fx, ids, hidden, fp8, f"V={V} B={B} quantize={quantize}")


# ---------------------------------------------------------------------------------------------------------------------
# MLP tied / untied and stacked sum_rnn
# ---------------------------------------------------------------------------------------------------------------------
def _sequential_names(ck):
    """The reference's nn.Sequential names: the base module of emb / proj / ln is index 0."""
    seq = {}
    for name, v in ck.items():
        parts = name.split(".")
        seq["speculator." + (".".join(parts[:2] + ["0"] + parts[2:]) if parts[0] in ("emb", "proj", "ln") and len(parts) == 3
                             else name)] = v
    return seq


@pytest.mark.parametrize("kind", ["mlp_tied", "mlp_untied", "sum_rnn_stacked"])
@pytest.mark.parametrize("fp8", [False, True])
def test_other_families_exact(kind, fp8):
    from arcticinference_amd.speculator import (ArcticMLPSpeculator, ArcticSumRNNSpeculator, LSTMSpeculatorConfig,
                                                MLPSpeculatorConfig, lstm_family_speculator, random_mlp_weights)
    V, H, Ds, k, B = 5003, 768, 512, 3, 12
    tie = kind != "mlp_untied"
    stacks = (1, 1, 1) if kind == "sum_rnn_stacked" else (0, 0, 0)
    scale_input = kind != "mlp_tied"
    mcfg = MLPSpeculatorConfig(vocab_size=V, emb_dim=H, inner_dim=Ds, n_predict=k, num_lookahead_tokens=k, tie_weights=tie,
                               scale_input=scale_input)
    ck = random_mlp_weights(mcfg, seed=12, std=0.05)
    g = torch.Generator().manual_seed(13)
    F.add_sum_rnn_stacks(ck, stacks, tie, Ds, k, g)
    hidden = torch.randn(B, H, generator=g).to(torch.bfloat16)
    ids = torch.randint(0, V, (B,), generator=g)
    fx = F.build_fixture("mlp", ck, ids, hidden, k, fp8=fp8, n_predict=k, scale_input=scale_input, tie=tie, stacks=stacks,
                         seed=14)
    assert len(set(fx.head_keys)) == (1 if tie else k)
    if kind == "sum_rnn_stacked":
        dims = lambda n: ".".join([str(Ds)] * (n + 1))
        cfg = LSTMSpeculatorConfig(vocab_size=V, input_hidden_dim=H, inner_dim=dims(stacks[2]), emb_dim=dims(stacks[0]),
                                   proj_dim=dims(stacks[1]), n_predict=k, num_lookahead_tokens=k, tie_weights=tie,
                                   scale_input=scale_input, method="sum_rnn")
        m = lstm_family_speculator(cfg, max_num_seqs=16, device=DEV, quantize_lm_head=fp8)
        assert isinstance(m, ArcticSumRNNSpeculator) and m.stacks == stacks
        m.load_weights(_sequential_names(fx.ckpt).items())
    else:
        m = ArcticMLPSpeculator(mcfg, max_num_seqs=16, device=DEV, quantize_lm_head=fp8)
        m.load_weights(fx.ckpt.items())
    _exact(m, fx, ids, hidden, fp8, f"{kind} fp8={fp8}")


# ---------------------------------------------------------------------------------------------------------------------
# every LSTM draft schedule against the ORACLE: head by head / fused / fused + on-the-fly fp8 quantisation, x one or
# three cell launches, on planted, exact-tie and bf16-tie fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,fp8,B", [("exact", False, 40), ("exact", True, 20), ("exact_tie", False, 40),
                                            ("exact_tie", True, 7), ("exact_tie", False, 64), ("bf16_tie", False, 20),
                                            ("bf16_tie", False, 64)])
def test_lstm_every_schedule_exact(variant, fp8, B):
    """V = 50000: 782 head blocks, so the tie partners sit in neighbouring lanes, other waves and the same thread of the
    arg-max over the per-block partials (argmax_finish_kernel, and block_argmax inside the next cell launch), and in the
    same lane / other lanes / other waves of the GEMM epilogue.  Ties sit at every head; a bf16-tie companion sits in the
    same block or another one."""
    N = _native()
    lib = N.lib()
    cfg, fx, ids, hidden = F.lstm_fixture(50000, 512, 768, B, fp8=fp8, variant=variant, seed=21)
    if variant != "exact":
        assert {p[1] for p in fx.ties + fx.bf16_pairs} == {0, 1, 2}
    m = _lstm_model(cfg, fx, 64, fp8)
    hid_d = hidden.to(DEV)
    try:
        for mode in (0, 1, 2):
            for cell_launches in (1, 3):
                lib.aic_debug_lstm_fused(mode)
                lib.aic_debug_lstm_cell_launches(cell_launches)
                toks, vals = _propose(m, hid_d, ids, B, 3)
                tag = f"{variant} fp8={fp8} B={B} fused={mode} cell_launches={cell_launches}"
                assert torch.equal(toks, fx.tokens), (tag, (toks != fx.tokens).nonzero().tolist()[:8])
                _check_values(vals, fx, fp8, tag)
    finally:
        lib.aic_debug_lstm_fused(1)
        lib.aic_debug_lstm_cell_launches(1)


# ---------------------------------------------------------------------------------------------------------------------
# negative logits (padded columns must stay masked) and ties across vocab shards
# ---------------------------------------------------------------------------------------------------------------------
def _vocab_parallel(cfg, ck, tp, hidden_d, ids, B, k):
    """The vocab-parallel loop of generate_proposals with the all-gather emulated by a stack (all ranks on this GPU):
    (tokens, value of the picked (value, index) pair)."""
    from arcticinference_amd.speculator import ArcticLSTMSpeculator
    ranks = []
    for r in range(tp):
        m = ArcticLSTMSpeculator(cfg, max_num_seqs=64, tp_size=tp, tp_rank=r, device=DEV, quantize_lm_head=False)
        m.load_weights(ck.items())
        ranks.append(m)
    assert sum(m.shard_rows for m in ranks) == cfg.vocab_size
    for m in ranks:
        m.begin(hidden_d, None, B)
    last = ids.to(torch.int32).to(DEV)
    toks, vals = [], []
    for head in range(k):
        parts = []
        for m in ranks:
            tok, val = m.head_step(head, last, B)
            parts.append(torch.stack([val.to(torch.float64).view(torch.int64), tok]))
        gathered = torch.stack(parts)
        nxt = ArcticLSTMSpeculator.pick_global(gathered)
        v = gathered[:, 0, :].contiguous().view(torch.float64)
        vals.append(v.gather(0, torch.argmax(v, dim=0, keepdim=True)).reshape(-1))
        toks.append(nxt)
        last = nxt.to(torch.int32)
    return torch.stack(toks, dim=1).cpu(), torch.stack(vals, dim=1).cpu()


@pytest.mark.parametrize("fp8", [False, True])
def test_lstm_negative_logits_single_rank(fp8):
    """V = 3001: 7 zero-filled rows in the last head block.  Every real logit is negative, so a zero column that got
    past the epilogue's n < n_valid_rows test would win."""
    cfg, fx, ids, hidden = F.lstm_fixture(3001, 512, 768, 9, fp8=fp8, variant="negative", seed=31)
    assert all(float(lg.float().max()) < 0 for lg in fx.logits)
    m = _lstm_model(cfg, fx, 16, fp8)
    got = m.generate_proposals(ids.to(DEV), hidden.to(DEV), 3).cpu()
    assert (got < 3001).all() and torch.equal(got, fx.tokens), got
    toks, vals = _propose(m, hidden.to(DEV), ids, 9, 3)
    assert torch.equal(toks, fx.tokens) and (vals < 0).all()
    _check_values(vals, fx, fp8, "negative")


@pytest.mark.parametrize("tp", [2, 4])
def test_lstm_negative_logits_vocab_parallel(tp):
    """Every shard of V = 3001 over 2 / 4 ranks ends in a partly valid block (1504 / 1497 rows; 752 / 745 rows)."""
    B = 10
    cfg, fx, ids, hidden = F.lstm_fixture(3001, 512, 512, B, variant="negative", tp=tp, seed=32 + tp)
    got, vals = _vocab_parallel(cfg, fx.ckpt, tp, hidden.to(DEV), ids, B, 3)
    assert (got < 3001).all() and torch.equal(got, fx.tokens), (tp, got)
    assert (vals < 0).all()
    _check_values(vals, fx, False, f"negative tp={tp}")


@pytest.mark.parametrize("variant", ["exact_tie", "bf16_tie"])
@pytest.mark.parametrize("tp", [2, 4])
def test_lstm_ties_across_vocab_shards(variant, tp):
    """The first tie pairs straddle two shards (last real row of rank r, first row of rank r + 1): both ranks report the
    same bf16 value (bf16_tie: the upper rank's logit is larger before rounding) and pick_global must take the lower rank,
    i.e. the lower index."""
    B = 10
    cfg, fx, ids, hidden = F.lstm_fixture(3001, 512, 512, B, variant=variant, tp=tp, seed=40 + tp)
    bounds = F.shard_bounds(3001, tp)
    pairs = [p[:4] for p in fx.ties + fx.bf16_pairs]
    straddling = [(lo, hi) for _, _, lo, hi in pairs if any(lo == e - 1 and hi == e for _, e in bounds[:-1])]
    assert len(straddling) == tp - 1, pairs
    got, vals = _vocab_parallel(cfg, fx.ckpt, tp, hidden.to(DEV), ids, B, 3)
    assert torch.equal(got, fx.tokens), (variant, tp, got, fx.tokens)
    _check_values(vals, fx, False, f"{variant} tp={tp}")
    # and the single rank agrees
    m = _lstm_model(cfg, fx, 16, False)
    assert torch.equal(m.generate_proposals(ids.to(DEV), hidden.to(DEV), 3).cpu(), fx.tokens)
