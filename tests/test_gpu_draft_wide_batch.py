"""Draft batches above 64 rows: the wide GEMMs (65..256 rows in one native call) and even chunks above that, pinned
EXACTLY on the margin-planted LM-head fixtures of oracle/draft_fixtures.py, like test_gpu_draft_exact.py does below 64.

Every case requires `torch.equal` tokens on every head of every row through generate_proposals and aic_lstm_propose, and
the bf16-rounded maximum logit beside each token within 1 bf16 step of the oracle's logit at that token (every case here
takes the bf16 head: padded batches above 32 rows do, whatever quantize_lm_head says).  The row counts sit on both sides
of every padded width (80 / 96 / 128 / 256 rows; 128- and 256-row activation tiles), the vocabularies end in a partly
valid 128-row block (3001, 50000, 8003, 5003), and K = 2048 walks the weight ring several times round."""
import pytest
import torch

from oracle import draft_fixtures as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_FIXTURES = {}


def _lstm_fixture(*a, **kw):
    """Fixtures are built once per argument set and never modified."""
    key = (a, tuple(sorted(kw.items())))
    if key not in _FIXTURES:
        _FIXTURES[key] = F.lstm_fixture(*a, **kw)
    return _FIXTURES[key]


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
# 1. row-count edges: both sides of 64 / 80 / 96 / 128 / 192 / 256 rows, a partly valid last block, many blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [3001, 50000])
@pytest.mark.parametrize("B", [65, 80, 96, 97, 128, 129, 192, 200, 256])
def test_lstm_row_count_edges_exact(V, B):
    cfg, fx, ids, hidden = _lstm_fixture(V, 512, 768, B, seed=7)
    m = _lstm_model(cfg, fx, 256, False)
    assert m.max_batch == 256 and m.capacity == 256
    _exact(m, fx, ids, hidden, False, f"V={V} B={B}")


@pytest.mark.parametrize("V", [3001, 50000])
def test_lstm_65_rows_quantized_head_takes_bf16_arithmetic(V):
    """quantize_lm_head=True serves padded batches up to 32 rows from the fp8 head; 65 rows must take the bf16 arithmetic:
    the fixture is the bf16 one and the values are held to it within 1 step."""
    cfg, fx, ids, hidden = _lstm_fixture(V, 512, 768, 65, seed=7)
    m = _lstm_model(cfg, fx, 256, True)
    _exact(m, fx, ids, hidden, False, f"V={V} B=65 quantize_lm_head")


@pytest.mark.parametrize("V", [3001, 50000])
def test_lstm_129_rows_with_hidden_index(V):
    """The engine's call form: a shuffled row index into a pool of 3 B hidden-state rows."""
    B = 129
    cfg, fx, ids, hidden = _lstm_fixture(V, 512, 768, B, seed=7)
    m = _lstm_model(cfg, fx, 256, False)
    g = torch.Generator().manual_seed(B)
    idx = torch.randperm(3 * B, generator=g)[:B]
    pool = torch.randn(3 * B, 768, generator=g).to(torch.bfloat16)
    pool[idx] = hidden
    idx_d = idx.to(torch.int32).to(DEV)
    toks, vals = _propose(m, pool.to(DEV), ids, B, 3, index=idx_d)
    assert torch.equal(toks, fx.tokens)
    _check_values(vals, fx, False, f"hidden_index V={V}")
    got = m.generate_proposals(ids.to(DEV), pool.to(DEV), 3, hidden_index=idx_d).cpu()
    assert torch.equal(got, fx.tokens)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a K loop longer than the weight register ring: K = 2048 is 64 k-steps (16 / 32 chunks at 128 / 256 padded rows)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [96, 256])
def test_lstm_long_k_loop_exact(B):
    cfg, fx, ids, hidden = _lstm_fixture(8003, 2048, 2048, B, seed=5)
    m = _lstm_model(cfg, fx, 256, False)
    _exact(m, fx, ids, hidden, False, f"K=2048 B={B}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. masking and ties at the new widths, on every draft schedule (head by head / fused)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,B", [("exact_tie", 129), ("exact_tie", 256), ("negative", 129), ("negative", 256),
                                       ("bf16_tie", 129)])
@pytest.mark.parametrize("V", [3001, 50000])
def test_lstm_ties_and_masking_wide(V, variant, B):
    """exact_tie: a target row copied bit for bit to a second index (the lowest index must win at every level: lane, wave,
    128-row block, the reduction over blocks); bf16_tie: a companion larger before rounding and equal after it; negative:
    every real logit is negative, so a zero-filled padded vocabulary row that got past the mask would win.  V = 3001 ends
    in a 57-row block of the wide head (7 zero-filled rows behind it), V = 50000 has 391 blocks, so tie partners meet in
    every level of the reduction over the per-block candidates.  (bf16_tie stops at 129 rows: the fixture generator cannot
    place its companion rows at 200 or 256.)"""
    N = _native()
    lib = N.lib()
    cfg, fx, ids, hidden = _lstm_fixture(V, 512, 768, B, variant=variant, seed=9)
    if variant == "negative":
        assert all(float(lg.float().max()) < 0 for lg in fx.logits)
    else:
        assert len(fx.ties + fx.bf16_pairs) > 0
    m = _lstm_model(cfg, fx, 256, False)
    _exact(m, fx, ids, hidden, False, f"V={V} {variant} B={B}")
    hid_d = hidden.to(DEV)
    try:
        lib.aic_debug_lstm_fused(0)          # head by head: the LM head alone, argmax_finish_kernel after every head
        toks, vals = _propose(m, hid_d, ids, B, 3)
    finally:
        lib.aic_debug_lstm_fused(1)
    assert torch.equal(toks, fx.tokens), (variant, B, "head by head")
    if variant == "negative":
        assert (toks < V).all() and (vals < 0).all()
    _check_values(vals, fx, False, f"{variant} B={B} head by head")


# ---------------------------------------------------------------------------------------------------------------------
# 4. vocab-parallel: two shards in one process, driven head by head
# ---------------------------------------------------------------------------------------------------------------------
def test_lstm_vocab_parallel_80_rows():
    from arcticinference_amd.speculator import ArcticLSTMSpeculator
    B, tp, k = 80, 2, 3
    cfg, fx, ids, hidden = _lstm_fixture(3001, 512, 768, B, tp=tp, seed=3)
    ranks = []
    for r in range(tp):
        m = ArcticLSTMSpeculator(cfg, max_num_seqs=256, tp_size=tp, tp_rank=r, device=DEV, quantize_lm_head=False)
        m.load_weights(fx.ckpt.items())
        ranks.append(m)
    assert sum(m.shard_rows for m in ranks) == cfg.vocab_size
    hid_d = hidden.to(DEV)
    for m in ranks:
        m.begin(hid_d, None, B)
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
    got, vals = torch.stack(toks, dim=1).cpu(), torch.stack(vals, dim=1).cpu()
    assert torch.equal(got, fx.tokens), (got != fx.tokens).nonzero().tolist()[:8]
    _check_values(vals, fx, False, "vocab-parallel B=80")


# ---------------------------------------------------------------------------------------------------------------------
# 5. MLP tied / untied and the stacked sum_rnn form
# ---------------------------------------------------------------------------------------------------------------------
def _sequential_names(ck):
    """The reference's nn.Sequential names: the base module of emb / proj / ln is index 0."""
    seq = {}
    for name, v in ck.items():
        parts = name.split(".")
        seq["speculator." + (".".join(parts[:2] + ["0"] + parts[2:]) if parts[0] in ("emb", "proj", "ln") and len(parts) == 3
                             else name)] = v
    return seq


@pytest.mark.parametrize("kind,B", [("mlp_tied", 80), ("mlp_tied", 200), ("mlp_untied", 80), ("mlp_untied", 200),
                                    ("sum_rnn_stacked", 80)])
def test_other_families_wide(kind, B):
    from arcticinference_amd.speculator import (ArcticMLPSpeculator, ArcticSumRNNSpeculator, LSTMSpeculatorConfig,
                                                MLPSpeculatorConfig, lstm_family_speculator, random_mlp_weights)
    V, H, Ds, k = 5003, 768, 512, 3
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
    fx = F.build_fixture("mlp", ck, ids, hidden, k, fp8=False, n_predict=k, scale_input=scale_input, tie=tie, stacks=stacks,
                         seed=14)
    if kind == "sum_rnn_stacked":
        dims = lambda n: ".".join([str(Ds)] * (n + 1))
        cfg = LSTMSpeculatorConfig(vocab_size=V, input_hidden_dim=H, inner_dim=dims(stacks[2]), emb_dim=dims(stacks[0]),
                                   proj_dim=dims(stacks[1]), n_predict=k, num_lookahead_tokens=k, tie_weights=tie,
                                   scale_input=scale_input, method="sum_rnn")
        m = lstm_family_speculator(cfg, max_num_seqs=256, device=DEV, quantize_lm_head=False)
        assert isinstance(m, ArcticSumRNNSpeculator) and m.stacks == stacks
        m.load_weights(_sequential_names(fx.ckpt).items())
    else:
        m = ArcticMLPSpeculator(mcfg, max_num_seqs=256, device=DEV, quantize_lm_head=False)
        m.load_weights(fx.ckpt.items())
    _exact(m, fx, ids, hidden, False, f"{kind} B={B}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. above the native cap: even chunks, all on the bf16 head
# ---------------------------------------------------------------------------------------------------------------------
def test_lstm_above_native_cap_is_chunked_evenly():
    from arcticinference_amd.speculator import draft_chunks
    B = 300
    cfg, fx, ids, hidden = _lstm_fixture(3001, 512, 768, B, seed=6)
    m = _lstm_model(cfg, fx, 300, True)
    assert m.capacity == 384 and m.max_batch == _native().lib().aic_lstm_max_rows() == 256
    hid_d = hidden.to(DEV)
    got = m.generate_proposals(ids.to(DEV), hid_d, 3).cpu()
    assert torch.equal(got, fx.tokens), (got != fx.tokens).nonzero().tolist()[:8]
    # the values of the calls generate_proposals made: within 1 bf16 step of the bf16 fixture, i.e. no chunk took the fp8 head
    sizes = draft_chunks(B, m.max_batch)
    assert sizes == [150, 150]
    toks, vals, lo = [], [], 0
    for n in sizes:
        t, v = _propose(m, hid_d[lo:lo + n], ids[lo:lo + n], n, 3)
        toks.append(t)
        vals.append(v)
        lo += n
    assert torch.equal(torch.cat(toks), fx.tokens)
    _check_values(torch.cat(vals), fx, False, "B=300 in two chunks")
    # with a row index the chunks index the caller's pool
    idx = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=DEV)
    got = m.generate_proposals(ids.to(DEV), hid_d.flip(0).contiguous(), 3, hidden_index=idx).cpu()
    assert torch.equal(got, fx.tokens)
    # one native call never takes more than the cap, and the capacity still bounds the batch
    with pytest.raises(_native().NativeError):
        _propose(m, hid_d, ids, B, 3)
    with pytest.raises(ValueError, match="exceeds max_num_seqs padding 384"):
        m.generate_proposals(torch.zeros(385, dtype=torch.int64, device=DEV),
                             torch.zeros(385, 768, dtype=torch.bfloat16, device=DEV), 3)


# ---------------------------------------------------------------------------------------------------------------------
# 7. a larger capacity does not change what a narrow batch computes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,fp8", [(64, False), (32, True)])
def test_capacity_does_not_change_narrow_results(B, fp8):
    cfg, fx, ids, hidden = _lstm_fixture(3001, 512, 768, B, fp8=fp8, seed=7)
    hid_d = hidden.to(DEV)
    out = []
    for max_num_seqs in (64, 256):
        m = _lstm_model(cfg, fx, max_num_seqs, fp8)
        out.append(_propose(m, hid_d, ids, B, 3) + (m.generate_proposals(ids.to(DEV), hid_d, 3).cpu(),))
        del m
    (t64, v64, g64), (t256, v256, g256) = out
    assert torch.equal(t64, fx.tokens) and torch.equal(g64, fx.tokens)
    assert torch.equal(t64, t256) and torch.equal(g64, g256)
    assert torch.equal(v64.view(torch.int32), v256.view(torch.int32))       # bit-identical values
    _check_values(v256, fx, fp8, f"capacity 256, B={B}")
