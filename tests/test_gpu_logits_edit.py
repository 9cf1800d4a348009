"""GPU: aic_logits_edit (ops.edit_logits) against the torch-CPU restatement of vLLM's logits edits
(tests/logits_edit_oracle.py), bit for bit (torch.equal on the f32 rows), on fixtures whose properties
tests/test_logits_edit_host.py checks on the CPU.

Shapes: V = 1000 (one ragged segment) and V = 2 S + 1004 for the kernel's segment size S (three segments, a ragged last
one, rows a multiple of 4 but not of 8 tokens long), rows 1 and 5; bf16 / fp16 / f32; gathered rows, rows picked by
`row_index` out of a taller matrix with an aligned row stride (16-byte loads) and with an odd one (scalar loads).
Planted histories: token 7 occurs 300 times in row 0's output (a count above 255); tokens 0, S - 1, S and V - 1 in the
outputs; token 11 in row 0's and row 1's prompt only (repetition applies, frequency and presence do not); row 1's
output is empty; prompts are padded with V; row 2's prompt is padding only.  Planted logits: 2.5, -1.25, 0 and -inf at
tokens 0 .. 3 of every row (token 3 also carries a bias in row 0: -inf stays -inf).  Repetition penalties 1.3, 0.8, 1,
1.5, 0.9; frequency and presence penalties of both signs.  min-p rows keep every token 1e-3 clear of the threshold; row
1 (min_p = 0) and row 2 (greedy) are not touched by it."""
import numpy as np
import pytest
import torch

import logits_edit_oracle as E
import sampler_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
_cache = {}


def _ops():
    from arcticinference_amd import ops
    return ops


def _fixture(V, rows):
    """One fixture and its expectations per shape: built once, shared, never written."""
    key = (V, rows)
    if key not in _cache:
        fx = E.build_fixture(V, rows, _ops().logits_edit_segment())
        _cache[key] = (fx, {case: fx.expected(case) for case in E.CASES})
    return _cache[key]


def _shapes():
    return E.shapes(E.segment_size())


def _csr(lists, with_values=None):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    tok = []
    for i, row in enumerate(lists):
        tok += list(row)
        off[i + 1] = len(tok)
    out = (torch.from_numpy(off).to(DEV), torch.tensor(tok, dtype=torch.int32, device=DEV))
    if with_values is not None:
        out += (torch.tensor([v for row in with_values for v in row], dtype=torch.float32, device=DEV),)
    return out


def _f32(values):
    return torch.tensor(values, dtype=torch.float32, device=DEV)


def _kwargs(fx, case):
    """The fixture as device arguments of ops.edit_logits, by plain loops (the plugin's packing is not used here)."""
    kw = {}
    if case in ("mask", "all"):
        kw["allowed_mask"] = fx.mask.to(DEV)
    if case in ("ban", "all"):
        kw["ban"] = _csr(fx.bans)
    if case in ("bias", "all"):
        dicts = [b or {} for b in fx.bias]
        kw["bias"] = _csr([list(d.keys()) for d in dicts], [list(d.values()) for d in dicts])
    if case in ("penalties", "all"):
        kw.update(prompt=_csr(fx.prompts), output=_csr(fx.outputs), repetition=_f32(fx.repetition),
                  frequency=_f32(fx.frequency), presence=_f32(fx.presence))
    if case in ("min_p", "all"):
        kw.update(min_p=_f32(fx.min_p), temperature=_f32(fx.temperature))
    return kw


def _place(logits, dtype, layout):
    """(device logits, row_index): the rows gathered, or scattered into a taller matrix whose row stride keeps the
    16-byte loads ("indexed") or breaks them ("unaligned": odd stride, base one element in)."""
    rows, V = logits.shape
    lg = logits.to(dtype)
    if layout == "gathered":
        return lg.to(DEV), None
    pad = 8 + (-V) % 8 if layout == "indexed" else 3 + (-V) % 2     # row stride a multiple of 8 elements / odd
    tall = torch.full((2 * rows + 3, V + pad), 1.0, dtype=dtype)
    idx = torch.randperm(tall.shape[0], generator=torch.Generator().manual_seed(rows + V))[:rows]
    first = 0 if layout == "indexed" else 1
    tall[idx, first:first + V] = lg
    return tall.to(DEV)[:, first:first + V], idx.to(DEV)


@pytest.mark.parametrize("layout", ["gathered", "indexed", "unaligned"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "f32"])
@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: f"V{s[0]}x{s[1]}")
def test_edited_rows_equal_the_oracle_bit_for_bit(shape, dtype, layout):
    fx, want = _fixture(*shape)
    lg, idx = _place(fx.logits, dtype, layout)
    before = lg.clone()
    for case in E.CASES:
        got = _ops().edit_logits(lg, row_index=idx, **_kwargs(fx, case))
        assert got.dtype == torch.float32 and got.shape == (fx.rows, fx.V) and got.is_contiguous()
        got = got.cpu()
        same = (got == want[case]) | (got.isnan() & want[case].isnan())
        assert torch.equal(got, want[case]), (case, int((~same).sum()), (~same).nonzero()[:5].tolist())
    assert torch.equal(lg, before)                       # the raw rows are only read


@pytest.mark.parametrize("shape", _shapes()[1::2], ids=lambda s: f"V{s[0]}x{s[1]}")
def test_the_planted_cases_are_what_the_docstring_says(shape):
    """The expectations themselves carry the planted properties (so a kernel that equals them has met each one)."""
    fx, want = _fixture(*shape)
    S, V = fx.segment, fx.V
    pen = want["penalties"]
    raw = fx.logits
    # row 0, token 7: 300 occurrences: x * (1 / 1.3 or 1.3) - 0.5 * 300 - 0.25
    x = raw[0, 7]
    rep = torch.tensor(1.3)
    scaled = x * (1.0 / rep) if x > 0 else x * rep
    assert pen[0, 7] == (scaled - torch.tensor(0.5) * 300) - torch.tensor(0.25)
    # token 11 is in row 0's prompt only: repetition alone
    if 11 not in fx.outputs[0]:
        x = raw[0, 11]
        assert pen[0, 11] == (x * (1.0 / rep) if x > 0 else x * rep)
    # -inf stays -inf through bias and penalties; the edge tokens were counted
    assert want["all"][0, 3] == float("-inf") and want["bias"][0, 3] == float("-inf")
    for t in (0, S - 1, S, V - 1):
        if t < V:
            assert pen[0, t] != raw[0, t]
    # an empty output: row 1 changes only where its prompt has a token
    changed = (pen[1] != raw[1]).nonzero().flatten().tolist()
    assert changed and set(changed) <= set(fx.prompts[1])
    # row 2: penalties 1 / 0 / 0 change nothing
    assert torch.equal(pen[2], raw[2])
    # min-p leaves rows 1 (min_p = 0) and 2 (greedy) alone and cuts the others
    mp = want["min_p"]
    assert torch.equal(mp[1], raw[1]) and torch.equal(mp[2], raw[2])
    for r in (0, 3, 4):
        assert 1 <= int((mp[r] != float("-inf")).sum()) < int((raw[r] != float("-inf")).sum())


def test_min_p_kept_sets_equal_the_f64_evaluation():
    for shape in _shapes():
        fx, want = _fixture(*shape)
        lg, _ = _place(fx.logits, torch.bfloat16, "gathered")
        for case in ("min_p", "all"):
            got = _ops().edit_logits(lg, **_kwargs(fx, case)).cpu()
            d = E.min_p_distance(E.edit(fx.logits, **fx.oracle_kwargs(case)), fx.min_p, fx.temperature)
            edited = E.edit(fx.logits, **fx.oracle_kwargs(case))
            kept = (d >= 0) & (edited != float("-inf")).numpy()
            assert ((got != float("-inf")).numpy() == kept).all(), (shape, case)


def test_edit_then_sample_equals_the_sampler_oracle_on_the_oracles_rows():
    """A mixed greedy / temperature / top-k / top-p batch: ops.sample_tokens on the rows ops.edit_logits returns against
    tests/sampler_oracle.py on the oracle's edited rows.  p is the first of a fixed list that keeps every ascending
    cumulative sum 5e-3 clear of 1 - p on the edited row, and the noise is redrawn until the f64 winner leads by 1e-4
    (the sampler fixtures' own two properties)."""
    V, rows = _shapes()[1]
    fx, want = _fixture(V, rows)
    edited = want["all"]
    temps = fx.temperature                      # row 2 greedy
    ks = [0, 40, 5, 0, 12]
    ps = []
    for r in range(rows):
        if temps[r] <= 0 or r == 0:
            ps.append(1.0)                      # row 0: temperature only
            continue
        x = O.scaled_f32(edited[r], temps[r])
        ps.append(next(p for p in (0.9, 0.8, 0.7, 0.6, 0.5, 0.95, 0.4) if O.cumsums_clear(x, ks[r] or V, p)))
    g = torch.Generator().manual_seed(3)
    q = torch.empty(rows, V).exponential_(generator=g)
    for r in range(rows):
        if temps[r] <= 0:
            continue
        for _ in range(50):
            if O.winner_margin(O.probs_f64(edited[r], temps[r], ks[r] or V, ps[r]), q[r])[1] >= O.WINNER_MARGIN:
                break
            q[r] = torch.empty(V).exponential_(generator=g)
        else:
            raise RuntimeError("no noise row with a clear winner")
    lg, idx = _place(fx.logits, torch.bfloat16, "indexed")
    rows_f32 = _ops().edit_logits(lg, row_index=idx, **_kwargs(fx, "all"))
    got = _ops().sample_tokens(rows_f32, _f32(temps), q.to(DEV), top_k=torch.tensor(ks, dtype=torch.int32, device=DEV),
                               top_p=_f32(ps)).cpu()
    assert torch.equal(got, O.sample_literal(edited, temps, ks, ps, q)), got.tolist()
    # the greedy row is the arg-max of its EDITED row: its raw maximum (22) is banned
    assert got[2] == edited[2].argmax() == 40 and fx.logits[2].argmax() == 22


def test_the_call_is_capturable_and_replays_over_new_inputs():
    V, rows = _shapes()[3]
    fx, want = _fixture(V, rows)
    kw = _kwargs(fx, "all")
    lg = torch.empty(rows, V, dtype=torch.bfloat16, device=DEV)
    # three inputs over the same buffers: the fixture, the fixture with another row's histories and penalties, and one
    # without penalties at all (repetition 1, frequency 0, presence 0)
    variants = [dict(logits=fx.logits, rep=fx.repetition, freq=fx.frequency),
                dict(logits=fx.logits.flip(0).contiguous(), rep=fx.repetition, freq=[-f for f in fx.frequency]),
                dict(logits=fx.logits, rep=[1.0] * rows, freq=[0.0] * rows)]

    def load(v):
        lg.copy_(v["logits"].to(torch.bfloat16))
        kw["repetition"].copy_(torch.tensor(v["rep"]))
        kw["frequency"].copy_(torch.tensor(v["freq"]))

    def expect(v):
        ok = fx.oracle_kwargs("all")
        ok.update(repetition=v["rep"], frequency=v["freq"])
        return E.apply_min_p(E.edit(v["logits"], **ok), fx.min_p, fx.temperature)

    load(variants[0])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _ops().edit_logits(lg, **kw)                       # warm-up: the workspace of this stream exists
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = _ops().edit_logits(lg, **kw)
    for i in (1, 2, 0):
        load(variants[i])
        graph.replay()
        torch.cuda.synchronize()
        # the flipped logits may put a token near the min-p threshold: compare outside the margin only
        w = expect(variants[i])
        ok = fx.oracle_kwargs("all")
        ok.update(repetition=variants[i]["rep"], frequency=variants[i]["freq"])
        clear = torch.from_numpy(np.abs(E.min_p_distance(E.edit(variants[i]["logits"], **ok), fx.min_p, fx.temperature))
                                 >= E.MIN_P_MARGIN)
        got = out.cpu()
        assert clear.float().mean() > 0.99
        assert torch.equal(torch.where(clear, got, torch.zeros(())), torch.where(clear, w, torch.zeros(()))), i


def test_no_rows_no_edits_and_refusals_before_any_launch():
    ops = _ops()
    V = 1000
    lg = torch.randn(4, V, device=DEV).to(torch.bfloat16)
    # no edit input at all: the f32 copy of the rows
    assert torch.equal(ops.edit_logits(lg), lg.float())
    assert ops.edit_logits(lg[:0]).shape == (0, V)
    assert ops.edit_logits(lg, row_index=torch.empty(0, dtype=torch.int64, device=DEV)).shape == (0, V)
    off = torch.zeros(5, dtype=torch.int32, device=DEV)
    tok = torch.zeros(0, dtype=torch.int32, device=DEV)
    f = torch.ones(4, device=DEV)
    # empty lists are nobody's edits
    assert torch.equal(ops.edit_logits(lg, ban=(off, tok), bias=(off, tok, tok.float()), prompt=(off, tok), output=(off, tok)),
                       lg.float())
    for kw in (dict(min_p=f), dict(ban=(off.long(), tok)), dict(ban=(off[:4], tok)), dict(bias=(off, tok)),
               dict(allowed_mask=torch.zeros(4, V, device=DEV)), dict(allowed_mask=torch.zeros(3, V, dtype=torch.bool, device=DEV)),
               dict(repetition=f.double()), dict(frequency=f[:3]), dict(row_index=torch.zeros(2, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            ops.edit_logits(lg, **kw)
    with pytest.raises(ValueError):
        ops.edit_logits(lg.double())
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.edit_logits(lg, repetition=torch.ones(4))
    # the C entry point refuses min_p without temperature itself
    from arcticinference_amd import _native as N
    out = torch.empty(4, V, device=DEV)
    rc = N.lib().aic_logits_edit(lg.data_ptr(), N.DT_BF16, V, V, None, 4, None, None, None, 0, None, None, None, 0, None,
                                 None, 0, None, None, 0, None, None, None, f.data_ptr(), None, out.data_ptr(), None, None)
    assert rc == N.AIC_ERR_INVALID
    rc = N.lib().aic_logits_edit(lg.data_ptr(), N.DT_FP8_E4M3, V, V, None, 4, None, None, None, 0, None, None, None, 0,
                                 None, None, 0, None, None, 0, None, None, None, None, None, out.data_ptr(), None, None)
    assert rc == N.AIC_ERR_UNSUPPORTED
    torch.cuda.synchronize()
