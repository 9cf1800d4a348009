"""CPU: the host half of the grouped shared-prefix attention call (aic_verify_attention_prefix_groups).

  * the grouped marked-key probe of tests/prefix_group_fixtures.py: the oracle returns its closed form, and a reference
    that drops the marked key, or counts it twice, moves every concerned row by at least ten times the bar — so the GPU
    test that uses the probe at each group's seam cannot pass with either fault;
  * runner_logic.prefix_groups, the plugin's decision, on hand-made block tables;
  * ops.PrefixGroups and ops.verify_attention's argument rules, which are answered before the device check;
  * the header declares the entry points, the built library exports them and answers its argument rules without a device;
  * step_context.publish keeps its two-argument form."""
import os

import numpy as np
import pytest
import torch

import attention_fixtures as F
import prefix_group_fixtures as PG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ_GROUP, GROUP_LEN, Q_LENS, CTXS = PG.SEAM_REQ_GROUP, PG.SEAM_GROUP_LEN, PG.SEAM_Q_LENS, PG.SEAM_CTXS
SEAM_KEYS = PG.SEAM_KEYS


@pytest.mark.parametrize("t", SEAM_KEYS)
def test_grouped_marked_key_probe_closed_form_and_mutants(t):
    c = PG.grouped_marked_case(t, Q_LENS, CTXS, Hq=4, Hkv=2, D=64, bs=16, req_group=REQ_GROUP, group_len=GROUP_LEN)
    assert max(CTXS) <= 92 and sorted(SEAM_KEYS) == sorted([p - 1 for p in GROUP_LEN] + GROUP_LEN)
    assert any(cx - ql == GROUP_LEN[g] for ql, cx, g in zip(Q_LENS, CTXS, REQ_GROUP) if g >= 0)
    # the pages: members share their leader's below the group's length and nothing else; the loner shares nothing
    for i, g in enumerate(REQ_GROUP):
        for j in range(i):
            n = GROUP_LEN[g] // 16 if g >= 0 and REQ_GROUP[j] == g else 0
            assert torch.equal(c.bt[i, :n], c.bt[j, :n])
            rest_i, rest_j = c.bt[i, n:(CTXS[i] + 15) // 16], c.bt[j, n:(CTXS[j] + 15) // 16]
            assert not set(rest_i.tolist()) & set(rest_j.tolist())
    want = F.oracle(c)
    assert torch.allclose(want, c.expected, atol=1e-6, rtol=1e-5)
    assert torch.allclose(PG.marked_reference(c).float(), c.expected, atol=1e-6, rtol=1e-5)
    concerned = c.pos >= t
    assert concerned.any()
    for g in range(len(GROUP_LEN)):        # every group has a concerned row of its own
        rows = torch.cat([torch.full((q,), REQ_GROUP[i]) for i, q in enumerate(Q_LENS)])
        assert (concerned & (rows == g)).any() or t >= GROUP_LEN[g]
    for w in (0.0, 2.0):                   # key t dropped / counted twice
        moved = (PG.marked_reference(c, w) - c.expected.double()).abs()
        floor = 10.0 * PG.bar(c.expected.double())
        assert bool((moved[concerned] >= floor[concerned]).all()), (t, w, float(moved[concerned].min()))
        assert float(moved[~concerned].max()) == 0.0


def test_share_in_groups_shares_pages_per_group():
    c0 = F.planted_case([1, 3, 2, 1], [100, 90, 20, 110], 4, 1, 128, 16, seed=5)
    before = c0.bt.clone()
    c = PG.share_in_groups(c0, [0, 1, -1, 0], [64, 70])
    assert c.leader == [0, 1]
    assert torch.equal(c.bt[3, :4], c.bt[0, :4]) and not torch.equal(c.bt[3, 4:6], c.bt[0, 4:6])
    assert torch.equal(c.bt[1], before[1]) and torch.equal(c.bt[2], before[2]) and torch.equal(c.bt[0], before[0])
    with pytest.raises(AssertionError):
        PG.share_in_groups(F.planted_case([1, 30], [100, 90], 4, 1, 128, 16, seed=5), [0, 0], [64])   # 90 - 30 < 64


# ---- the plugin's decision ------------------------------------------------------------------------------------------
@pytest.fixture
def floor_thresholds(monkeypatch):
    from arcticinference_amd.vllm_plugin import runner_logic as R
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_LEN", 32)
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_ITEMS", 1)
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_ITEMS_FP8", 1)
    monkeypatch.setattr(R, "PREFIX_GROUPS_MIN_MEMBERS", 2)
    monkeypatch.setattr(R, "PREFIX_GROUPS_MIN_MEMBERS_FP8", 2)
    monkeypatch.setattr(R, "PREFIX_GROUPS_MAX_SUFFIX_FRACTION", 1.0)
    monkeypatch.setattr(R, "PREFIX_GROUPS_MAX_SUFFIX_FRACTION_FP8", 1.0)
    monkeypatch.setattr(R, "PREFIX_GROUPS_MAX_LEN_SPREAD_FP8", 1 << 30)
    return R


def _table(rows, width=8):
    bt = np.zeros((len(rows), width), dtype=np.int32)
    for i, r in enumerate(rows):
        bt[i, :len(r)] = r
    return bt


def test_prefix_groups_two_groups_and_a_loner(floor_thresholds):
    R = floor_thresholds
    # pages of 16; members not adjacent in batch order: A B - A B A
    bt = _table([[1, 2, 3, 4, 50], [10, 11, 12, 13, 14, 15, 60], [70, 71], [1, 2, 3, 4, 51], [10, 11, 12, 13, 14, 15, 61],
                 [1, 2, 3, 4, 52]])
    computed = np.array([70, 100, 20, 75, 105, 66])
    got = R.prefix_groups(bt, computed, [1, 4, 2, 3, 9, 1], 16, 4, False)
    assert got is not None
    req_group, lens = got
    assert req_group.tolist() == [0, 1, -1, 0, 1, 0] and lens == [64, 96]       # largest group first
    # a group capped by its members' smallest computed-token count: request 4 has only 70 tokens in the cache
    computed[4] = 70
    assert R.prefix_groups(bt, computed, [1, 4, 2, 3, 9, 1], 16, 4, False)[1] == [64, 70]
    # unused columns are zero in every row: they never lengthen a group past what is computed
    same = _table([[1, 2], [1, 2], [1, 2]])
    assert R.prefix_groups(same, np.array([32, 40, 33]), [1, 1, 1], 16, 4, False)[1] == [32]
    # a request with fewer computed tokens than the shortest prefix served is in no group
    got = R.prefix_groups(same, np.array([32, 40, 31]), [1, 1, 1], 16, 4, False)
    assert got[0].tolist() == [0, 0, -1] and got[1] == [32]


def test_prefix_groups_floors_caps_and_refusals(floor_thresholds, monkeypatch):
    R = floor_thresholds
    bt = _table([[1, 2, 3], [1, 2, 3], [7, 8, 9]])
    computed, ql = np.array([48, 48, 48]), [1, 1, 1]
    assert R.prefix_groups(bt, computed, ql, 16, 4, False)[0].tolist() == [0, 0, -1]     # a bucket of one: below the floor
    monkeypatch.setattr(R, "PREFIX_GROUPS_MIN_MEMBERS", 3)
    assert R.prefix_groups(bt, computed, ql, 16, 4, False) is None
    assert R.prefix_groups(bt, computed, ql, 16, 4, True) is not None                      # fp8 has a constant of its own
    monkeypatch.setattr(R, "PREFIX_GROUPS_MIN_MEMBERS", 2)
    # the length floor, and never below one tile whatever the constants
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_LEN", 64)
    assert R.prefix_groups(bt, computed, ql, 16, 4, False) is None
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_LEN", 0)
    assert R.prefix_groups(_table([[1], [1]]), np.array([31, 31]), [1, 1], 16, 4, False) is None
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_LEN", 32)
    # grouped requests x kv heads against the item threshold
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_ITEMS", 9)
    assert R.prefix_groups(bt, computed, ql, 16, 4, False) is None and R.prefix_groups(bt, computed, ql, 16, 8, False) is not None
    monkeypatch.setattr(R, "SHARED_PREFIX_MIN_ITEMS", 1)
    # 17 buckets of two, the first of three: the cap keeps 16, largest first, the 17th stays ungrouped
    from arcticinference_amd import ops
    assert R.PREFIX_GROUPS_MAX == ops.prefix_max_groups() == 16
    rows = [[100 + 2 * b, 101 + 2 * b, 500 + 3 * b + k] for b in range(17) for k in range(2)] + [[100, 101, 999]]
    got = R.prefix_groups(_table(rows), np.full(35, 40), [1] * 35, 16, 4, False)
    req_group, lens = got
    assert len(lens) == 16 and lens == [32] * 16
    assert req_group[0] == req_group[1] == req_group[34] == 0                # three members: first
    assert req_group[32] == req_group[33] == -1 and (req_group[:32] >= 0).all()
    assert sorted(set(req_group[:32].tolist())) == list(range(16))
    ops.PrefixGroups(req_group, lens, [1] * 35, "cpu")                       # what the decision returns is a valid argument


def test_host_block_table_accessor(floor_thresholds):
    R = floor_thresholds
    bt = _table([[1, 2, 3], [1, 2, 3]])

    class WithGetter:
        def get_numpy_array(self):
            return bt

    class WithField:
        block_table_np = bt

    class Multi:
        def __init__(self, n):
            self.block_tables = [WithGetter() for _ in range(n)]

    for ok in (bt, WithGetter(), WithField(), [bt], (WithGetter(),), [WithField()], Multi(1)):
        assert R.host_block_table(ok) is bt
        assert R.prefix_groups(ok, np.array([40, 40]), [1, 1], 16, 4, False) is not None
    for bad in (None, [bt, bt], Multi(2), [], "table", 3, torch.zeros(2, 3, dtype=torch.int32), np.zeros(4, dtype=np.int32)):
        assert R.host_block_table(bad) is None
        assert R.prefix_groups(bad, np.array([40, 40]), [1, 1], 16, 4, False) is None        # two kv-cache groups: no groups


def test_publish_keeps_its_positional_form_and_reads_the_switch(floor_thresholds, monkeypatch):
    from arcticinference_amd.vllm_plugin import step_context
    R = floor_thresholds
    assert R.PREFIX_GROUPS_ENV == "ARCTIC_INFERENCE_HIP_PREFIX_GROUPS" and "prefix_groups" in step_context.calls
    bt, computed = _table([[1, 2, 3], [1, 2, 3]]), np.array([40, 40])
    dev = torch.device("cpu")
    try:
        monkeypatch.setenv(R.PREFIX_GROUPS_ENV, "1")
        step_context.publish(np.array([1, 1]), False)                    # the old two positional arguments: no groups
        assert step_context.prefix_groups_on() and step_context.prefix_groups(4, False, dev) is None
        step_context.publish(np.array([1, 1]), False, block_table=bt, num_computed=computed, block_size=16)
        g = step_context.prefix_groups(4, False, dev)
        assert g is not None and g.n_groups == 1 and step_context.prefix_groups(4, False, dev) is g    # once per step
        assert g.group_prefix_len.tolist() == [40] and g.group_leader.tolist() == [0]      # every column equal: capped by what is computed
        monkeypatch.delenv(R.PREFIX_GROUPS_ENV)
        assert step_context.prefix_groups_on()                           # not before the next step
        step_context.publish(np.array([1, 1]), False, block_table=bt, num_computed=computed, block_size=16)
        assert not step_context.prefix_groups_on() and step_context.prefix_groups(4, False, dev) is None   # switch off
    finally:
        monkeypatch.delenv(R.PREFIX_GROUPS_ENV, raising=False)
        step_context.publish(np.array([1]), False)
        step_context.clear()


def test_shipped_group_thresholds_are_the_measured_break_evens():
    from arcticinference_amd.vllm_plugin import runner_logic as R
    assert (R.PREFIX_GROUPS_MIN_MEMBERS, R.PREFIX_GROUPS_MIN_MEMBERS_FP8) == (4, 8)
    assert (R.PREFIX_GROUPS_MAX_SUFFIX_FRACTION, R.PREFIX_GROUPS_MAX_SUFFIX_FRACTION_FP8) == (0.64, 0.52)
    assert R.PREFIX_GROUPS_MAX_LEN_SPREAD_FP8 == 31
    text = open(os.path.join(ROOT, "arcticinference_amd", "vllm_plugin", "runner_logic.py")).read()
    assert "profiles/prefix_groups_microbench.txt" in text[text.index("PREFIX_GROUPS_ENV ="):text.index("def host_block_table")]
    assert os.path.exists(os.path.join(ROOT, "profiles", "prefix_groups_microbench.txt"))

    def ask(sizes, P, fp8=False, loners=0, loner_ctx=4224, kv_heads=8, ctx=4224):
        """How many groups the decision keeps for the measured step: sizes[g] requests share P[g] tokens, 4 query tokens
        each, 4224-token contexts, pages of 16."""
        lens = [P] * len(sizes) if isinstance(P, int) else P
        width = ctx // 16 + 1
        rows, seq = [], []
        for g, (n, length) in enumerate(zip(sizes, lens)):
            for m in range(n):
                rows.append([100000 * (g + 1) + j for j in range(length // 16)] + [5000000 + 1000 * len(rows) + j
                                                                                  for j in range(width - length // 16)])
                seq.append(ctx)
        for _ in range(loners):
            rows.append([9000000 + 1000 * len(rows) + j for j in range(width)])
            seq.append(loner_ctx)
        got = R.prefix_groups(_table(rows, width), np.asarray(seq) - 4, [4] * len(rows), 16, kv_heads, fp8)
        return 0 if got is None else len(got[1])
    # the measured shapes: wins are taken, losses refused
    assert ask([64], 2048) == 1 and ask([32, 32], 2048) == 2 and ask([16] * 4, 2048) == 4 and ask([8] * 8, 2048) == 8
    assert ask([4] * 16, 2048) == 16 and ask([4] * 16, 2048, fp8=True) == 0
    assert ask([64], 2048, fp8=True) == 1 and ask([32, 32], 2048, fp8=True) == 2 and ask([8] * 8, 2048, fp8=True) == 8
    assert ask([24, 24], 2048, loners=16) == 0 and ask([31, 31], 2048, loners=2) == 0
    assert ask([24, 24], 2048, loners=16, fp8=True) == 0 and ask([31, 31], 2048, loners=2, fp8=True) == 0
    # (the loners' pages differ in the first 2048 tokens, so with the shipped length floor the 1024-token group is a
    # bucket of its own and is refused as too short: 32 requests in no group, and the step is the plain call)
    assert ask([32, 32], [1024, 3072]) == 0 and ask([32, 32], [1024, 3072], fp8=True) == 0
    assert ask([32, 32], [2048, 3072]) == 2 and ask([32, 32], [2048, 3072], fp8=True) == 0
    # members below the floor stay ungrouped, and then keep their whole context: refused
    assert ask([3, 61], 2048) == 0 and ask([7, 57], 2048, fp8=True) == 0
    # requests in no group that are SHORT against the longest context do not set the launch's end: taken
    assert ask([31, 31], 2048, loners=2, loner_ctx=2000) == 2 and ask([31, 31], 2048, loners=2, loner_ctx=2800) == 0
    assert ask([31, 31], 2048, loners=2, loner_ctx=2000, fp8=True) == 0      # 62 x 8 = 496 items: under the fp8 item threshold
    # fewer than SHARED_PREFIX_MIN_ITEMS grouped requests x kv heads (a rank of Ulysses SP = 8 has one kv head)
    assert ask([32, 32], 2048, kv_heads=1) == 0 and ask([16, 16], 2048) == 2 and ask([15, 15], 2048) == 0


# ---- ops: answered before the device check --------------------------------------------------------------------------
def _call(groups, q_lens=(1, 2, 1), seq_lens=(100, 80, 20), **kw):
    from arcticinference_amd import ops
    Hq, Hkv, D, bs = 4, 1, 128, 16
    T = sum(q_lens)
    q = torch.zeros(T, Hq, D, dtype=torch.bfloat16)
    kc = torch.zeros(16, bs, Hkv, D, dtype=torch.bfloat16)
    bt = torch.zeros(len(q_lens), 8, dtype=torch.int32)
    qsl = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)), dtype=torch.int32)
    return ops.verify_attention(q, kc, kc.clone(), bt, torch.tensor(seq_lens, dtype=torch.int32), qsl, max(q_lens),
                                max(seq_lens), D ** -0.5, q_lens_host=list(q_lens), prefix_groups=groups, **kw)


def test_ops_refuses_bad_group_arguments_without_a_device():
    from arcticinference_amd import ops
    ql = [1, 2, 1]
    good = ops.PrefixGroups([0, 0, -1], [64], ql, "cpu")
    assert good.n_groups == 1 and good.group_leader.tolist() == [0] and good.group_token_start.tolist() == [0, 3]
    assert good.group_token_index.tolist() == [0, 1, 2] and good.req_prefix_len.tolist() == [64, 64, 0]
    with pytest.raises(ValueError, match="at most 16"):
        ops.PrefixGroups(list(range(17)), [32] * 17, [1] * 17, "cpu")
    with pytest.raises(ValueError, match="request 1: group index 1 out of range"):
        ops.PrefixGroups([0, 1, -1], [64], ql, "cpu")
    with pytest.raises(ValueError, match="request 2: group index -2"):
        ops.PrefixGroups([0, 0, -2], [64], ql, "cpu")
    with pytest.raises(ValueError, match="group 1 has no members"):
        ops.PrefixGroups([0, 0, -1], [64, 32], ql, "cpu")
    with pytest.raises(ValueError, match="q_lens_host"):
        ops.PrefixGroups([0, 0, -1], [64], None, "cpu")
    with pytest.raises(ValueError, match=">= 0"):
        ops.PrefixGroups([0, 0, -1], [-64], ql, "cpu")
    with pytest.raises(ValueError, match="give one"):
        _call(good, shared_prefix_len=64, prefix_block_table=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="sliding window"):
        _call(good, sliding_window=128)
    with pytest.raises(ValueError, match="request 1"):
        _call(good, seq_lens=(100, 65, 20))                              # 65 - 2 < 64, lengths on the host (a CPU tensor)
    with pytest.raises(ValueError, match="request 0"):
        _call(good, seq_lens_host=[64, 80, 20])                          # the host lengths decide
    with pytest.raises(ValueError, match="requests"):
        _call(ops.PrefixGroups([0, 0], [64], [1, 2], "cpu"))             # another step's groups
    with pytest.raises(ValueError, match="max_seq_len"):
        _call(ops.PrefixGroups([0, 0, -1], [128], ql, "cpu"), seq_lens=(100, 80, 20), seq_lens_host=[200, 200, 20])
    # a good call, and one without groups, get as far as the device check (CPU tensors): nothing above is what stops them
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(good)
    with pytest.raises(RuntimeError, match="GPU only"):
        _call(None)


# ---- header and library ---------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_group_entry_points():
    from arcticinference_amd import _native as N
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    for name in ("aic_verify_attention_prefix_groups", "aic_prefix_max_groups"):
        assert f"int {name}(" in text, name
        assert name in N._SIGNATURES and name in N.EXPORTED_SYMBOLS
        assert hasattr(N.lib(), name), f"libarctic_hip.so lacks {name}"
    assert N.lib().aic_prefix_max_groups() == 16
    dt, gr = N._SIGNATURES["aic_verify_attention_dt"][1], N._SIGNATURES["aic_verify_attention_prefix_groups"][1]
    assert gr[:len(dt) - 1] == dt[:-1] and len(gr) == len(dt) + 6       # dt's arguments before `stream`, then six, then stream
    decl = text[text.index("int aic_verify_attention_prefix_groups("):]
    decl = decl[:decl.index(";")]
    for a, b in zip(("int n_groups", "group_prefix_len", "group_leader", "group_token_start", "group_token_index",
                     "req_prefix_len"), ("group_prefix_len", "group_leader", "group_token_start", "group_token_index",
                                         "req_prefix_len", "void* stream")):
        assert decl.index("int q_dtype") < decl.index(a) < decl.index(b)
    assert "ulysses.py:510" in text[text.index("aic_verify_attention_dt for a step whose requests fall into GROUPS"):
                                    text.index("int aic_prefix_max_groups(")]


def _i32(xs):
    return np.asarray(xs, dtype=np.int32)


def test_group_entry_answers_argument_errors_before_any_launch():
    """A call that breaks the argument rules is answered before the device is looked for; without a device, one that keeps
    them ends at AIC_ERR_NO_DEVICE."""
    from arcticinference_amd import _native as N
    L = N.lib()

    def call(n, lens, leaders, starts, index=1, req_len=1, window=0, max_seq_len=200, batch=2, tokens=3):
        keep = [None if a is None else _i32(a) for a in (lens, leaders, starts)]
        ptr = [None if a is None else a.ctypes.data for a in keep]
        return L.aic_verify_attention_prefix_groups(1, 512, 1, 1, 16 * 128, N.DT_BF16, None, None, 1, 8, 1, 1, batch, tokens, 2, 4,
                                                    1, 128, 16, 0.088, 1, 512, 1, 1 << 20, max_seq_len, None, 0, None, 0,
                                                    window, None, N.DT_BF16, n, ptr[0], ptr[1], ptr[2], index, req_len, None)
    bad = N.AIC_ERR_INVALID
    assert call(-1, None, None, None) == bad
    assert call(17, [64] * 17, [0] * 17, [0] * 18) == bad                   # above the cap
    assert call(1, None, [0], [0, 3]) == bad and call(1, [64], None, [0, 3]) == bad and call(1, [64], [0], None) == bad
    assert call(1, [64], [0], [0, 3], index=None) == bad and call(1, [64], [0], [0, 3], req_len=None) == bad
    assert call(1, [-1], [0], [0, 3]) == bad                                # a negative length
    assert call(1, [64], [2], [0, 3]) == bad and call(1, [64], [-1], [0, 3]) == bad    # a leader outside the batch
    assert call(2, [64, 32], [0, 1], [0, 2, 1]) == bad                      # starts decrease
    assert call(1, [64], [0], [0, 4]) == bad                                # ... or end above the call's tokens
    assert call(1, [64], [0], [0, 3], max_seq_len=64) == bad                # no query token behind the longest P_g
    assert call(1, [64], [0], [0, 3], window=128) == N.AIC_ERR_UNSUPPORTED
    if not torch.cuda.is_available():                    # (with a device these would launch on the dummy pointers)
        assert call(1, [64], [0], [0, 3]) == N.AIC_ERR_NO_DEVICE
        assert call(2, [64, 20], [0, 1], [0, 2, 3]) == N.AIC_ERR_NO_DEVICE
        assert call(1, [95], [0], [0, 3], max_seq_len=65) == N.AIC_ERR_NO_DEVICE # P_g is 64: the rounded length counts
        assert call(0, None, None, None, None, None) == N.AIC_ERR_NO_DEVICE      # the plain call
        assert call(1, [20], [0], [0, 3]) == N.AIC_ERR_NO_DEVICE                 # below one tile: the plain call too
