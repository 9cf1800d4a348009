"""CPU: the host half of whole-step attention (aic_step_attention) — the three-way request partition, the compact
decode layout, the plugin's routing decision and the workspace bound.  No GPU needed."""
import numpy as np
import pytest

from arcticinference_amd import ops
from arcticinference_amd.vllm_plugin import step_context


def _parts(q_lens, G):
    order, ns, npf, nl = ops.split_order3(q_lens, G)
    return order.tolist(), order[:ns].tolist(), order[ns:ns + npf].tolist(), order[ns + npf:].tolist(), (ns, npf, nl)


def test_split_order3_partitions_in_batch_order():
    # G = 4: short = q_len <= 8; prefill = q_len > 33; long = the rest (9 .. 33)
    q_lens = [1, 200, 9, 4, 34, 33, 8, 2048]
    order, short, pf, long_, counts = _parts(q_lens, 4)
    assert short == [0, 3, 6] and pf == [1, 4, 7] and long_ == [2, 5]
    assert sorted(order) == list(range(len(q_lens))) and counts == (3, 3, 2)
    assert order.__class__ is list and ops.split_order3(q_lens, 4)[0].dtype == np.int32


@pytest.mark.parametrize("q_lens,G,want", [
    ([4, 3, 1], 4, ([0, 1, 2], [], [])),              # decode only: no prefill list
    ([100, 64, 34], 8, ([], [0, 1, 2], [])),          # prefill only
    ([33, 5], 8, ([], [], [0, 1])),                   # long drafts only (G = 8: 5 tokens are 40 rows)
    ([34, 1, 500, 2, 35], 1, ([1, 3], [0, 2, 4], [])),  # prefill requests interleaved with decodes
    ([], 4, ([], [], [])),
])
def test_split_order3_edge_cases(q_lens, G, want):
    _, short, pf, long_, _ = _parts(q_lens, G)
    assert (short, pf, long_) == want


def test_split_order3_agrees_with_split_order_without_prefill():
    rng = np.random.default_rng(0)
    for _ in range(50):
        q_lens = rng.integers(1, 34, size=rng.integers(1, 40))
        G = int(rng.choice([1, 2, 4, 8]))
        order2, n_short = ops.split_order(q_lens, G)
        order3, ns, npf, nl = ops.split_order3(q_lens, G)
        assert npf == 0 and ns == n_short and order3.tolist() == order2.tolist()


def test_decode_index_compacts_the_decode_rows():
    q_lens = [3, 100, 1, 34, 4]
    qsl, idx, max_dec = ops.decode_index(q_lens)
    assert qsl.tolist() == [0, 3, 3, 4, 4, 8]              # the prefill requests get empty ranges
    # tokens of the call: r0 0..2, r1 3..102, r2 103, r3 104..137, r4 138..141
    assert idx.tolist() == [0, 1, 2, 103, 138, 139, 140, 141]
    assert max_dec == 4 and qsl.dtype == np.int32 and idx.dtype == np.int32


def test_decode_index_edge_cases():
    qsl, idx, max_dec = ops.decode_index([64, 2048])
    assert qsl.tolist() == [0, 0, 0] and idx.size == 0 and max_dec == 0
    qsl, idx, max_dec = ops.decode_index([2, 33])
    assert qsl.tolist() == [0, 2, 35] and idx.tolist() == list(range(35)) and max_dec == 33


def test_decode_index_matches_a_reference_walk():
    rng = np.random.default_rng(1)
    for _ in range(30):
        q_lens = rng.choice([1, 2, 4, 9, 33, 34, 64, 300], size=rng.integers(1, 20))
        qsl, idx, _ = ops.decode_index(q_lens)
        want, start = [], 0
        for n in q_lens:
            if n <= 33:
                want += list(range(start, start + n))
            start += n
        assert idx.tolist() == want and int(qsl[-1]) == len(want)


@pytest.mark.parametrize("max_q,q_lens,batch,on,layer_ok,capturing,want", [
    (4, [4, 1], 2, False, True, False, "verify"),      # decode steps: the verify route whatever the switch says
    (33, [33, 1], 2, True, False, True, "verify"),
    (34, [34, 1], 2, False, True, False, "fallback"),  # prefill, switch off: vLLM's backend, as before
    (34, [34, 1], 2, True, True, False, "step"),
    (200, [200], 1, True, True, False, "step"),
    (200, [200], 1, True, False, False, "fallback"),   # a layer the prefill body does not serve
    (200, [200], 1, True, True, True, "fallback"),     # under graph capture
    (200, None, 1, True, True, False, "fallback"),     # nothing published
    (200, [200, 4], 3, True, True, False, "fallback"),  # the published step does not describe the call
    (200, [100, 4], 2, True, True, False, "fallback"),
])
def test_route_is_a_pure_function(max_q, q_lens, batch, on, layer_ok, capturing, want):
    ql = None if q_lens is None else np.asarray(q_lens)
    assert step_context.route(max_q, ql, batch, on, layer_ok, capturing) == want


def test_switch_is_read_once_per_step(monkeypatch):
    monkeypatch.delenv(step_context.PREFILL_ENV, raising=False)
    step_context.publish(np.array([40, 1]), False)
    assert not step_context.prefill_on()
    monkeypatch.setenv(step_context.PREFILL_ENV, "1")
    assert not step_context.prefill_on()           # not before the next step
    step_context.publish(np.array([40, 1]), False)
    assert step_context.prefill_on()
    monkeypatch.setenv(step_context.PREFILL_ENV, "0")
    step_context.publish(np.array([40, 1]), False)
    assert not step_context.prefill_on()
    step_context.clear()


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (8, 1), (64, 8)])
def test_workspace_of_a_mixed_step_is_at_most_decode_plus_prefill(Hq, Hkv):
    from arcticinference_amd import _native as N
    ws = N.lib().aic_step_attention_workspace_bytes
    n_dec = sum(1 + (i % 33) for i in range(63))   # 63 decodes, q_len 1 .. 33
    for chunk in (34, 512, 2048, 8192):
        mixed = ws(n_dec, 1, chunk, Hq, Hkv, 128, 64)
        dec_only = ws(n_dec, 0, 0, Hq, Hkv, 128, 64)
        pf_only = ws(0, 1, chunk, Hq, Hkv, 128, 64)
        assert mixed <= dec_only + pf_only, (chunk, mixed, dec_only, pf_only)
        assert pf_only < 64 << 20            # the chunk's own need stays small: no per-token partials unsplit
    # a decode-only step needs exactly what aic_verify_attention_ex needs
    assert ws(n_dec, 0, 0, Hq, Hkv, 128, 64) == N.lib().aic_verify_attention_workspace_bytes(n_dec, Hq, 128, 64)
