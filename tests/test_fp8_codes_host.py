"""CPU: the bit-level fp8 encoder / decoder of tests/fp8_codes.py against the project's oracles, and the attention fixtures
of tests/test_gpu_fp8_codes.py on references alone (they must tell every finite code from its neighbours before a GPU
result on them means anything)."""
import numpy as np
import pytest
import torch

import attention_fixtures as F
import fp8_codes as C
from oracle import spec_oracle as O


def _sat(x_f32, fmt):
    return O.fp8_sat(torch.from_numpy(np.ascontiguousarray(x_f32)), C.ORACLE_KIND[fmt]).view(torch.uint8).numpy()


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_decode_of_encode_is_the_identity_on_every_finite_code(fmt):
    codes = C.finite_codes(fmt)
    assert codes.size == {"e4m3fn": 254, "e5m2": 248}[fmt]
    vals = C.decode(codes, fmt)
    assert np.isfinite(vals).all() and np.array_equal(vals.astype(np.float32).astype(np.float64), vals)
    e = C.encode(vals.astype(np.float32), fmt)
    assert not e.nan.any() and np.array_equal(e.code, codes)              # -0 -> 0x80 included
    assert vals.max() == {"e4m3fn": 448.0, "e5m2": 57344.0}[fmt]
    assert np.abs(vals[vals != 0]).min() == {"e4m3fn": 2.0 ** -9, "e5m2": 2.0 ** -16}[fmt]
    # the table agrees with torch's own decoder, the one the attention oracle reads caches with
    t = torch.arange(256, dtype=torch.uint8).view(C.TORCH_DTYPE[fmt]).float().numpy().astype(np.float64)
    assert np.array_equal(t[codes], vals) and np.isnan(C.decode_table(fmt)[~np.isfinite(t)]).sum() == np.isnan(t).sum()


@pytest.mark.parametrize("fmt", C.FORMATS)
def test_encode_is_monotone_and_saturates(fmt):
    x = C.f32_boundaries(fmt)
    finite = x[~np.isnan(x)]
    assert np.isnan(x).sum() == 4 and np.isinf(finite).sum() == 2 and x.size > 1500
    finite = np.sort(finite)
    e = C.encode(finite, fmt)
    assert not e.nan.any() and C.encode(x[np.isnan(x)], fmt).nan.all()
    key = C.order_key(e.code)
    assert (np.diff(key) >= 0).all()
    assert set(e.code.tolist()) == set(C.finite_codes(fmt).tolist())      # every finite code is some boundary's answer
    top = C.max_code(fmt)
    assert e.code[-1] == top and e.code[0] == (top | 0x80)                # +-inf
    big = C.decode(top, fmt)
    assert (C.encode(np.float32([big * 1.04, -big * 1.04, 3e38]), fmt).code == [top, top | 0x80, top]).all()
    # ties go to the even code: the midpoint of codes c and c + 1 is answered by whichever of them is even
    pos = np.arange(0, top, dtype=np.uint8)
    mids = ((C.decode(pos, fmt) + C.decode(pos + 1, fmt)) / 2).astype(np.float32)
    assert np.array_equal(C.encode(mids, fmt).code, pos + (pos & 1))
    assert np.array_equal(C.encode(-mids, fmt).code, (pos + (pos & 1)) | 0x80)
    assert (C.encode(np.float32([0.0, -0.0]), fmt).code == [0x00, 0x80]).all()


@pytest.mark.parametrize("scale", C.SCALES)
@pytest.mark.parametrize("fmt", C.FORMATS)
def test_encode_equals_the_oracles_conversion_outside_nan(fmt, scale):
    """oracle.spec_oracle.fp8_sat (clamp, then torch's conversion) on every 16-bit pattern and every f32 boundary,
    divided in f32 as the bulk KV write divides."""
    compared = 0
    for x in (C.all_bf16(), C.all_fp16(), C.f32_boundaries(fmt)):
        quo = C.divide(x, scale)
        e = C.encode(quo, fmt)
        assert np.array_equal(e.nan, np.isnan(quo))
        ok = ~e.nan
        assert np.array_equal(e.code[ok], _sat(quo, fmt)[ok])
        # on NaN torch keeps the sign; the bulk write does not (fp8_codes' docstring): the oracle's NaN codes are not
        # the kernel's, which is why a NaN is a class here
        assert C.is_nan_code(_sat(quo, fmt)[~ok], fmt).all()
        compared += int(ok.sum())
    assert compared > 2 * 65536 - 2 * 2100


def test_the_oracles_per_tensor_quantiser_is_encode_of_x_times_inverse_scale():
    for name, x in C.quant_inputs().items():
        codes, scale = C.quant_per_tensor(x)
        q, s = O.fp8_quant_per_tensor(C.bf16_tensor(x))
        assert float(s) == float(scale), name
        assert np.array_equal(q.view(torch.uint8).numpy(), codes), name
    inputs = C.quant_inputs()
    assert float(C.quant_per_tensor(inputs["all-zero"])[1]) == np.float32(1.0 / (448.0 * 512.0))
    codes, scale = C.quant_per_tensor(inputs["every-finite-bf16"])
    assert np.isin(codes & 0x7f, np.arange(8)).mean() > 0.9 and (codes & 0x7f).max() == 0x7e
    x = inputs["amax-rounds-above-448"]
    inv = np.float32(1.0) / C.quant_per_tensor(x)[1]
    assert np.float32(x[0]) * inv > np.float32(448.0) and C.quant_per_tensor(x)[0][0] == 0x7e and x.size % 4
    assert set(C.quant_per_tensor(inputs["bf16-up-to-448"])[0].tolist()) == set(C.finite_codes("e4m3fn").tolist())


# ---- the attention fixtures discriminate ------------------------------------------------------------------------------
# smallest ratio measured on the CPU (movement of an output element over the bar at that element, over every finite code
# and both neighbours): V sweep 14.18 (code 0x90 -> 0x8f), K sweep 15.49 (code 0x18 -> 0x17)
@pytest.mark.parametrize("sweep", ["v", "k"])
def test_sweeps_tell_every_code_from_its_neighbours(sweep):
    builder = C.v_sweep_case if sweep == "v" else C.k_sweep_case
    case = builder(torch.bfloat16)
    assert torch.allclose(C.reference(case).float(), F.oracle(case), atol=1e-5, rtol=1e-5)      # the project's oracle
    assert torch.allclose(C.sweep_reference(case)[0], C.reference(case), atol=1e-12, rtol=1e-12)
    assert sorted(set(case.codes.tolist())) == C.finite_codes("e4m3fn").tolist()
    ratios = C.discrimination(case)
    assert len(ratios) == 2 * 254 - 4                    # both neighbours, +-0 and +-448 have one
    assert {c for c, _ in ratios} == set(C.finite_codes("e4m3fn").tolist())
    worst = min(ratios, key=ratios.get)
    print(f"{sweep} sweep: smallest discrimination ratio {ratios[worst]:.2f} at code {worst[0]:#04x} -> {worst[1]:#04x}")
    assert ratios[worst] >= 10.0, (worst, ratios[worst])


def test_sweep_rows_are_what_their_docstrings_say():
    v = C.v_sweep_case(torch.float16)
    want = C.reference(v)
    rows = torch.from_numpy(C.code_of_row())
    value = torch.from_numpy(C.decode(v.codes, "e4m3fn"))[rows] * v.vs
    assert torch.allclose(want, value[..., None].expand_as(want), atol=1e-6, rtol=1e-6)   # the target holds the whole row
    assert float(value.abs().max()) == 448 * 64 and float(value.abs()[value != 0].min()) == 0.125
    assert torch.isfinite(want.to(torch.float16)).all()
    k = C.k_sweep_case(torch.float16)
    want = C.reference(k)
    dims = torch.tensor([[C.k_sweep_dim(int(c)) for c in r] for r in C.code_of_row()])
    own = want.gather(2, dims[..., None]).squeeze(-1)
    table = C.decode(np.arange(256), "e4m3fn")
    mant = np.array([abs(table[c]) / 2.0 ** np.floor(np.log2(abs(table[c]))) if table[c] == table[c] and table[c] != 0 else 0.0
                     for c in range(256)])
    n = 15 + 4 + (torch.arange(64) % 4 + 1)[:, None].double()       # the other keys a row sees
    expect = torch.tanh((C.K_SWEEP_GAIN * torch.from_numpy(mant)[rows] - torch.log(n)) / 2)
    assert torch.allclose(own, expect, atol=1e-9)
    assert float(own.abs().max()) < 0.95                  # no row saturates: the zero codes score 0 against 23 keys


# ---- the uniform-code and round-trip fixtures --------------------------------------------------------------------------
def test_uniform_codes_keep_the_scores_within_a_few_nats():
    c = C.uniform_case([33], [200], 8, 2, 16, seed=1, dtype=torch.bfloat16)
    assert C.UNIFORM_K_SCALE == 2.0 ** -6 and 1.0 < C.score_spread(c) < 3.0
    codes = c.kc.view(torch.uint8).numpy()
    assert not np.isin(codes, C.NAN_CODES).any()
    first_tile = codes[int(c.bt[0, 0])]                                   # subnormals and the top binade in every tile
    assert ((first_tile & 0x7f) < 8).any() and ((first_tile & 0x7f) >= 0x78).any()
    assert torch.isfinite(F.oracle(c)).all()


def test_round_trip_source_saturates_about_one_percent():
    keys, values = C.round_trip_source()
    for x in (keys, values):
        quo = C.divide(x, C.ROUND_TRIP_SCALE)
        frac = float((np.abs(quo) > 448.0).mean())
        assert 0.005 < frac < 0.02, frac
        codes = C.encode(quo, "e4m3fn").code
        assert ((codes & 0x7f) == 0x7e).mean() >= frac and ((codes & 0x7f) == 0).any() and ((codes & 0x7f) < 8).mean() > 0.1
        assert np.array_equal(C.bf16_tensor(x).float().numpy(), x)
