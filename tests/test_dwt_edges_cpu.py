"""No GPU: oracle/dwt_oracle.py against PyWavelets 1.1.1 at the edges of tests/golden/dwt_edge_cases.py (tests/golden/dwt_edges.npz,
written by tests/golden/make_dwt_edge_golden.py), so that tests/test_gpu_dwt_kernel_edges.py leans on nothing that was not compared with
pywt: signals shorter than the filter in all six modes, 22 .. 64 taps, and the 13 wavelets of 66 .. 102 taps.

Every fixture entry equals the oracle to 1e-12 x max(1, peak); table and fixture name the same cases (but for the reflect extension of
one sample, where PyWavelets does not return: dwt_edge_cases._case).  ``MEASURED_FP32`` records, per edge group, what the operation
itself costs in float32: the largest |oracle in float32 - oracle in float64| over the group's cases as a fraction of max(1, peak).  The GPU
module takes its fp32 bound from this table, never from a kernel's result."""
import os

import numpy as np
import pytest

from oracle import dwt_oracle as dwo
from tests.conftest import GOLDEN
from tests.golden import dwt_edge_cases as ec

FIX = ec.load_fixture(os.path.join(GOLDEN, "dwt_edges.npz"))
TOL = 1e-12

# group -> largest fp32 cost of the operation itself, x max(1, peak), as printed by test_fp32_cost (E5 / E7: the cases beyond the fixture)
MEASURED_FP32 = {"E1": 6.07e-07, "E2": 4.26e-07, "E3": 2.86e-07, "E4": 3.47e-07, "LONG": 4.79e-07, "E5": 1.82e-07, "E7": 5.61e-07}
TOL_FP32 = 2e-5  # the project's fp32 coefficient bound (tests/test_gpu_wavelet.py)


def fp32_bound(group):
    """2e-5 x max(1, peak), unless the group's measured cost exceeds a quarter of it: then four times that cost"""
    m = MEASURED_FP32[group]
    return 4.0 * m if m > TOL_FP32 / 4 else TOL_FP32


def oracle_results(case, dtype=np.float64):
    """(lo, hi, rec) of the whole batch: analysis of x, synthesis of the case's own coefficient inputs"""
    x, (lo, hi) = ec.inputs(case)
    x, lo, hi = (v.astype(dtype) for v in (x, lo, hi))
    wave, mode = case["wave"], case["mode"]
    if case["dim"] == 1:
        dec_lo, dec_hi, rec_lo, rec_hi = dwo.taps(wave)
        a, d = dwo.dwt_axis(x, dec_lo, dec_hi, mode, -1)
        return a, d, dwo.idwt_axis(lo, hi, rec_lo, rec_hi, mode, -1)
    ll, bands = dwo.dwt2(x, wave, mode)
    return ll, bands, dwo.idwt2(lo, hi, wave, mode)


def fixture_form(case, res):
    """what the fixture keeps of a result: row / plane [0, 0], 2-D planes through probe()"""
    picked = [np.asarray(r[0, 0], dtype=np.float64) for r in res]
    return [p.ravel() for p in picked] if case["dim"] == 1 else [ec.probe(p).ravel() for p in picked]


def test_table_and_fixture_name_the_same_cases():
    want = {k for c in ec.CASES if c["pywt"] for k in ec.fixture_keys(c)}
    assert want == set(FIX), (sorted(want - set(FIX))[:5], sorted(set(FIX) - want)[:5])
    no_pywt = [c["id"] for c in ec.CASES if not c["pywt"]]
    assert no_pywt and all("-reflect-" in i for i in no_pywt)
    for wave, flen in {**ec.E1_WAVES, **ec.E2_WAVES, **ec.LONG_WAVES}.items():
        assert len(dwo.taps(wave)[0]) == flen, wave
    groups = {c["group"] for c in ec.CASES}
    assert groups == set(ec.GROUPS)
    e1 = {(c["wave"], c["mode"], c["dim"]) for c in ec.CASES if c["group"] == "E1"}
    assert len(e1) == len(ec.E1_WAVES) * 6 * 2
    assert {c["wave"] for c in ec.CASES if c["group"] == "LONG"} == set(ec.LONG_WAVES) and len(ec.LONG_WAVES) == 13


@pytest.mark.parametrize("group", ec.GROUPS)
def test_oracle_matches_pywt(group):
    n = 0
    for case in ec.CASES:
        if case["group"] != group or not case["pywt"]:
            continue
        for key, got in zip(ec.fixture_keys(case), fixture_form(case, oracle_results(case))):
            want = FIX[key]
            assert got.shape == want.shape, (key, got.shape, want.shape)
            err = np.abs(got - want)
            bound = TOL * max(1.0, float(np.abs(want).max()))
            assert err.max() <= bound, f"{key}: oracle and pywt differ by {err.max():.3g} > {bound:.3g}, first at index {int(np.argmax(err > bound))}"
        n += 1
    assert n > 0


def test_reflect_of_one_sample_is_constant_extension():
    """the cases without a pywt result: the oracle must give there what the constant extension gives (one sample repeated)"""
    for case in ec.CASES:
        if case["pywt"]:
            continue
        x, _ = ec.inputs(case)
        dec_lo, dec_hi, _, _ = dwo.taps(case["wave"])
        axis = -2 + case["shape"].index(1) if case["dim"] == 2 else -1  # the axis of length 1
        a, d = dwo.dwt_axis(x, dec_lo, dec_hi, "reflect", axis)
        ca, cd = dwo.dwt_axis(x, dec_lo, dec_hi, "constant", axis)
        np.testing.assert_array_equal(a, ca)
        np.testing.assert_array_equal(d, cd)


def _cost(pairs):
    worst = 0.0
    for lo_p, hi_p in pairs:
        peak = max(1.0, float(np.abs(hi_p).max()))
        worst = max(worst, float(np.abs(lo_p.astype(np.float64) - hi_p).max()) / peak)
    return worst


def _beyond_fixture(dtype):
    """E5 and E7 through the oracle in ``dtype``: {group: [result arrays]}"""
    out = {"E5": [], "E7": []}
    for spec, dim in ((ec.E5_1D, 1), (ec.E5_2D, 2)):
        x = ec.big_inputs(f"E5-{dim}d", spec["batch"], spec["shape"]).astype(dtype)
        if dim == 1:
            dec_lo, dec_hi, rec_lo, rec_hi = dwo.taps(spec["wave"])
            a, d = dwo.dwt_axis(x, dec_lo, dec_hi, spec["mode"], -1)
            out["E5"] += [a, d, dwo.idwt_axis(a, d, rec_lo, rec_hi, spec["mode"], -1)]
        else:
            ll, hi = dwo.dwt2(x, spec["wave"], spec["mode"])
            out["E5"] += [ll, hi, dwo.idwt2(ll, hi, spec["wave"], spec["mode"])]
    for cases, shape, dec, rec in ((ec.E7_2D, ec.E7_PLANE, dwo.wavedec2, dwo.waverec2), (ec.E7_1D, ec.E7_ROW, dwo.wavedec1, dwo.waverec1)):
        for wave, mode, level in cases:
            x = ec.big_inputs(f"E7-{wave}-{len(shape)}d", ec.BATCH, shape).astype(dtype)
            yl, yh = dec(x, wave, mode, level)
            out["E7"] += [yl, *yh, rec(yl, yh, wave, mode)]
    return out


def test_fp32_cost():
    """the fp32 cost of the operation itself, per edge group; printed (run with -s); the record may not understate it (2 % for the last
    digit) nor overstate it twofold"""
    cost = {}
    for group in ec.GROUPS:
        cases = [c for c in ec.CASES if c["group"] == group]
        cost[group] = _cost((lo_p, hi_p) for c in cases for lo_p, hi_p in zip(oracle_results(c, np.float32), oracle_results(c)))
    low, high = _beyond_fixture(np.float32), _beyond_fixture(np.float64)
    for group in low:
        cost[group] = _cost(zip(low[group], high[group]))
    print("MEASURED_FP32 =", {g: float(f"{v:.3g}") for g, v in cost.items()})
    print("fp32 bounds   =", {g: fp32_bound(g) for g in cost})
    for group, v in cost.items():
        rec = MEASURED_FP32[group]
        assert rec / 2 <= v <= 1.02 * rec, f"{group}: measured {v:.4g}, recorded {rec:.4g}"
