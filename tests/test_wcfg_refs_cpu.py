"""CPU: tests/wcfg_refs.py, the host restatement of the fused WaveletCFG entry points, against the reference-run fixtures of
tests/golden/wavelet_cfg.npz -- so that the GPU module that leans on it (tests/test_gpu_wcfg_kernel_edges.py) is not compared with a second
unanchored opinion -- and the fp32-oracle bound of every case of that module.

Fixtures: the three forms must reproduce every 4-D high-precision case whose rule they can express, to 1e-12 of the output's peak before
the final rounding; the fixtures hold fp32, so 1 ulp of fp32 at the peak is allowed on top.

fp32 bound: every GPU case runs here through the oracle in float32 and in float64.  The difference is what fp32 arithmetic costs the
OPERATION (numpy's summation order); it must stay inside the project's tolerance (5e-5 x max(1, peak)), so the case list holds no case
the reference itself would fail -- except the cases listed in ``wcfg_refs.MEASURED_FP32``, whose measured error is recorded there and checked here,
and which the GPU module allows four times that (fused multiply-adds and another summation order bound the gap in practice)."""
import importlib
import json

import numpy as np
import pytest

from tests import wavelet_helpers as wh
from tests import wcfg_refs as wr
from tests.conftest import GOLDEN
from tests.golden import wavelet_cases as wc
from oracle import dwt_oracle as dwo

WCFG = np.load(f"{GOLDEN}/wavelet_cfg.npz", allow_pickle=False)
FIXTURE_CASES = ("placeholder", "haar_per", "lerp_diff", "subtract_diff", "all_scales", "odd_sizes", "two_levels_inv_wave", "mixed_modes")
BANDS_CASES = tuple(n for n in FIXTURE_CASES if n != "mixed_modes")  # the form rests on IDWT(DWT(u)) = u, which a mismatched pair does not give
LOWPASS_CASES = ("placeholder", "haar_per", "subtract_diff", "two_levels_inv_wave")  # one scale per level, difference only


@pytest.fixture(scope="module")
def mod(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.wavelet_cfg")


def _rule(mod, name):
    """(inputs, want, rule as plain numbers) of a fixture case; the rule through the product's host logic, which
    tests/test_wavelet_host_cpu.py pins to the reference's own outputs."""
    case = wc.WCFG_CASES[name]
    args = wh.wcfg_args(case, name, wc.FakeModel())
    kw = wh.resolve_for_oracle(mod, case, args)
    assert kw is not None and kw["high_precision"] and kw["target"] == "denoised" and kw["wcfg_blend"] == 1.0 and kw["blend_mode"] == "lerp"
    levels = kw["level"]
    tabs = []
    for key in ("cond_scales", "uncond_scales", "diff_scales", "final_scales"):
        pair = kw[key]
        if pair is None:
            tabs.append((1.0, ((1.0,) * 3,) * levels))
        else:
            rows = dwo.expand_yh_scales(levels, 3, 1.0 if pair[1] is None else pair[1])
            rows = tuple(rows) + ((1.0,) * 3,) * (levels - len(rows))
            tabs.append((float(pair[0]), rows))
    n = wh.numpy_args(args)
    return n["cond_denoised"], n["uncond_denoised"], n["input"], WCFG[f"{name}__out"], kw, tabs


def _close(got, want):
    peak = float(np.abs(want).max())
    tol = 1e-12 * peak + float(np.spacing(np.float32(peak)))
    err = float(np.abs(got - want.astype(np.float64)).max())
    assert got.shape == want.shape and err <= tol, (err, tol)


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_ref_fused_reproduces_fixture(mod, name):
    cond, uncond, x, want, kw, tabs = _rule(mod, name)
    got = wr.ref_fused(cond, uncond, x, wave=kw["wave"], levels=kw["level"], mode=kw["mode"], inv_mode=kw["inv_mode"], inv_wave=kw["inv_wave"],
                       yl_scales=[t[0] for t in tabs], yh_scales=[[t[1][j] for t in tabs] for j in range(kw["level"])], blend_mode=kw["blend"],
                       strength=kw["strength"])
    _close(got, want)


@pytest.mark.parametrize("name", BANDS_CASES)
def test_ref_bands_reproduces_fixture(mod, name):
    """Difference-only rules in one call on (cond, uncond); ``all_scales`` as the two calls of WaveletCFG.wavelet_cfg_bands (A C + B U)."""
    cond, uncond, x, want, kw, tabs = _rule(mod, name)
    levels, blend, t = kw["level"], kw["blend"], kw["strength"]
    assert kw["inv_wave"] in (None, kw["wave"])
    common = dict(wave=kw["wave"], levels=levels, mode=kw["mode"], inv_mode=kw["inv_mode"])
    if name != "all_scales":
        assert all(tab[0] == 1.0 and all(v == 1.0 for row in tab[1] for v in row) for i, tab in enumerate(tabs) if i != 2)
        _, _, ku, kt = _kukt(blend, t)
        got = wr.ref_bands(cond, uncond, x, yh_scales=tabs[2][1], yl_scale=tabs[2][0], ku=ku, kt=kt, **common)
    else:
        ab = [[wr.blend_coeffs(*(tab[1][j][k] for tab in tabs), blend, t) for k in range(3)] for j in range(levels)]
        yl_a, yl_b = wr.blend_coeffs(*(tab[0] for tab in tabs), blend, t)
        out1 = wr.ref_bands(uncond, None, x, yh_scales=[[v[1] for v in row] for row in ab], yl_scale=yl_b, ku=0.0, kt=1.0, **common)
        got = wr.ref_bands(cond, None, out1, yh_scales=[[v[0] for v in row] for row in ab], yl_scale=yl_a, ku=0.0, kt=1.0, **common)
    _close(got, want)


def _kukt(blend, t):
    sign = -1.0 if blend == "subtract_b" else 1.0
    keep = 1.0 - t if blend == "lerp" else 1.0
    return sign, keep, keep, sign * t


@pytest.mark.parametrize("name", LOWPASS_CASES)
def test_ref_lowpass_reproduces_fixture(mod, name):
    cond, uncond, x, want, kw, tabs = _rule(mod, name)
    levels = kw["level"]
    d = [row[0] for row in tabs[2][1]]
    assert all(v == row[0] for row in tabs[2][1] for v in row)
    g = [d[0], *(d[j] - d[j - 1] for j in range(1, levels)), tabs[2][0] - d[-1]]
    _, _, ku, kt = _kukt(kw["blend"], kw["strength"])
    _close(wr.ref_lowpass(cond, uncond, x, wave=kw["wave"], levels=levels, mode=kw["mode"], inv_mode=kw["inv_mode"], g=g, ku=ku, kt=kt), want)


@pytest.mark.parametrize("wave,mode,levels,shape", [("db4", "symmetric", 3, (37, 50)), ("haar", "periodization", 2, (8, 10)), ("db9", "zero", 2, (33, 47)),
                                                    ("bior2.2", "periodic", 2, (24, 36))])
def test_ref_lowpass_agrees_with_ref_bands_and_ref_fused(wave, mode, levels, shape):
    """One scale per level: the three forms state one rule (g telescoped from d; a difference-only table; ku / kt of a lerp)."""
    cond, uncond, x = wr.inputs(9, 2, *shape)
    g, d = wr.lowpass_weights(levels, 0.6)
    t = 0.35
    low = wr.ref_lowpass(cond, uncond, x, wave=wave, levels=levels, mode=mode, g=g, ku=1.0 - t, kt=t)
    bands = wr.ref_bands(cond, uncond, x, wave=wave, levels=levels, mode=mode, yh_scales=[(s,) * 3 for s in d], yl_scale=0.6, ku=1.0 - t, kt=t)
    fused = wr.ref_fused(cond, uncond, x, wave=wave, levels=levels, mode=mode, blend_mode="lerp", strength=t,
                         **dict(zip(("yl_scales", "yh_scales"), wr.diff_tables(levels, 0.6, [(s,) * 3 for s in d]))))
    peak = float(np.abs(bands).max())
    assert float(np.abs(low - bands).max()) <= 1e-12 * peak
    assert float(np.abs(fused - bands).max()) <= 1e-12 * peak  # perfect reconstruction: IDWT(DWT(u)) = u


def test_single_level_refs():
    """ref_dwt2 / ref_idwt2: perfect reconstruction, the larger ``ll`` and the crop."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 9, 14))
    ll, hi = wr.ref_dwt2(x, wave="db4", mode="symmetric")
    assert ll.shape == (2, 8, 10) and hi.shape == (2, 3, 8, 10)
    big = np.concatenate([np.concatenate([ll, rng.standard_normal((2, 1, 10))], axis=1), rng.standard_normal((2, 9, 1))], axis=2)
    rec = wr.ref_idwt2(big, hi, wave="db4", mode="symmetric", out_hw=(9, 13))
    assert rec.shape == (2, 9, 13) and float(np.abs(rec - x[..., :13]).max()) < 1e-12


# ------------------------------------------------------------------------------------------------ the fp32 cost of the GPU module's cases
MEASURED_FP32 = wr.MEASURED_FP32


def _groups():
    groups = {}
    for gname, fn in (("filter", wr.filter_cases), ("mode", wr.mode_cases), ("short", wr.short_cases), ("tile", wr.tile_cases),
                      ("level", wr.level_cases), ("scale", wr.scale_cases)):
        for key, cases in fn().items():
            groups[f"{gname}:{key}"] = cases
    for key, c in wr.align_cases().items():
        groups[f"align:{key}"] = [c]
    return groups


GROUPS = _groups()


def fp32_cost(c, sel=slice(None)):
    """max |fp32 oracle - fp64 oracle| relative to max(1, peak of the fp64 result)."""
    want = wr.reference(c, np.float64, sel)
    got = wr.reference(c, np.float32, sel)
    assert got.dtype == np.float32
    return float(np.abs(got.astype(np.float64) - want).max()) / max(1.0, float(np.abs(want).max()))


def _check(ident, cost):
    if ident in MEASURED_FP32:
        rec = MEASURED_FP32[ident]
        assert cost > wr.TOL_OUT[False], f"{ident}: listed as measured but inside the project's tolerance ({cost:.3g})"
        assert abs(cost - rec) <= 0.02 * rec, f"{ident}: measured {cost:.4g}, recorded {rec:.4g}"
    else:
        assert cost <= wr.TOL_OUT[False], f"{ident}: the fp32 oracle itself is off by {cost:.3g} x max(1, peak)"


@pytest.mark.parametrize("group", list(GROUPS))
def test_fp32_oracle_stays_inside_the_tolerance(group):
    for i, c in enumerate(GROUPS[group]):
        _check(f"{group}#{i}", fp32_cost(c))


def test_fp32_oracle_plane_loop_and_budget_cases(pkg):
    """The cases whose SHAPE comes from the library's plan queries (host functions; no GPU needed), and the plane loop's planes."""
    lib = pkg.hip_lib.load()
    for b in wr.budget_cases(lib):
        _check(f"budget:{b['id']}", fp32_cost(b["case"] if b["node"] is None else b["node"]))
    L = wr.LOOP_SMALL
    small = wr.bands_case(8000, L["planes"], L["H"], L["W"], L["wave"], L["levels"], L["mode"])
    _check("loop:small", fp32_cost(small, slice(2046, 2051)))


def test_measured_table_names_real_cases():
    known = set()
    for group, cases in GROUPS.items():
        known |= {f"{group}#{i}" for i in range(len(cases))}
    assert all(k in known or k.startswith(("budget:", "loop:")) for k in MEASURED_FP32), sorted(set(MEASURED_FP32) - known)
    json.dumps(MEASURED_FP32)
