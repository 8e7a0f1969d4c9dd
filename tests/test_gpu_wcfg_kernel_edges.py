"""-m gpu: the fused WaveletCFG kernels (csrc/dwt_lowpass.h ``sonar_wcfg_lowpass_*``, csrc/dwt_bands.h ``sonar_wcfg_bands_*``, csrc/dwt_tile.h
``sonar_wcfg_fused_*`` and the single-level tile kernels) against the fp64 oracle (tests/wcfg_refs.py over oracle/dwt_oracle.py, pinned to
the reference-run fixtures by tests/test_wcfg_refs_cpu.py), called DIRECTLY through hip_lib at the places where their plans change route.
Every test asserts that the route it is about was taken (a tensor came back) or refused before any launch (None came back).

The edges and the test that stands at each:
   1 filter length (with_taps 2 .. 20)      test_filter_lengths: haar, db2 .. db10 (2 .. 20 taps, 14 and 18 included), bior2.2, sym7
   2 the ZERO instantiations                 test_modes (zero, and zero -> periodic), test_short_planes (all six modes)
   3 extension pairs                         test_modes: three mixed non-periodised pairs, haar with periodization on one side (both ways),
                                             db2 with periodization on one side: refused, and the node's fallback checked
   4 tile heights, W % 4                     test_tile_heights: H in 15 .. 42 around 8 / 16 / 24 / 32 / 40, W in 32 .. 35, first bad row reported
   5 the LDS budget                          test_lds_budget: accepted / refused neighbours from the library's plan queries for both kernels,
                                             both element sizes, cV kept or not; > 64 KiB launches, AHEAD on and off (by taps and by LDS),
                                             the 1024-thread instantiation
   6 the plane loop                          test_plane_loop_small (2048 + 37 planes of 8 x 10), test_plane_loop_large (256 + 5 single-workgroup
                                             fp64 planes), test_empty_batch
   7 level count                             test_levels: 8 levels everywhere, 9 refused by the two LDS kernels, FusedCall at 9 and 10
   8 planes shorter than the filter          test_short_planes: (1, 8) .. (5, 64) with haar, db4, db10 at 1 and 8 levels
   9 pointer alignment                       test_alignment: offsets 1, 2, 3 per tensor and all together, even and odd W
  10 the cV storage form                     test_scale_tables (same_v / any_v / no_b), test_hi_storage (sonar_wcfg_hi_storage 0 and 1)
  11 scales of 1, 0 and below                test_scale_tables: unit / zero / negative entries in every table position, the three blends at
                                             strengths 0, 0.35, 1
  single-level tile kernels                  test_single_level_tile_kernels, test_single_level_lds_limit

Tolerances are the project's (tests/test_gpu_wavelet.py, same oracle): outputs 2e-6 x max(1, peak) in fp64 arithmetic (the outputs are fp32
tensors), 5e-5 x max(1, peak) in fp32 arithmetic; coefficients 1e-11 / 2e-5.  None had to be measured instead: tests/test_wcfg_refs_cpu.py
runs every case of this module through the oracle in float32 and float64, and the largest fp32 cost of the operation itself is 4.9e-7 x
max(1, peak) (8 levels of db10 on a 2 x 2 plane, constant extension); 1.8e-7 for 8 levels of haar on 256 x 128, 2.9e-7 in the filter-length
sweep (sym7), 2.2e-7 on the LDS-boundary planes -- all a hundredth of 5e-5, so ``wcfg_refs.MEASURED_FP32`` is empty.

256 x 128 at 8 levels fits the two LDS kernels in fp32 arithmetic only: in fp64 their plans refuse it (asserted), and the node's route for
that rule is compared instead.

Mixed pairs with a periodised side and more than two taps have a reference result only for symmetric -> periodization at one level
(wcfg_refs.mode_cases says why); the node's fallback is compared there, the refusal is asserted for both directions at two levels."""
import importlib
import re
import types

import numpy as np
import pytest
import torch

from oracle import dwt_oracle as dwo
from tests import wcfg_refs as wr
from tests.golden.wavelet_cases import SAMPLE_SIGMAS, FakeModel

pytestmark = pytest.mark.gpu

MODEL_OPTIONS = {"transformer_options": {"sample_sigmas": SAMPLE_SIGMAS["karras12"]}}
PRECISIONS = [pytest.param(True, id="fp64"), pytest.param(False, id="fp32")]


@pytest.fixture(scope="module")
def api(pkg):
    lib = pkg.hip_lib.load()
    return types.SimpleNamespace(hl=pkg.hip_lib, lib=lib, wc=importlib.import_module("comfyui_sonar_amd.py.wavelet_cfg"))


def taps(wave):
    return dict(zip(("dec_lo", "dec_hi", "rec_lo", "rec_hi"), (list(map(float, t)) for t in dwo.taps(wave))))


def reconstructs(kw):
    flen = len(dwo.taps(kw["wave"])[0])
    return flen == 2 or (kw["mode"] == "periodization") == (kw["inv_mode"] == "periodization")


def device_inputs(c, sel=slice(None)):
    return tuple(torch.from_numpy(np.ascontiguousarray(t[:, sel])).cuda() for t in wr.inputs(c["seed"], c["planes"], c["H"], c["W"]))


def launch(api, c, hp, tensors=None, out=None):
    """The case through its entry point: the output tensor, or None when the entry point refused."""
    cond, uncond, x = device_inputs(c) if tensors is None else tensors
    kw = dict(c["kw"])
    t = taps(kw.pop("wave"))
    if c["kind"] == "node":
        rules = api.wc.WCFGRules.build(**wr.node_params(c, hp))
        fn = api.wc.WaveletCFG(existing_cfg=None, rules=rules)
        args = {"input": x, "cond_scale": 7.0, "cond": x - cond, "uncond": x - uncond, "cond_denoised": cond, "uncond_denoised": uncond,
                "sigma": torch.full((x.shape[0],), 7.0, device="cuda"), "model": FakeModel(), "model_options": MODEL_OPTIONS}
        return fn(args)
    xin = x if kw["subtract_from_x"] else None
    if c["kind"] == "bands":
        has_b = kw.pop("has_b")
        return api.hl.wcfg_bands(cond, uncond if has_b else None, xin, out, high_precision=hp, **t, **kw)
    if c["kind"] == "lowpass":
        return api.hl.wcfg_lowpass(cond, uncond, xin, dec_lo=t["dec_lo"], rec_lo=t["rec_lo"], high_precision=hp, **kw)
    call = api.hl.FusedCall(high_precision=hp, perfect_reconstruction=reconstructs(c["kw"]), **t, **kw)
    return call(cond, uncond, xin)


def tolerance(c, hp, want, ident=None):
    peak = max(1.0, float(np.abs(want).max()))
    rel = wr.TOL_OUT[hp]
    if not hp and ident in wr.MEASURED_FP32:
        rel = max(rel, 4.0 * wr.MEASURED_FP32[ident])
    return rel * peak


def compare(got, want, tol, what):
    """max |got - want| <= tol, with the first bad ROW named: a wrong tile seam shows as wrong values in the rows next to it."""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    if not np.isfinite(err).all() or float(err.max()) > tol:
        rows = np.nanmax(np.where(np.isfinite(err), err, np.inf).reshape(-1, *err.shape[-2:]), axis=(0, 2))
        bad = np.nonzero(rows > tol)[0]
        raise AssertionError(f"{what}: max error {float(np.nanmax(err)):.3g} > {tol:.3g}; first bad row {int(bad[0])} of {err.shape[-2]}, "
                             f"bad rows {bad[:12].tolist()}, per-row error there {rows[bad[:6]].tolist()}")


def check(api, c, hp, ident=None, what=""):
    got = launch(api, c, hp)
    assert got is not None, f"{what} {c['kind']}: the entry point refused a shape its plan takes"
    assert got.dtype == torch.float32 and got.is_contiguous()
    want = wr.reference(c)
    compare(got, want, tolerance(c, hp, want, ident), f"{what} {c['kind']} {c['H']}x{c['W']} {c['kw'].get('wave')} L{c['kw'].get('levels')} "
            f"{c['kw'].get('mode')}->{c['kw'].get('inv_mode')}")
    return got


def check_group(api, group, cases, hp):
    """Every case of a group; a bands / lowpass case that the plan refuses (LDS) must come back as None, and the node's route for the same
    rule is compared instead."""
    for i, c in enumerate(cases):
        if c["kind"] in ("bands", "lowpass") and not accepted(api, c, hp):
            assert launch(api, c, hp) is None, f"{group}#{i}: launched a shape the plan query refuses"
            kw = c["kw"]
            node = wr.node_case(c["seed"], c["planes"], c["H"], c["W"], kw["wave"], kw["levels"], kw["mode"], kw["inv_mode"])
            if c["kind"] == "lowpass":
                node["kw"]["yh_scales"] = [(s,) * 3 for s in wr.lowpass_weights(kw["levels"])[1]]
            c = node
        check(api, c, hp, ident=f"{group}#{i}", what=f"{group}#{i}")


def accepted(api, c, hp):
    """What the library's plan queries say about a bands / lowpass case (host functions; they restate nothing of the result)."""
    kw = c["kw"]
    flen = len(dwo.taps(kw["wave"])[0])
    m, mi, elem = wr.MODE_IDS[kw["mode"]], wr.MODE_IDS[kw["inv_mode"]], 8 if hp else 4
    if c["kind"] == "lowpass":
        return api.lib.sonar_wcfg_lowpass_lds_bytes(c["H"], c["W"], kw["levels"], flen, m, mi, elem) >= 0
    any_v = int(any(row[1] != row[2] for row in kw["yh_scales"]))
    return api.lib.sonar_wcfg_bands_lds_bytes(c["H"], c["W"], kw["levels"], flen, m, mi, elem, any_v) >= 0


# ------------------------------------------------------------------------------------------------ 1: filter lengths
FILTER = wr.filter_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("wave", list(FILTER))
def test_filter_lengths(api, wave, hp):
    check_group(api, f"filter:{wave}", FILTER[wave], hp)


# ------------------------------------------------------------------------------------------------ 2, 3: modes and pairs
MODE = wr.mode_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("key", list(MODE))
def test_modes(api, key, hp):
    wave, mode, inv_mode = key.split("-")
    ok = dict((f"{w}-{m}-{i}", a) for w, m, i, a in wr.MODE_CASES)[key]
    if ok:
        check_group(api, f"mode:{key}", MODE[key], hp)
        return
    # a periodised side against any other extension, more than two taps: both LDS kernels refuse before any launch
    for c in (wr.bands_case(1, 3, 33, 47, wave, 2, mode, inv_mode), wr.lowpass_case(2, 3, 33, 47, wave, 2, mode, inv_mode)):
        assert not accepted(api, c, hp)
        assert launch(api, c, hp) is None
    check_group(api, f"mode:{key}", MODE[key], hp)  # the node with that rule (where the reference has a result)


# ------------------------------------------------------------------------------------------------ 8: planes shorter than the filter
SHORT = wr.short_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("key", list(SHORT))
def test_short_planes(api, key, hp):
    check_group(api, f"short:{key}", SHORT[key], hp)


# ------------------------------------------------------------------------------------------------ 4: tile heights
TILE = wr.tile_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("key", list(TILE))
def test_tile_heights(api, key, hp):
    check_group(api, f"tile:{key}", TILE[key], hp)


# ------------------------------------------------------------------------------------------------ 7: level count
LEVEL = wr.level_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("key", list(LEVEL))
def test_levels(api, key, hp):
    check_group(api, f"level:{key}", LEVEL[key], hp)


def test_deep_level_limits(api):
    """kLowMaxLevels = 8 for both LDS kernels; FusedCall's resident deeper-levels call takes levels - 1 <= kDeepMaxLevels = 8 (read from
    the header, so that a changed constant changes the case list's premise loudly)."""
    src = open(api.hl.__file__.replace("hip_lib.py", "csrc/dwt_tile.h")).read()
    low = open(api.hl.__file__.replace("hip_lib.py", "csrc/dwt_lowpass.h")).read()
    assert int(re.search(r"kDeepMaxLevels = (\d+);", src).group(1)) == 8 and int(re.search(r"kLowMaxLevels = (\d+);", low).group(1)) == 8
    for hp in (True, False):
        for c in (wr.bands_case(1, 2, 256, 128, "haar", 9, "periodization"), wr.lowpass_case(2, 2, 256, 128, "haar", 9, "periodization")):
            assert not accepted(api, c, hp)
            assert launch(api, c, hp) is None
        check(api, wr.node_case(3, 2, 256, 128, "haar", 9, "periodization"), hp, what="9 levels through the node")


# ------------------------------------------------------------------------------------------------ 10, 11: scale tables
SCALE = wr.scale_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("key", list(SCALE))
def test_scale_tables(api, key, hp):
    check_group(api, f"scale:{key}", SCALE[key], hp)


def test_hi_storage(api):
    """fp64 arithmetic of the tile route with level 1's detail bands (and the resident call's cV planes) stored in fp64 and in fp32."""
    cases = [wr.fused_case(5400, 3, 40, 36, "db4", 3, "symmetric"), wr.fused_case(5401, 3, 40, 36, "db4", 3, "symmetric", tables=wr.diff_tables(3)),
             wr.fused_case(5402, 3, 37, 50, "db2", 2, "reflect")]
    assert api.lib.sonar_wcfg_hi_storage(-1) == 1
    try:
        for setting in (0, 1):
            api.lib.sonar_wcfg_hi_storage(setting)
            assert api.lib.sonar_wcfg_hi_storage(-1) == setting
            for i, c in enumerate(cases):
                check(api, c, True, what=f"hi_storage={setting}#{i}")
    finally:
        api.lib.sonar_wcfg_hi_storage(1)


# ------------------------------------------------------------------------------------------------ 9: alignment
ALIGN = wr.align_cases()


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("key", list(ALIGN))
def test_alignment(api, key, hp):
    """Views at storage offsets of 1, 2 and 3 elements, one tensor at a time and all together: the oracle's values, and the aligned
    call's bits (vec2 / vec4 only choose the access width)."""
    c = ALIGN[key]
    want = wr.reference(c)
    tol = tolerance(c, hp, want)
    base = device_inputs(c)
    aligned = launch(api, c, hp, base)
    assert aligned is not None
    compare(aligned, want, tol, f"{key} aligned")

    def shifted(t, off):
        if off == 0:
            return t
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
        view = buf[off: off + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.storage_offset() == off
        return view

    for off in (1, 2, 3):
        for who in ("a", "b", "x", "out", "all"):
            offs = [off if who in (name, "all") else 0 for name in ("a", "b", "x")]
            tensors = tuple(shifted(t, o) for t, o in zip(base, offs))
            if c["kind"] == "bands":
                out = shifted(torch.zeros_like(base[0]), off if who in ("out", "all") else 0)
                got = launch(api, c, hp, tensors, out)
                assert got is out
            elif who == "out":
                continue  # wcfg_lowpass allocates its output itself
            else:
                got = launch(api, c, hp, tensors)
            assert got is not None
            compare(got, want, tol, f"{key} {who} at offset {off}")
            assert torch.equal(got, aligned), f"{key}: {who} at offset {off} changed bits"


# ------------------------------------------------------------------------------------------------ 5: the LDS budget
@pytest.fixture(scope="module")
def budget(api):
    return wr.budget_cases(api.lib)


def _bands_route(b):
    """Restates launch_bands_z / wcfg_bands (csrc/dwt_bands.h) from the QUERIED byte count: which instantiation a launch takes."""
    lds = b["lds"]
    two_wg = 3 * (lds + 512) > 160 * 1024           # at most two workgroups fit a CU's LDS
    few_taps = b["flen"] <= 10                        # bands_rows_ahead_ok (the tensors are fp32 here)
    per_cu = max(1, min(8, (160 * 1024) // (lds + 512)))
    return dict(ahead=two_wg and few_taps, two_wg=two_wg, few_taps=few_taps, wide=b["elem"] == 8 and per_cu == 1, big=lds > 64 * 1024)


def test_lds_budget_sweep_covers_the_routes(budget):
    fits = [b for b in budget if b["lds"] >= 0]
    assert all(b["lds"] >= 0 for b in budget if b["id"].endswith(("-fits", "-small"))) and all(b["node"] is not None for b in budget if b["lds"] < 0)
    low = [b for b in fits if b["kernel"] == "lowpass"]
    bands = [_bands_route(b) for b in fits if b["kernel"] == "bands"]
    assert any(b["lds"] > 64 * 1024 for b in low) and any(r["big"] for r in bands)          # launches through lds_attr
    assert any(b["lds"] <= 80 * 1024 for b in low) and all(b["lds"] <= 80 * 1024 for b in low)
    assert all(b["lds"] <= 158 * 1024 for b in fits)
    assert any(r["few_taps"] and r["two_wg"] for r in bands) and any(r["few_taps"] and not r["two_wg"] for r in bands)
    assert any(not r["few_taps"] and r["two_wg"] for r in bands) and any(not r["few_taps"] and not r["two_wg"] for r in bands)
    assert any(r["wide"] for r in bands) and any(r["ahead"] and r["wide"] for r in bands)
    for elem in (4, 8):
        for tag in ("-v0-", "-v1-"):
            assert any(b["elem"] == elem and tag in b["id"] and b["lds"] >= 0 for b in budget) and any(
                b["elem"] == elem and tag in b["id"] and b["lds"] < 0 for b in budget)


BUDGET_IDS = [f"{k}-{w}-{lv}-e{e}{v}" for w, _m, lv, _h in wr.BUDGET_SERIES for e in (4, 8) for k, v in (("low", ""), ("bands", "-v0"), ("bands", "-v1"))]


@pytest.mark.parametrize("prefix", BUDGET_IDS)
def test_lds_budget(api, budget, prefix):
    """An accepted plane whose neighbour (one column wider) is refused: the accepted one through the direct entry point, the refused
    one asserted refused and then through WaveletCFG; plus, per band series, a small plane (three or more workgroups per CU)."""
    mine = [b for b in budget if b["id"].startswith(prefix + "-")]
    if "bands" in prefix and prefix.endswith("-v1"):
        mine += [b for b in budget if b["id"] == prefix[:-3] + "-small"]
    assert {b["id"][len(prefix) + 1:] for b in mine} >= {"fits", "refused"}
    for b in mine:
        hp = b["elem"] == 8
        if b["lds"] >= 0:
            assert accepted(api, b["case"], hp)
            check(api, b["case"], hp, ident=f"budget:{b['id']}", what=b["id"])
        else:
            assert not accepted(api, b["case"], hp)
            assert launch(api, b["case"], hp) is None, b["id"]
            check(api, b["node"], hp, ident=f"budget:{b['id']}", what=b["id"] + " (node)")


# ------------------------------------------------------------------------------------------------ 6: the plane loop
def _loop(api, c, hp, chunk, probes, what):
    """The batched call == the concatenation of calls on chunks of at most ``chunk`` planes, bit for bit; the probed plane ranges
    against the oracle."""
    tensors = device_inputs(c)
    whole = launch(api, c, hp, tensors)
    assert whole is not None
    parts = []
    for p0 in range(0, c["planes"], chunk):
        part = dict(c, planes=min(chunk, c["planes"] - p0))
        parts.append(launch(api, part, hp, tuple(t[:, p0: p0 + chunk].contiguous() for t in tensors)))
    assert torch.equal(whole, torch.cat(parts, dim=1)), f"{what}: the plane loop changed bits"
    for sel in probes:
        want = wr.reference(c, np.float64, sel)
        compare(whole[:, sel], want, tolerance(c, hp, want), f"{what} planes {sel.start}..{sel.stop}")


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("kind", ["bands", "lowpass", "fused", "fused-diff"])
def test_plane_loop_small(api, kind, hp):
    """2048 + 37 planes of 8 x 10: one workgroup runs several planes through the same LDS (grid = min(planes, 256 x per_cu))."""
    L = wr.LOOP_SMALL
    shape = (L["planes"], L["H"], L["W"], L["wave"], L["levels"], L["mode"])
    c = {"bands": wr.bands_case(8000, *shape), "lowpass": wr.lowpass_case(8001, *shape), "fused": wr.fused_case(8002, *shape),
         "fused-diff": wr.fused_case(8003, *shape, tables=wr.diff_tables(L["levels"]))}[kind]
    n = L["planes"]
    _loop(api, c, hp, 256, [slice(0, 256), slice(n - n % 256, n), slice(2046, 2051)], f"loop-small {kind}")


def test_plane_loop_large(api, budget):
    """256 + 5 planes that leave a CU ONE workgroup in fp64 arithmetic (the 1024-thread instantiation, rows requested an item ahead):
    the loop starts above 256 planes."""
    b = next(b for b in budget if b["id"] == "bands-haar-1-e8-v1-fits")
    route = _bands_route(b)
    assert route["wide"] and route["ahead"]
    c = dict(b["case"], planes=256 + 5, seed=8100)
    _loop(api, c, True, 256, [slice(0, 256), slice(256, 261), slice(254, 259)], "loop-large bands")


@pytest.mark.parametrize("hp", PRECISIONS)
def test_empty_batch(api, hp):
    """planes = 0: an empty tensor and no error from any of the three entry points (an empty batch has no storage to point at)."""
    for c in wr.three(8200, 4, 24, 36, "db4", 2, "symmetric"):
        empty = tuple(torch.empty((0, 4, 24, 36), device="cuda") for _ in range(3))
        got = launch(api, c, hp, empty)
        assert got is not None and tuple(got.shape) == (0, 4, 24, 36)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the single-level tile kernels
def _coef_close(got, want, hp, what):
    tol = wr.TOL_COEF[hp]
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), want, rtol=tol, atol=tol, err_msg=what)


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("wave,mode", [("db4", m) for m in wr.MODES] + [("dmey", "symmetric"), ("haar", "periodization"), ("db9", "zero")])
def test_single_level_tile_kernels(api, wave, mode, hp):
    """dwt2_forward / dwt2_inverse on an odd plane: the coefficients, the reconstruction from an ``ll`` one row and one column larger
    than the bands, and an ``out_hw`` smaller than the full reconstruction.  dmey (62 taps) is outside tile_taps_ok: per-pass kernels."""
    dt = torch.float64 if hp else torch.float32
    rng = np.random.default_rng(31)
    x = rng.standard_normal((2, 2, 21, 27)) + 0.25
    if not hp:
        x = x.astype(np.float32).astype(np.float64)
    t = taps(wave)
    ll, hi = api.hl.dwt2_forward(torch.from_numpy(x).to(dt).cuda(), t["dec_lo"], t["dec_hi"], mode)
    wl, whi = wr.ref_dwt2(x, wave=wave, mode=mode)
    _coef_close(ll, wl, hp, "ll")
    _coef_close(hi, whi, hp, "hi")
    h, w = whi.shape[-2:]
    big = rng.standard_normal((2, 2, h + 1, w + 1))
    big[..., :h, :w] = wl
    bands = whi * np.array([1.5, 0.5, -0.75]).reshape(3, 1, 1)
    if not hp:
        big, bands = big.astype(np.float32).astype(np.float64), bands.astype(np.float32).astype(np.float64)
    full = wr.ref_idwt2(big, bands, wave=wave, mode=mode)
    dev_ll, dev_hi = (torch.from_numpy(np.ascontiguousarray(v)).to(dt).cuda().contiguous() for v in (big, bands))
    rec = api.hl.dwt2_inverse(dev_ll, dev_hi, t["rec_lo"], t["rec_hi"], mode)
    assert tuple(rec.shape) == full.shape
    _coef_close(rec, full, hp, "full reconstruction")
    out_hw = (min(21, full.shape[-2]) - 2, min(27, full.shape[-1]) - 3)
    crop = api.hl.dwt2_inverse(dev_ll, dev_hi, t["rec_lo"], t["rec_hi"], mode, out_hw=out_hw)
    _coef_close(crop, wr.ref_idwt2(big, bands, wave=wave, mode=mode, out_hw=out_hw), hp, "cropped reconstruction")


def _fwd_lds_bytes(W, h, w, F, elem):
    """fwd_lds_bytes of csrc/dwt_tile.h for one tensor and kFwdRows = 8: picks the WIDTH under test, nothing else."""
    return 8 * 2 * (2 * ((W + 1) // 2)) * elem + (2 * w + 2 * h + 2 * F) * 4


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("mode", ["symmetric", "periodization"])
def test_single_level_lds_limit(api, mode, hp):
    """Either side of kTileLdsLimit (64 KiB): the widest plane the tile kernels take and the next one, which the per-pass kernels take;
    both must give the oracle's coefficients and reconstruction.  H = 9."""
    elem, F, H = (8 if hp else 4), 8, 9
    dt = torch.float64 if hp else torch.float32
    h = dwo.out_len(H, F, mode)
    fits = lambda W: _fwd_lds_bytes(W, h, dwo.out_len(W, F, mode), F, elem) <= 64 * 1024  # noqa: E731
    W = next(W for W in range(2048, 8, -1) if fits(W))
    assert fits(W) and not fits(W + 1) and abs(W - (510 if hp else 1020)) < 80
    # the synthesis tile: kInvRows (16) x 2 w values
    w_inv = 64 * 1024 // (16 * 2 * elem)
    t = taps("db4")
    rng = np.random.default_rng(37)
    for width in (W - 1, W, W + 1, W + 2):
        x = (rng.standard_normal((1, 3, H, width)) + 0.25).astype(np.float32).astype(np.float64)
        ll, hi = api.hl.dwt2_forward(torch.from_numpy(x).to(dt).cuda(), t["dec_lo"], t["dec_hi"], mode)
        wl, whi = wr.ref_dwt2(x, wave="db4", mode=mode)
        _coef_close(ll, wl, hp, f"ll at W = {width}")
        _coef_close(hi, whi, hp, f"hi at W = {width}")
    for w in (w_inv - 1, w_inv, w_inv + 1):
        ll = (rng.standard_normal((1, 3, h, w)) + 0.25).astype(np.float32).astype(np.float64)
        hi = rng.standard_normal((1, 3, 3, h, w)).astype(np.float32).astype(np.float64)
        rec = api.hl.dwt2_inverse(torch.from_numpy(ll).to(dt).cuda().contiguous(), torch.from_numpy(hi).to(dt).cuda().contiguous(), t["rec_lo"], t["rec_hi"], mode)
        _coef_close(rec, wr.ref_idwt2(ll, hi, wave="db4", mode=mode), hp, f"reconstruction at w = {w}")
