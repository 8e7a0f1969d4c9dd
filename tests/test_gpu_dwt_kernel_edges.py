"""-m gpu: the per-pass 2-D DWT kernels (csrc/dwt.hip ``dwt_rows_kernel``, ``dwt_cols_kernel``, ``idwt_cols_kernel``, ``idwt_rows_kernel``
over ``synth()`` of csrc/dwt_common.h) and the 1-D kernels (``dwt1_fwd_kernel``, ``dwt1_inv_kernel``), called DIRECTLY through
``hip_lib.dwt1_forward`` / ``dwt1_inverse`` / ``dwt2_forward`` / ``dwt2_inverse`` at the cases of tests/golden/dwt_edge_cases.py, against
PyWavelets 1.1.1 (tests/golden/dwt_edges.npz) where the fixture has the case and against oracle/dwt_oracle.py everywhere (the oracle is
compared with the same fixture by tests/test_dwt_edges_cpu.py).

The edges and the test that stands at each:
  E1 extension wrap                test_extension_wrap: all six modes, n in {1, 2, 3, F/2 - 1, F/2, F - 1, F, F + 1, 2F + 1}, rows of n and
                                   planes (n, m), haar / db2 / db4 (tile route, the control) and db11 / sym20 / dmey / db32 (22 .. 64 taps)
  E2 periodization                 test_periodization: odd n, n = 1, F > 2k in synthesis; the 1-D kernel's parity walk and synth()
  E3 interior / border switch      test_interior_border_switch: L = 4F + 3, 4F + 4, db4 and db11, every mode; first bad index named
  E4 crop arguments                test_crop_arguments: lo / ll one sample / row / column larger with a finite sentinel in the surplus,
                                   out_len / out_hw = full, full - 1, 1; the oversized call must return the bits of the exact one
  E5 grid-stride loops             test_grid_stride_loops: more than kMaxGrid x kBlock = 524288 work items in each of the six kernels
  E6 both precisions               every test runs the fp64 and the fp32 kernels on the same float32-representable inputs
  E7 multi-level through Wavelet   test_multi_level: 33 x 47 and 1601 samples, forward / inverse / two_step_inverse
  the 13 wavelets of 66 .. 102 taps  test_every_wavelet_transforms (all 106 names), test_long_wavelets (against PyWavelets),
                                   test_long_filter_refusals_and_fallback

Every 2-D case asserts the route that ran: the entry point is called once more with a workspace of known bytes -- the per-pass kernels
write their intermediate there, the tile kernels never touch it -- and the observation must equal what the filter length and the LDS
formula of csrc/dwt_tile.h say.  A case meant for the per-pass kernels fails if it passes through the tile kernels.

Tolerances: fp64 1e-11 x max(1, peak) (tests/test_gpu_wavelet.py).  fp32: 2e-5 x max(1, peak), unless the operation's own fp32 cost,
measured on the CPU by tests/test_dwt_edges_cpu.py (oracle in float32 against oracle in float64), exceeds a quarter of that.  It does not:
    MEASURED_FP32   E1 6.07e-07  E2 4.26e-07  E3 2.86e-07  E4 3.47e-07  LONG 4.79e-07  E5 1.82e-07  E7 5.61e-07
    bound           2e-5 for every group (a quarter of it is 5e-6; 64 products per pass of O(1) data stay a tenth of that)
A probe of the fixture (2-D: a plane's rows contracted with known weights) is allowed the bound times the sum of the weights."""
import functools
import importlib
import types

import numpy as np
import pytest
import torch

from oracle import dwt_oracle as dwo
from tests import test_dwt_edges_cpu as cpu
from tests.golden import dwt_edge_cases as ec
from tests.golden.wavelet_cases import SAMPLE_SIGMAS, FakeModel

pytestmark = pytest.mark.gpu

PRECISIONS = [pytest.param(True, id="fp64"), pytest.param(False, id="fp32")]
TOL_FP64 = 1e-11
MODEL_OPTIONS = {"transformer_options": {"sample_sigmas": SAMPLE_SIGMAS["karras12"]}}
FILL = 0xA5


@pytest.fixture(scope="module")
def api(pkg):
    lib = pkg.hip_lib.load()
    return types.SimpleNamespace(hl=pkg.hip_lib, lib=lib, wf=importlib.import_module("comfyui_sonar_amd.py.wavelet_functions"),
                                 wc=importlib.import_module("comfyui_sonar_amd.py.wavelet_cfg"))


@functools.lru_cache(maxsize=None)
def taps(wave):
    return dict(zip(("dec_lo", "dec_hi", "rec_lo", "rec_hi"), (list(map(float, t)) for t in dwo.taps(wave))))


def dev(a, hp):
    return torch.from_numpy(np.array(a, order="C")).to(torch.float64 if hp else torch.float32).cuda().contiguous()  # a copy: the references are read-only


def bound(group, hp, want):
    return (TOL_FP64 if hp else cpu.fp32_bound(group)) * max(1.0, float(np.abs(want).max()))


def compare(got, want, tol, what):
    """max |got - want| <= tol, with the first bad coefficient named (its full index; the last entry is the index along the row)."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= tol)  # a NaN is bad
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside {tol:.3g}, max error {float(np.nanmax(err)):.3g}; first bad coefficient "
                             f"at {first} (index {first[-1]} of {want.shape[-1]} along the row): got {got[first]!r}, want {want[first]!r}")


# ------------------------------------------------------------------------------------------------ references (computed once, never modified)
CASES = {c["id"]: c for c in ec.CASES}


@functools.lru_cache(maxsize=None)
def reference(ident):
    """(x, (lo_in, hi_in), (lo, hi, rec)) of a table case in fp64; the inputs are float32 values, so both precisions share it"""
    case = CASES[ident]
    x, synth_in = ec.inputs(case)
    res = cpu.oracle_results(case)
    for a in (x, *synth_in, *res):
        a.setflags(write=False)
    return x, synth_in, res


def against_fixture(case, got, tol, what):
    """row / plane [0, 0] of (lo, hi, rec) against PyWavelets, in the fixture's form"""
    if not case["pywt"]:
        return
    got = [t.detach().cpu().numpy() for t in got]
    for key, g, full in zip(ec.fixture_keys(case), cpu.fixture_form(case, got), got):
        weight = 1.0 if case["dim"] == 1 else float(ec.probe(np.ones(full.shape[-1])))  # the probe's weights are positive: their sum
        compare(g, cpu.FIX[key], tol * weight, f"{what} {key} against PyWavelets")


# ------------------------------------------------------------------------------------------------ routes
def expected_route(flen, elem, *, W=None, h=None, w=None, inverse=False):
    """tile_taps_ok and fwd_lds_bytes (kFwdRows = 8, one tensor) / inv_lds_bytes (kInvRows = 16) of csrc/dwt_tile.h against its 64 KiB limit"""
    if not (2 <= flen <= 20 and flen % 2 == 0):
        return "per-pass"
    lds = 16 * 2 * w * elem if inverse else 8 * 2 * (2 * ((W + 1) // 2)) * elem + (2 * w + 2 * h + 2 * flen) * 4
    return "tile" if lds <= 64 * 1024 else "per-pass"


def _observed(ws):
    return "per-pass" if bool((ws != FILL).any()) else "tile"


def forward_route(api, x, t, mode):
    """sonar_dwt2_fwd_* on a workspace of known bytes: (route that ran, ll, hi)"""
    hl, lib = api.hl, api.lib
    H, W = x.shape[-2:]
    planes, flen, m = x.numel() // (H * W), len(t["dec_lo"]), hl.DWT_MODE_IDS[mode]
    h, w = ec.out_len(H, flen, mode), ec.out_len(W, flen, mode)
    ll = torch.empty((*x.shape[:-2], h, w), dtype=x.dtype, device=x.device)
    hi = torch.empty((*x.shape[:-2], 3, h, w), dtype=x.dtype, device=x.device)
    need = int(lib.sonar_dwt2_ws_bytes(planes, H, W, flen, m, x.element_size(), 0))
    assert need == planes * H * 2 * w * x.element_size()
    ws = torch.full((max(need, 8),), FILL, dtype=torch.uint8, device=x.device)
    fn = lib.sonar_dwt2_fwd_f64 if x.dtype == torch.float64 else lib.sonar_dwt2_fwd_f32
    hl._check(fn(x.data_ptr(), ll.data_ptr(), hi.data_ptr(), planes, H, W, hl._darr(t["dec_lo"]), hl._darr(t["dec_hi"]), flen, m, ws.data_ptr(),
                 hl._stream()), "sonar_dwt2_fwd")
    return _observed(ws), ll, hi


def inverse_route(api, ll, hi, t, mode, out_hw=None):
    """sonar_dwt2_inv_* on a workspace of known bytes: (route that ran, out)"""
    hl, lib = api.hl, api.lib
    h, w = hi.shape[-2:]
    planes, flen, m = hi.numel() // (3 * h * w), len(t["rec_lo"]), hl.DWT_MODE_IDS[mode]
    Ho, Wo = (ec.rec_len(h, flen, mode), ec.rec_len(w, flen, mode)) if out_hw is None else out_hw
    out = torch.empty((*hi.shape[:-3], Ho, Wo), dtype=hi.dtype, device=hi.device)
    need = int(lib.sonar_dwt2_ws_bytes(planes, h, w, flen, m, hi.element_size(), 1))
    assert need == planes * 2 * ec.rec_len(h, flen, mode) * w * hi.element_size()
    ws = torch.full((max(need, 8),), FILL, dtype=torch.uint8, device=hi.device)
    fn = lib.sonar_dwt2_inv_f64 if hi.dtype == torch.float64 else lib.sonar_dwt2_inv_f32
    hl._check(fn(ll.data_ptr(), ll.shape[-2], ll.shape[-1], hi.data_ptr(), out.data_ptr(), planes, h, w, Ho, Wo, hl._darr(t["rec_lo"]),
                 hl._darr(t["rec_hi"]), flen, m, ws.data_ptr(), hl._stream()), "sonar_dwt2_inv")
    return _observed(ws), out


def assert_routes(api, what, flen, hp, x, got_fwd, ll_in, hi_in, got_inv, t, mode, want_route=None, out_hw=None):
    """both directions once more on a marked workspace: the route that ran is the one the formula gives (and ``want_route`` when the case is
    meant for one), and the marked call returns the bits of the hip_lib call"""
    elem = 8 if hp else 4
    H, W = x.shape[-2:]
    h, w = hi_in.shape[-2:]
    route, ll, hi = forward_route(api, x, t, mode)
    exp = expected_route(flen, elem, W=W, h=ll.shape[-2], w=ll.shape[-1])
    assert route == exp and (want_route is None or route == want_route), f"{what}: forward ran the {route} kernels, formula {exp}, meant {want_route}"
    assert torch.equal(ll, got_fwd[0]) and torch.equal(hi, got_fwd[1]), f"{what}: two forward calls differ"
    route, out = inverse_route(api, ll_in, hi_in, t, mode, out_hw)
    exp = expected_route(flen, elem, w=w, inverse=True)
    assert route == exp and (want_route is None or route == want_route), f"{what}: inverse ran the {route} kernels, formula {exp}, meant {want_route}"
    assert torch.equal(out, got_inv), f"{what}: two inverse calls differ"


def meant_route(case):
    """what a table case is for: 22 taps and more are the per-pass kernels' cases, db4 and shorter the tile kernels' (the control)"""
    return "per-pass" if case["flen"] > 20 else "tile"


# ------------------------------------------------------------------------------------------------ one table case
def check_case(api, case, hp):
    x, (lo_in, hi_in), (lo, hi, rec) = reference(case["id"])
    t, mode, what = taps(case["wave"]), case["mode"], f"{case['id']} {'fp64' if hp else 'fp32'}"
    dx, dlo, dhi = dev(x, hp), dev(lo_in, hp), dev(hi_in, hp)
    if case["dim"] == 1:
        ga, gd = api.hl.dwt1_forward(dx, t["dec_lo"], t["dec_hi"], mode)
        grec = api.hl.dwt1_inverse(dlo, dhi, t["rec_lo"], t["rec_hi"], mode)
    else:
        ga, gd = api.hl.dwt2_forward(dx, t["dec_lo"], t["dec_hi"], mode)
        grec = api.hl.dwt2_inverse(dlo, dhi, t["rec_lo"], t["rec_hi"], mode)
        assert_routes(api, what, case["flen"], hp, dx, (ga, gd), dlo, dhi, grec, t, mode, meant_route(case))
    for name, got, want in (("lo", ga, lo), ("hi", gd, hi), ("rec", grec, rec)):
        compare(got, want, bound(case["group"], hp, want), f"{what} {name}")
    peak = max(float(np.abs(v).max()) for v in (lo, hi, rec))
    against_fixture(case, (ga, gd, grec), bound(case["group"], hp, np.array([peak])), what)


def group_cases(group, **match):
    return [c for c in ec.CASES if c["group"] == group and all(c[k] == v for k, v in match.items())]


# ------------------------------------------------------------------------------------------------ E1
@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("wave", list(ec.E1_WAVES))
def test_extension_wrap(api, wave, mode, hp):
    cases = group_cases("E1", wave=wave, mode=mode)
    assert {c["dim"] for c in cases} == {1, 2} and len(cases) >= 8
    for case in cases:
        check_case(api, case, hp)


# ------------------------------------------------------------------------------------------------ E2
@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("wave", list(ec.E2_WAVES))
def test_periodization(api, wave, hp):
    cases = group_cases("E2", wave=wave)
    flen = ec.E2_WAVES[wave]
    ks = [ec.out_len(c["shape"][0], flen, "periodization") for c in cases if c["dim"] == 1]
    assert 1 in ks and any(flen > 2 * k for k in ks) and any(c["shape"][0] % 2 for c in cases)
    for case in cases:
        check_case(api, case, hp)


# ------------------------------------------------------------------------------------------------ E3
@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("wave", list(ec.E3_WAVES))
def test_interior_border_switch(api, wave, mode, hp):
    """dwt1_fwd_kernel reads the taps straight when ``top < L && top - (F - 1) >= 0``: with L = 4F + 3 and 4F + 4 the switch falls on both
    parities of L at the right end, and F / 2 coefficients in at the left; compare() names the first bad coefficient index."""
    for case in group_cases("E3", wave=wave, mode=mode):
        check_case(api, case, hp)


# ------------------------------------------------------------------------------------------------ LONG against PyWavelets
@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("wave", list(ec.LONG_WAVES))
def test_long_wavelets(api, wave, hp):
    for case in group_cases("LONG", wave=wave):
        check_case(api, case, hp)


# ------------------------------------------------------------------------------------------------ E4
@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("mode", ec.E4_MODES)
@pytest.mark.parametrize("wave", list(ec.E4_WAVES))
def test_crop_arguments(api, wave, mode, hp):
    """``lo`` / ``ll`` one sample / row / column larger than the bands, SENTINEL in the surplus: the result is that of the exact band, bit for
    bit (the same kernel on the same numbers: any difference is a read of the surplus), at out_len / out_hw = full, full - 1 and 1."""
    t, flen = taps(wave), ec.E4_WAVES[wave]
    for case in group_cases("E4", wave=wave, mode=mode):
        check_case(api, case, hp)
        _, (lo_in, hi_in), (_, _, rec) = reference(case["id"])
        what = f"{case['id']} {'fp64' if hp else 'fp32'}"
        pad = [(0, 0)] * (lo_in.ndim - case["dim"]) + [(0, 1)] * case["dim"]
        big = np.pad(lo_in, pad, constant_values=ec.SENTINEL)
        assert big.shape[-1] == lo_in.shape[-1] + 1 and big[..., -1].min() == ec.SENTINEL
        dlo, dbig, dhi = dev(lo_in, hp), dev(big, hp), dev(hi_in, hp)
        if case["dim"] == 1:
            full = rec.shape[-1]
            for n in (full, full - 1, 1):
                exact = api.hl.dwt1_inverse(dlo, dhi, t["rec_lo"], t["rec_hi"], mode, out_len=n)
                got = api.hl.dwt1_inverse(dbig, dhi, t["rec_lo"], t["rec_hi"], mode, out_len=n)
                want = rec[..., :n]
                compare(got, want, bound("E4", hp, rec), f"{what} out_len {n} of {full}, oversized lo")
                compare(exact, want, bound("E4", hp, rec), f"{what} out_len {n} of {full}")
                assert torch.equal(got, exact), f"{what} out_len {n}: the surplus sample of lo leaked"
            continue
        fh, fw = rec.shape[-2:]
        for hw in ((fh, fw), (fh - 1, fw - 1), (fh, 1), (1, 1)):
            exact = api.hl.dwt2_inverse(dlo, dhi, t["rec_lo"], t["rec_hi"], mode, out_hw=hw)
            got = api.hl.dwt2_inverse(dbig, dhi, t["rec_lo"], t["rec_hi"], mode, out_hw=hw)
            want = rec[..., :hw[0], :hw[1]]
            compare(got, want, bound("E4", hp, rec), f"{what} out_hw {hw} of {(fh, fw)}, oversized ll")
            compare(exact, want, bound("E4", hp, rec), f"{what} out_hw {hw} of {(fh, fw)}")
            assert torch.equal(got, exact), f"{what} out_hw {hw}: the surplus row / column of ll leaked"
            route, marked = inverse_route(api, dbig, dhi, t, mode, hw)
            assert route == meant_route(case) == expected_route(flen, 8 if hp else 4, w=hi_in.shape[-1], inverse=True), (what, hw, route)
            assert torch.equal(marked, got)


# ------------------------------------------------------------------------------------------------ E5
@functools.lru_cache(maxsize=None)
def grid_reference(dim):
    spec = ec.E5_1D if dim == 1 else ec.E5_2D
    x = ec.big_inputs(f"E5-{dim}d", spec["batch"], spec["shape"])
    if dim == 1:
        dec_lo, dec_hi, rec_lo, rec_hi = dwo.taps(spec["wave"])
        lo, hi = dwo.dwt_axis(x, dec_lo, dec_hi, spec["mode"], -1)
        lo_in, hi_in = ec._f32(lo), ec._f32(hi)
        rec = dwo.idwt_axis(lo_in, hi_in, rec_lo, rec_hi, spec["mode"], -1)
    else:
        lo, hi = dwo.dwt2(x, spec["wave"], spec["mode"])
        lo_in, hi_in = ec._f32(lo), ec._f32(hi)
        rec = dwo.idwt2(lo_in, hi_in, spec["wave"], spec["mode"])
    for a in (x, lo, hi, lo_in, hi_in, rec):
        a.setflags(write=False)
    return x, lo, hi, lo_in, hi_in, rec


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("dim", [1, 2])
def test_grid_stride_loops(api, dim, hp):
    """grid_for caps every grid at kMaxGrid = 2048 blocks of kBlock = 256 threads: above 524288 work items a thread takes a second trip
    round its loop.  All six kernels get there, none stays at one trip: dwt1_fwd (2056 rows x 256 coefficients), dwt1_inv (2056 x 510),
    dwt_rows (480 planes x 4 x 551), dwt_cols (480 x 3 x 551), idwt_cols (480 x 4 x 551), idwt_rows (480 x 4 x 1100).  The 2-D plane is db2
    on 4 x 1100: wider than the tile kernels' LDS tile in both precisions, so the per-pass kernels run (asserted)."""
    spec = ec.E5_1D if dim == 1 else ec.E5_2D
    x, lo, hi, lo_in, hi_in, rec = grid_reference(dim)
    t, mode, what = taps(spec["wave"]), spec["mode"], f"E5 {dim}-D {'fp64' if hp else 'fp32'}"
    flen = len(t["dec_lo"])
    if dim == 1:
        rows = x.size // x.shape[-1]
        assert rows * lo.shape[-1] > ec.GRID_ITEMS and rows * rec.shape[-1] > ec.GRID_ITEMS and rows * lo.shape[-1] < 2 * ec.GRID_ITEMS
        ga, gd = api.hl.dwt1_forward(dev(x, hp), t["dec_lo"], t["dec_hi"], mode)
        grec = api.hl.dwt1_inverse(dev(lo_in, hp), dev(hi_in, hp), t["rec_lo"], t["rec_hi"], mode)
    else:
        planes, (H, W), (h, w) = x.size // (x.shape[-1] * x.shape[-2]), x.shape[-2:], lo.shape[-2:]
        Hr, Wr = rec.shape[-2:]
        for items in (planes * H * w, planes * h * w, planes * Hr * w, planes * Hr * Wr):
            assert items > ec.GRID_ITEMS
        dx, dlo, dhi = dev(x, hp), dev(lo_in, hp), dev(hi_in, hp)
        ga, gd = api.hl.dwt2_forward(dx, t["dec_lo"], t["dec_hi"], mode)
        grec = api.hl.dwt2_inverse(dlo, dhi, t["rec_lo"], t["rec_hi"], mode)
        assert_routes(api, what, flen, hp, dx, (ga, gd), dlo, dhi, grec, t, mode, "per-pass")
    for name, got, want in (("lo", ga, lo), ("hi", gd, hi), ("rec", grec, rec)):
        compare(got, want, bound("E5", hp, want), f"{what} {name}")


# ------------------------------------------------------------------------------------------------ E7
@functools.lru_cache(maxsize=None)
def level_reference(wave, mode, level, one_d):
    shape = ec.E7_ROW if one_d else ec.E7_PLANE
    x = ec.big_inputs(f"E7-{wave}-{len(shape)}d", ec.BATCH, shape)
    dec, rec = (dwo.wavedec1, dwo.waverec1) if one_d else (dwo.wavedec2, dwo.waverec2)
    yl, yh = dec(x, wave, mode, level)
    yl_in, yh_in = ec._f32(yl), [ec._f32(b) for b in yh]
    back = rec(yl_in, yh_in, wave, mode)
    for a in (x, yl, *yh, yl_in, *yh_in, back):
        a.setflags(write=False)
    return x, yl, yh, yl_in, yh_in, back


@pytest.mark.parametrize("hp", PRECISIONS)
@pytest.mark.parametrize("wave,mode,level,one_d", [(*c, False) for c in ec.E7_2D] + [(*c, True) for c in ec.E7_1D])
def test_multi_level(api, wave, mode, level, one_d, hp):
    """``Wavelet`` over several levels of a 22 .. 62-tap filter: from the second level on every plane is shorter than the filter, and the
    coarser approximation is one row / column / sample larger than its band where the level below had an odd size."""
    x, yl, yh, yl_in, yh_in, back = level_reference(wave, mode, level, one_d)
    what = f"E7 {wave} {mode} L{level} {'1-D' if one_d else '2-D'} {'fp64' if hp else 'fp32'}"
    wv = api.wf.Wavelet(wave=wave, level=level, mode=mode, use_1d_dwt=one_d)
    gl, gh = wv.forward(dev(x, hp))
    assert len(gh) == level
    compare(gl, yl, bound("E7", hp, yl), f"{what} yl")
    for j in range(level):
        compare(gh[j], yh[j], bound("E7", hp, yh[j]), f"{what} yh[{j}]")
    dl, dh = dev(yl_in, hp), [dev(b, hp) for b in yh_in]
    compare(wv.inverse(dl, dh), back, bound("E7", hp, back), f"{what} inverse")
    compare(wv.inverse(dl, dh, two_step_inverse=True), back, bound("E7", hp, back), f"{what} two_step_inverse")


# ------------------------------------------------------------------------------------------------ all 106 wavelets
def test_every_wavelet_transforms(api):
    """Every advertised name transforms a (1, 2, 24, 20) plane and a (1, 2, 50) row: symmetric, one level, fp64, oracle at 1e-11.  Before
    the per-pass and 1-D kernels took 102 taps this failed for db33 .. db38 and coif11 .. coif17 with "1..64 filter taps required"."""
    names = api.wf.Wavelet.wavelist()
    assert len(names) == 106 and set(ec.LONG_WAVES) <= set(names)
    plane, row = ec.big_inputs("every-2d", (1, 2), (24, 20)), ec.big_inputs("every-1d", (1, 2), (50,))
    failed = {}
    for name in names:
        try:
            for x, one_d, dec in ((plane, False, dwo.wavedec2), (row, True, dwo.wavedec1)):
                wv = api.wf.Wavelet(wave=name, level=1, mode="symmetric", use_1d_dwt=one_d)
                gl, gh = wv.forward(dev(x, True))
                yl, yh = dec(x, name, "symmetric", 1)
                compare(gl, yl, bound("LONG", True, yl), f"{name} yl")
                compare(gh[0], yh[0], bound("LONG", True, yh[0]), f"{name} yh")
        except (AssertionError, api.hl.SonarHipError) as e:
            failed[name] = str(e)[:160]
    assert not failed, f"{len(failed)} of {len(names)} wavelets: {failed}"


@pytest.mark.parametrize("hp", PRECISIONS)
def test_long_filter_refusals_and_fallback(api, hp):
    """The entry points that keep the 20-tap rule refuse coif17 (102 taps) before any launch -- None comes back -- and WaveletCFG with that
    wavelet gives ``dwo.wavelet_cfg``'s result through its per-pass fallback."""
    rng = np.random.default_rng(1702)
    shape = (2, 4, 32, 28)
    cond, uncond, x = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) for _ in range(3))
    t, level = taps("coif17"), 2
    dc, du, dx = cond.cuda(), uncond.cuda(), x.cuda()
    elem = 8 if hp else 4
    assert api.lib.sonar_wcfg_lowpass_lds_bytes(32, 28, level, 102, 1, 1, elem) < 0
    assert api.hl.wcfg_lowpass(dc, du, dx, levels=level, dec_lo=t["dec_lo"], rec_lo=t["rec_lo"], mode="symmetric", inv_mode="symmetric",
                               g=[1.0] * (level + 1), ku=1.0, kt=1.0, subtract_from_x=True, high_precision=hp) is None
    assert api.hl.wcfg_bands(dc, du, dx, levels=level, **t, mode="symmetric", inv_mode="symmetric", yh_scales=[(1.0, 1.0, 1.0)] * level,
                             yl_scale=1.0, ku=1.0, kt=1.0, subtract_from_x=True, high_precision=hp) is None
    fused = api.hl.FusedCall(levels=level, **t, mode="symmetric", inv_mode="symmetric", yl_scales=[1.0] * 4,
                             yh_scales=[[(1.0,) * 3] * 4] * level, blend_mode="lerp", strength=0.5, subtract_from_x=True, high_precision=hp)
    assert fused(dc, du, dx) is None
    with pytest.raises(api.hl.SonarHipError, match="1..102 filter taps required"):
        api.hl.dwt1_forward(dx, [0.0] * 104, [0.0] * 104, "symmetric")
    params = dict(difference=dict(yl_scale=2.0, yh_scales=[1.5, 0.5]), wave="coif17", level=level, difference_blend_mode="lerp",
                  difference_blend_strength=0.8, high_precision_mode=hp)
    rules = api.wc.WCFGRules.build(**params)
    fn = api.wc.WaveletCFG(existing_cfg=None, rules=rules)
    args = {"input": dx, "cond_scale": 7.0, "cond": dx - dc, "uncond": dx - du, "cond_denoised": dc, "uncond_denoised": du,
            "sigma": torch.full((2,), 7.0, device="cuda"), "model": FakeModel(), "model_options": MODEL_OPTIONS}
    out = fn(args)
    assert out.is_contiguous() and out.shape == x.shape and out.dtype == torch.float32
    dt = np.float64 if hp else np.float32
    res = dwo.wavelet_cfg(cond.numpy().astype(dt), uncond.numpy().astype(dt), "coif17", "symmetric", level, diff_scales=(2.0, [1.5, 0.5]),
                          strength=0.8, blend="lerp")
    want = x.numpy().astype(np.float64) - res[..., :32, :28].astype(np.float32).astype(np.float64)
    compare(out, want, (2e-6 if hp else 5e-5) * max(1.0, float(np.abs(want).max())), "WaveletCFG coif17")
