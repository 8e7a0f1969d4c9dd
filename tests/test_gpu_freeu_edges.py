"""-m gpu: the four kernels of csrc/freeu.hip through the C ABI (sonar_freeu_hidden_mean, sonar_freeu_apply; ctypes on hip_lib.load()), at
their plan, access, group and window edges, against the fp64 statements of tests/freeu_edge_refs.py.  The test chooses the strides, the
pointer offsets, the channel window, the workspace size and the mean / extremes buffers itself; the inputs are freeu_refs.make_input
normals with per-sample offsets, so a mis-indexed element is an O(1) error.

Bounds, all derived (tests/freeu_edge_refs.py states them):
    hidden mean    mean_bound: the depth of the kernel's summation tree times 2^-24 of mean_c |x|, per position; the extremes are
                   bit-equal to (min, max) of the device's own map.
    sweep kernel   the count of fp32 roundings of the finishing expression times 2^-24 of the magnitudes involved (apply_abi_ref,
                   with_bound), plus one rounding of a 16-bit output.
    fused kernel   8 max(E_size, E) of the statement's range per element, plus one rounding of a 16-bit output: E is the reference's own
                   fp32 distance from the fp64 statement over the small golden planes (tests/golden/freeu_extreme.npz), E_size the same
                   measured at the very size on this test's input and filter (tests/golden/freeu_edges.npz), 8 this operation's margin
                   (tests/test_gpu_freeu.py).
SONAR_ORACLE_ERRORS=<file> writes the fused kernel's measured distance per size and dtype next to E_size (profiles/freeu_edges.txt)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import freeu_edge_refs as F
from tests import freeu_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SENT = 7.0   # the fill of everything a kernel must not touch (exact in all three dtypes)
SCALE, BLEND = 1.3, F.f32(0.7)
MEASURED: dict = {}


@pytest.fixture(scope="module")
def hl(pkg):
    pkg.hip_lib.load()
    return pkg.hip_lib


@pytest.fixture(scope="module")
def lib(hl):
    return hl.load()


@pytest.fixture(scope="module")
def E():
    return R.reference_error(dict(np.load(os.path.join(ROOT, "tests", "golden", "freeu_extreme.npz"), allow_pickle=False)))


@pytest.fixture(scope="module")
def e_size():
    g = np.load(os.path.join(ROOT, "tests", "golden", "freeu_edges.npz"), allow_pickle=False)
    return {(int(h), int(w)): float(e) for (h, w), e in zip(g["sizes"], g["e_size"])}


@pytest.fixture(scope="module", autouse=True)
def _report_measured():
    yield
    path = os.environ.get("SONAR_ORACLE_ERRORS")
    if path:
        seen = {}
        if os.path.exists(path):  # (tests/test_gpu_power_any_sites.py and tests/test_gpu_generate_oracle.py write the same file)
            with open(path) as f:
                seen = json.load(f)
        seen.update(MEASURED)
        with open(path, "w") as f:
            json.dump(seen, f, indent=1)


def _st():
    return torch.cuda.current_stream().cuda_stream


def each_case(cases, body):
    """Run body(*case) for every case and report all that fail together: the cases of one kernel edge are one test (the suite's count of
    test ids stays small), yet a failure names every case it has.  Anything but a failed assertion -- a device error -- ends the test."""
    failed = []
    for case in cases:
        try:
            body(*case)
        except AssertionError as e:
            failed.append(f"{case}: {str(e).splitlines()[0] if str(e) else 'assert'}")
    assert not failed, f"{len(failed)} of {len(cases)} cases:\n" + "\n".join(failed)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


class View:
    """x [B, C, HW] laid into a flat buffer of SENT at element `off` with the strides (sb, sc): what the kernels are handed."""

    def __init__(self, x, dname, sb=None, sc=None, off=0, pad=8):
        B, C, HW = x.shape
        self.shape, self.dname = (B, C, HW), dname
        self.sc = HW if sc is None else sc
        self.sb = C * self.sc if sb is None else sb
        n = off + max(B - 1, 0) * self.sb + (C - 1) * self.sc + HW + pad
        self.buf = torch.full((n,), SENT, dtype=DT[dname], device="cuda")
        b, c, p = np.meshgrid(np.arange(B), np.arange(C), np.arange(HW), indexing="ij")
        self.idx = torch.from_numpy(off + b * self.sb + c * self.sc + p).cuda()
        self.buf[self.idx] = torch.from_numpy(x).to(DT[dname]).cuda()
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + off * self.buf.element_size()
        self.x64 = self.before[self.idx].float().cpu().numpy().astype(np.float64)  # the input as the kernel sees it

    def values(self):
        return self.buf[self.idx].float().cpu().numpy().astype(np.float64)

    def untouched_outside(self, c0=0, cn=0):
        """Everything but the channels c0 .. c0 + cn - 1 of the view -- the other channels and the storage around it -- is bit-identical."""
        now = self.buf.clone()
        win = self.idx[:, c0:c0 + cn].reshape(-1)
        now[win] = self.before[win]
        return torch.equal(now.view(torch.uint8), self.before.view(torch.uint8))


# ---- hidden mean -----------------------------------------------------------------------------------------------------------------------------
def run_hidden_mean(lib, v, form, want):
    """One call of sonar_freeu_hidden_mean on a View with the workspace of `form`; checks everything but the values of the mean.
    Returns (mean [B, HW], extremes [B, 2]) as float64 numpy, (groups, per_group) as run."""
    B, C, HW = v.shape
    room = F.ws_room(form, want)
    mean = torch.full((B * HW + 16,), SENT, device="cuda")
    ext = torch.full((2 * B + 8,), SENT, device="cuda")
    ws = None if room == 0 else torch.full((room * B * HW + 32,), SENT, device="cuda")
    rc = lib.sonar_freeu_hidden_mean(F.DTYPE_ID[v.dname], v.ptr, B, C, HW, v.sb, v.sc, mean.data_ptr(), ext.data_ptr(), _ptr(ws), room * B * HW, _st())
    assert rc == 0
    groups, per = F.groups_run(C, want, room)
    m = mean[:B * HW].view(B, HW)
    assert (mean[B * HW:] == SENT).all() and (ext[2 * B:] == SENT).all()
    if ws is not None:
        assert (ws[(groups * B * HW if groups > 1 else 0):] == SENT).all(), "the workspace past the groups that ran"
    assert v.untouched_outside()
    mn, mx = m.min(dim=1).values, m.max(dim=1).values
    nan = m.isnan().any(dim=1)
    e = ext[:2 * B].view(B, 2)
    want_ext = torch.stack([torch.where(nan, torch.full_like(mn, float("nan")), mn), torch.where(nan, torch.full_like(mx, float("nan")), mx)], dim=1)
    assert torch.equal(e.view(torch.int32)[~nan], want_ext.view(torch.int32)[~nan]), "extremes are not (min, max) of the device's own map, bit for bit"
    assert e[nan].isnan().all()
    return m.cpu().numpy().astype(np.float64), e.cpu().numpy().astype(np.float64), (groups, per)


MEAN_PARAMS = [(shape, want, dname, form) for shape, want, dtypes, _what in F.MEAN_CASES for dname in dtypes for form in F.WS_FORMS]


def _mean_case(lib, shape, want, dname, form):
    v = View(F.mean_input(shape, 40 + shape[1]), dname)
    m, _e, (groups, per) = run_hidden_mean(lib, v, form, want)
    ref, _ = F.hidden_mean_ref(v.x64)
    err, bound = np.abs(m - ref), F.mean_bound(v.x64, per, groups)
    print(f"{shape} {dname} {form}: groups {groups} x {per}, max |mean - ref| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), f"mean past its bound, {float((err / bound).max()):.3f} x"


def test_hidden_mean_groups_and_workspaces(lib):
    """Every case of MEAN_CASES in its dtypes, each with the four workspace forms; and B = 0, which returns SONAR_OK and writes nothing."""
    each_case(MEAN_PARAMS, lambda *c: _mean_case(lib, *c))
    v = View(F.mean_input((1, 8, 64), 1), "float32")
    mean, ext, ws = (torch.full((64,), SENT, device="cuda") for _ in range(3))
    assert lib.sonar_freeu_hidden_mean(0, v.ptr, 0, 8, 64, 512, 64, mean.data_ptr(), ext.data_ptr(), ws.data_ptr(), 64, _st()) == 0
    assert (mean == SENT).all() and (ext == SENT).all() and (ws == SENT).all() and v.untouched_outside()


def test_hidden_mean_on_a_view_inside_a_larger_tensor(lib):
    """stride_c > HW, stride_b > C * stride_c, the base pointer one element into the storage (aligned to the element size only)."""
    def case(shape, want, dname, form):
        B, C, HW = shape
        sc = HW + 3
        v = View(F.mean_input(shape, 60 + C), dname, sb=C * sc + 5, sc=sc, off=1)
        m, _e, (groups, per) = run_hidden_mean(lib, v, form, want)
        assert (np.abs(m - F.hidden_mean_ref(v.x64)[0]) <= F.mean_bound(v.x64, per, groups)).all(), "mean past its bound"

    each_case([(shape, want, dname, form) for shape, want in (((3, 96, 70), 3), ((2, 5, 64), 1), ((1, 100, 100), 3)) for dname in R.DTYPES
               for form in ("helper", "null")], case)


def test_hidden_mean_nan_in_the_last_group_at_a_tail_position(lib):
    def case(dname, form):
        x = F.mean_input((3, 96, 70), 77)
        x[1, 95, 69] = np.nan  # the last channel of the last group, the last position of the tail chunk
        m, e, _ = run_hidden_mean(lib, View(x, dname), form, 3)
        assert np.isnan(e[1]).all() and np.isfinite(e[[0, 2]]).all(), f"extremes {e.tolist()}"
        assert np.isnan(m[1, 69]) and np.isnan(m).sum() == 1, "the NaN is not at its one position of the map"

    each_case([(dname, form) for dname in R.DTYPES for form in ("helper", "two", "null")], case)


# ---- the sweep kernel: PLAIN and FILTERED ----------------------------------------------------------------------------------------------------
def run_apply(lib, v, H, W, c0, cn, mode, *, filt=None, filtered=None, mean=None, extremes=None, blend_mode=F.BLEND_NONE, B=None):
    Bv, C, _HW = v.shape
    keep = [_dev(a) for a in (filt, filtered, mean, extremes)]
    rc = lib.sonar_freeu_apply(F.DTYPE_ID[v.dname], v.ptr, Bv if B is None else B, C, H, W, v.sb, v.sc, c0, cn, mode, _ptr(keep[0]), _ptr(keep[1]),
                               _ptr(keep[2]), _ptr(keep[3]), SCALE, blend_mode, BLEND, _st())
    torch.cuda.synchronize()  # (keeps the argument tensors alive until the kernel has read them)
    return rc


def _sweep_id(case):
    (h, w, off, ds), dname, mode, kind, bm, (c0, cn) = case
    return f"{h}x{w}+{off}s{ds}-{dname}-{'plain' if mode == F.PLAIN else 'filtered'}-{kind}-blend{bm}-c{c0}n{cn}"


def _sweep_case(lib, *case):
    (H, W, off, ds), dname, mode, kind, blend_mode, (c0, cn) = case
    B, C, HW = 2, F.SWEEP_C, H * W
    sc = HW + ds
    v = View(R.make_input((B, C, H, W), 900 + 10 * HW + off + ds).reshape(B, C, HW), dname, sb=C * sc, sc=sc, off=off)
    x64 = v.x64.reshape(B, C, H, W)
    filtered = np.random.default_rng(5).standard_normal((B, cn, H, W)).astype(np.float32) if mode == F.FILTERED else None
    mean, ext = F.mean_arrays(x64) if kind == "map" else (None, None)
    assert run_apply(lib, v, H, W, c0, cn, mode, filtered=filtered, mean=mean, extremes=ext, blend_mode=blend_mode) == 0
    st, bound = F.apply_abi_ref(x64, c0, cn, mode, filtered=filtered, mean=mean, extremes=ext, scale=SCALE, blend_mode=blend_mode, blend=BLEND,
                                with_bound=True)
    if dname != "float32":
        bound = bound + R.HALF_EPS[dname] * np.abs(st)
    err = np.abs(v.values().reshape(st.shape) - st)
    worst = (err[:, c0:c0 + cn] / bound[:, c0:c0 + cn]).max()
    print(f"{_sweep_id(case)}: max err / bound = {worst:.3f}")
    assert (err[:, c0:c0 + cn] <= bound[:, c0:c0 + cn]).all(), f"past the bound, {worst:.3f} x"
    assert v.untouched_outside(c0, cn), "a channel outside the window or storage outside the view changed"  # bit-identical


def test_sweep_kernel_widths_modes_and_windows(lib):
    """SWEEP_CASES: the three access widths (by HW, by pointer offset, by stride) pairwise with dtype, mode, scale kind, blend and window;
    and cn = 0 and B = 0, which write nothing."""
    each_case(F.SWEEP_CASES, lambda *c: _sweep_case(lib, *c))
    for dname in R.DTYPES:
        v = View(R.make_input((2, 5, 4, 4), 3).reshape(2, 5, 16), dname)
        mean, ext = F.mean_arrays(v.x64)
        assert run_apply(lib, v, 4, 4, 2, 0, F.PLAIN, mean=mean, extremes=ext, blend_mode=F.LERP) == 0 and v.untouched_outside()
        assert run_apply(lib, v, 4, 4, 0, 5, F.PLAIN, mean=mean, extremes=ext, blend_mode=F.LERP, B=0) == 0 and v.untouched_outside()


def test_sweep_kernel_flat_map_gives_the_statements_nans(lib):
    """extremes with hi == lo: 0 / 0 where the mean is at that value, x / 0 elsewhere -- the statement's NaN / inf pattern, signs included."""
    each_case([(m,) for m in (F.BLEND_NONE, F.LERP, F.INJECT, F.SUBTRACT_B)], lambda m: _flat_map_case(lib, m))


def _flat_map_case(lib, blend_mode):
    v = View(R.make_input((2, 5, 4, 4), 4).reshape(2, 5, 16), "float32")
    x64 = v.x64.reshape(2, 5, 4, 4)
    mean, ext = F.mean_arrays(x64)
    flat = np.stack([ext[:, 0], ext[:, 0]], axis=1)
    assert run_apply(lib, v, 4, 4, 0, 5, F.PLAIN, mean=mean, extremes=flat, blend_mode=blend_mode) == 0
    with np.errstate(all="ignore"):
        st = F.apply_abi_ref(x64, 0, 5, F.PLAIN, mean=mean, extremes=flat, scale=SCALE, blend_mode=blend_mode, blend=BLEND)
    got = v.values().reshape(st.shape)
    assert np.isnan(st).sum() >= 10 and not np.isfinite(st).any()
    assert np.array_equal(np.isnan(got), np.isnan(st)) and np.array_equal(np.isposinf(got), np.isposinf(st)) and np.array_equal(np.isneginf(got), np.isneginf(st))


# ---- the fused kernel ------------------------------------------------------------------------------------------------------------------------
FUSED_FORMS = {"float32": ("map", F.LERP), "float16": ("scalar", F.BLEND_NONE), "bfloat16": ("map", F.INJECT)}


def run_fused(lib, x, filt, dname, c0, cn, kind, blend_mode, off=0):
    """sonar_freeu_apply FUSED on x [B, C, H, W] (fp32 numpy) laid densely at element `off` of a buffer.  Returns (device result as
    float64, the fp64 statement of the upcast input, the bits of the view as a tensor)."""
    B, C, H, W = x.shape
    v = View(x.reshape(B, C, H * W), dname, off=off)
    x64 = v.x64.reshape(x.shape)
    mean, ext = F.mean_arrays(x64) if kind == "map" else (None, None)
    assert run_apply(lib, v, H, W, c0, cn, F.FUSED, filt=filt, mean=mean, extremes=ext, blend_mode=blend_mode) == 0
    assert v.untouched_outside(c0, cn)
    st = F.apply_abi_ref(x64, c0, cn, F.FUSED, filt=filt, mean=mean, extremes=ext, scale=SCALE, blend_mode=blend_mode, blend=BLEND)
    return v.values().reshape(x.shape), st, v.buf[v.idx].clone()


def fused_bound(st, dname, E, es):
    return 8 * max(es, E) * R.spread(st) + (R.HALF_EPS[dname] * np.abs(st) if dname != "float32" else 0.0)


FUSED_SIZES = F.FREEU_SWEEP + F.FREEU_FIXED
FUSED_PARAMS = [(hw, dname) for i, hw in enumerate(FUSED_SIZES) for dname in R.DTYPES if dname != "bfloat16" or i % 4 == 0]


def test_fused_kernel_at_every_site(lib, E, e_size):
    """Four planes (channels 1 and 2 of three, two samples) at every size of FREEU_SWEEP and at the twelve fixed planes: float32 with the
    map and lerp, float16 with the scalar and no blend, bfloat16 (every fourth size) with the map and inject."""
    each_case(FUSED_PARAMS, lambda hw, dname: _fused_case(lib, E, e_size, hw, dname))


def _fused_case(lib, E, e_size, hw, dname):
    x, filt = F.fused_inputs(hw)
    kind, blend_mode = FUSED_FORMS[dname]
    got, st, _ = run_fused(lib, x, filt, dname, *F.FUSED_WINDOW, kind, blend_mode)
    err = np.abs(got - st)
    MEASURED[f"freeu_edges fused | {hw[0]}x{hw[1]} | {dname}"] = (float(err.max() / R.spread(st)), e_size[hw])
    print(f"{hw[0]}x{hw[1]} {dname}: max |kernel - statement| / range = {err.max() / R.spread(st):.3e}, E_size = {e_size[hw]:.3e}")
    assert (err <= fused_bound(st, dname, E, e_size[hw])).all(), f"past the bound, {float((err / fused_bound(st, dname, E, e_size[hw])).max()):.3f} x"


def test_fused_kernel_access_forms_agree_bit_for_bit(lib, E, e_size):
    """ACCESS_SIZES in the three dtypes.  Aligned (four elements per access at 14 x 28, pairs elsewhere), the base pointer one element off (element by element) and, at
    14 x 28, two elements off (pairs on a size that would take four): each within the bound, and the same bits -- the arithmetic does
    not depend on the access form."""
    def case(hw, dname):
        x, filt = F.fused_inputs(hw)
        es = e_size.get(hw, 0.0)
        bits = {}
        for off in (0, 1, 2) if hw == (14, 28) else (0, 1):
            got, st, bits[off] = run_fused(lib, x, filt, dname, *F.FUSED_WINDOW, "map", F.LERP, off=off)
            assert (np.abs(got - st) <= fused_bound(st, dname, E, es)).all(), f"pointer {off} elements off: past the bound"
        for off in bits:
            assert torch.equal(bits[off].view(torch.uint8), bits[0].view(torch.uint8)), f"pointer {off} elements off: other bits than aligned"

    each_case([(hw, dname) for hw in F.ACCESS_SIZES for dname in R.DTYPES], case)


def test_fused_kernel_plane_loop_both_workgroup_sizes(lib, E, e_size):
    """More planes than resident workgroups: 600 at 4 x 6 (512 workgroups of 512 threads: 88 of them take a second plane, behind the
    barrier that guards the plane buffer) and 260 at the smallest size of the sweep planned with 1024 threads (256 workgroups).  fp16 with
    the map; every plane is compared."""
    big = min((hw for hw in F.FREEU_SWEEP if F.freeu_plan(lib, *hw)["threads"] == 1024), key=lambda hw: hw[0] * hw[1])
    assert F.freeu_plan(lib, 4, 6)["threads"] == 512
    for hw, (B, C, c0, cn) in (((4, 6), (3, 202, 1, 200)), (big, (2, 131, 1, 130))):
        assert B * cn > 256 * (2 if hw == (4, 6) else 1)
        x, filt = F.fused_inputs(hw, B, C)
        got, st, _ = run_fused(lib, x, filt, "float16", c0, cn, "map", F.LERP)
        err, bound = np.abs(got - st), fused_bound(st, "float16", E, e_size.get(hw, 0.0))
        worst = (err / bound).reshape(B, C, -1).max(axis=2)
        print(f"{hw} x {B * cn} planes: worst plane at {np.unravel_index(worst.argmax(), worst.shape)}, err / bound = {worst.max():.3f}")
        assert (err <= bound).all(), (hw, np.argwhere(worst > 1)[:8].tolist())


# ---- layouts through Python ------------------------------------------------------------------------------------------------------------------
def _check_python_route(hl, base, view, dname, touched):
    """freeu_hidden_mean + freeu_apply_ (PLAIN, the map, inject) on `view` of `base`: the statement on the device's own fp32 map, the mean
    within its bound, and every channel of `base` not in `touched` bit-identical."""
    before = base.clone()
    x64 = view.float().cpu().numpy().astype(np.float64)
    B, C, H, W = x64.shape
    mean, ext = hl.freeu_hidden_mean(view)
    groups, per = F.groups_run(C, int(hl.load().sonar_freeu_hidden_mean_groups(B, C, H * W)), 16)
    assert (np.abs(mean.cpu().numpy() - F.hidden_mean_ref(x64)[0]) <= F.mean_bound(x64, per, groups)).all()
    assert hl.freeu_apply_(view, 0, C, mode=hl.FREEU_PLAIN, hidden=(mean, ext), scale=SCALE, blend_mode="inject", blend=BLEND) is view
    st, bound = F.apply_abi_ref(x64, 0, C, F.PLAIN, mean=mean.cpu().numpy(), extremes=ext.cpu().numpy(), scale=SCALE, blend_mode=F.INJECT, blend=BLEND,
                                with_bound=True)
    if dname != "float32":
        bound = bound + R.HALF_EPS[dname] * np.abs(st)
    assert (np.abs(view.float().cpu().numpy() - st) <= bound).all()
    rest = [c for c in range(base.shape[1]) if c not in touched]
    assert torch.equal(base[:, rest], before[:, rest])


def test_python_layouts(hl):
    """B = 1 with a channel-strided view (addressed in place, the skipped channels bit-identical) and C = 1, in the three dtypes; an
    expanded tensor and a width slice have no layout, and both entry points refuse them."""
    each_case([(d,) for d in R.DTYPES], lambda d: _python_layout_case(hl, d))
    expanded = torch.zeros(2, 1, 4, 6, device="cuda").expand(2, 3, 4, 6)
    narrow = torch.zeros(2, 3, 4, 6, device="cuda")[..., :4]
    for t in (expanded, narrow):
        assert hl.freeu_layout(t) is None
        with pytest.raises(hl.SonarHipError):
            hl.freeu_hidden_mean(t)
        with pytest.raises(hl.SonarHipError):
            hl.freeu_apply_(t, 0, 1, mode=hl.FREEU_PLAIN, scale=SCALE)


def _python_layout_case(hl, dname):
    base = torch.from_numpy(R.make_input((1, 6, 4, 6), 21)).to(DT[dname]).cuda()
    view = base[:, ::2]
    assert hl.freeu_layout(view) == (3 * 48, 48) and view.data_ptr() == base.data_ptr()
    _check_python_route(hl, base, view, dname, touched=(0, 2, 4))  # addressed in place: channels 1, 3, 5 are skipped
    one = torch.from_numpy(R.make_input((2, 1, 4, 6), 22)).to(DT[dname]).cuda()
    assert hl.freeu_layout(one) == (24, 24)
    _check_python_route(hl, one, one, dname, touched=(0,))
