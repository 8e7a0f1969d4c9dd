"""-m gpu: the three kernels of csrc/dtcwt.hip (``axis_taps_kernel``, ``dtcwt_q2c_kernel``, ``dtcwt_c2q_kernel``; float and double), each
called ALONE -- through ``hip_lib.axis_taps`` / ``dtcwt_q2c`` / ``dtcwt_c2q`` and through the C entry points, where the output has to be
prefilled -- against the plain statements of tests/dtcwt_refs.py (held to oracle/dtcwt_oracle.py by tests/test_dtcwt_refs_cpu.py), and the
whole transform at the tiny shapes against the oracle.

The bounds are derived (tests/dtcwt_refs.py has the derivations), per element, with u = 2^-24 (fp32) or 2^-53 (fp64):
  axis_taps   (taps + 1) u sum_k |coef[j, k]| |x[idx[j, k]]|: ``taps`` fused multiply-adds, gamma_taps <= (taps + 1) u; with accumulate one
              more rounded sum: + u (|base| + that sum)
  q2c / c2q   3 u (|p| + |q|) / sqrt 2 for an output (p +- q) / sqrt 2: one rounded sum, one rounded product, the rounded constant
  round trip  c2q(q2c(.)) within twice the c2q bound of the exact bands
The inputs are float32 values in both precisions, so one reference serves both and the rounding of the inputs is in no bound; the
reference sums in longdouble and its own error (the same formulas with longdouble's u) is added to what is allowed.  Every test prints its
largest error / bound, and the module prints the largest per kernel and dtype at its end.

The loops: ``grid_for(total, 2 * kBlock)`` launches one 256-lane workgroup per 512 elements, so a launch of more than kBlock = 256 elements
already takes a second trip, and the cap of kMaxGrid = 2048 workgroups binds past kMaxGrid * 2 * kBlock = 1 048 576 elements, where a
third trip begins.  test_grid_stride_loops runs both: just past kMaxGrid * kBlock = 524 288 (one full-width grid's worth) and just past
the cap.

Whole transform: the project's tolerances for it (tests/test_gpu_dtcwt.py): fp64 1e-12 and fp32 2e-5 of max(1, peak), reconstruction at
ten times that; the measured distance of every case is printed so that they can be tightened.

Measured on an MI355X, largest over the cases (error / bound; the bounds hold with room only where several roundings average out):
    axis_taps 0.68 fp32, 0.49 fp64; with accumulate 0.97 / 0.99 (one tap onto a dominant base: a single rounding attains the bound)
    q2c 0.66 / 0.54, c2q 0.66 / 0.54, c2q(q2c) 0.61 / 0.62
    whole transform: forward 3.2e-7 fp32, 5.8e-16 fp64; reconstruction 2.2e-7, 1.5e-15; the inverse alone 2.0e-7, 3.4e-16

No table here holds an index outside [0, n_in), and every refusal is checked to have launched nothing."""
import functools
import importlib
import itertools
import types

import numpy as np
import pytest
import torch

from oracle import dtcwt_oracle as dto
from tests import dtcwt_refs as R

pytestmark = pytest.mark.gpu

K_BLOCK, K_MAX_GRID = 256, 2048  # csrc/common.h
ONE_GRID = K_MAX_GRID * K_BLOCK  # 524 288
GRID_CAP = 2 * ONE_GRID  # grid_for(total, 2 * kBlock) reaches kMaxGrid here
DTYPES = [pytest.param(torch.float32, id="fp32"), pytest.param(torch.float64, id="fp64")]
BANKS = ("near_sym_a", "legall", "antonini")
PAD = 64  # guard elements on either side of a prefilled output
WORST: dict = {}


@pytest.fixture(scope="module")
def api(pkg):
    lib = pkg.hip_lib.load()
    mods = {m: importlib.import_module(f"comfyui_sonar_amd.py.{m}") for m in ("wavelet_functions", "dtcwt")}
    yield types.SimpleNamespace(**mods, hl=pkg.hip_lib, lib=lib)
    for key in sorted(WORST):
        print(f"largest error / bound, {key}: {WORST[key]:.3f}")


def name_of(dtype):
    return "float32" if dtype == torch.float32 else "float64"


def kind_of(dtype):
    return "f32" if dtype == torch.float32 else "f64"


def dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(dtype).cuda().contiguous()  # a copy: the references are read-only


def f32_values(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def guarded(shape, dtype, fill=float("nan")):
    """(whole, view): a contiguous ``shape`` view with PAD guard elements of ``fill`` before and after it"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n].view(shape)


def guards_intact(whole, fill=float("nan")):
    edge = torch.cat((whole[:PAD], whole[-PAD:]))
    return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


def within(got, want, bound1, dtype, key, what):
    """|got - want| <= (u + U_REF) * bound1 at every element (bound1: the bound for u = 1; every bound is linear in u); NaN fails"""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements are not finite (never written?)"
    u = R.U[name_of(dtype)]
    r = R.ratio(got, want, (u + R.U_REF) * bound1)
    tag = f"{key} {name_of(dtype)}"
    WORST[tag] = max(WORST.get(tag, 0.0), r)
    if not r <= 1.0:
        err = np.abs(got.astype(R.WIDE) - want)
        first = tuple(int(i) for i in np.argwhere(~(err <= (u + R.U_REF) * bound1))[0])
        raise AssertionError(f"{what}: error / bound {r:.3g}; first bad element {first}: got {got[first]!r}, want {float(want[first])!r}, "
                             f"allowed {float((u + R.U_REF) * bound1[first]):.3g}")
    return r


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ axis_taps
@functools.lru_cache(maxsize=None)
def taps_case(shape, axis, n_out, taps, seed=0):
    """(x, idx, coef, base, want, want + base, bound1, bound1 with base): random float32 values, indices uniform in [0, n_in) (repeats allowed)"""
    rng = np.random.default_rng([seed, axis + 2, n_out, taps, *shape])
    n_in = shape[axis]
    x = f32_values(rng, shape)
    idx = rng.integers(0, n_in, (n_out, taps)).astype(np.int32)
    assert 0 <= idx.min() and idx.max() < n_in
    coef = f32_values(rng, (n_out, taps))
    out_shape = list(shape)
    out_shape[axis] = n_out
    base = f32_values(rng, out_shape)
    return frozen(x, idx, coef, base, R.axis_taps(x, idx, coef, axis), R.axis_taps(x, idx, coef, axis, base),
                  R.axis_taps_bound(x, idx, coef, axis, None, 1.0), R.axis_taps_bound(x, idx, coef, axis, base, 1.0))


def run_taps(api, case, axis, dtype, what):
    x, idx, coef, base, want, want_b, b1, b1_b = case
    xd, cd, id_ = dev(x, dtype), dev(coef, dtype), torch.from_numpy(idx.copy()).cuda()
    keep = xd.clone()
    whole, out = guarded(want.shape, dtype)
    got = api.hl.axis_taps(xd, id_, cd, axis, out=out, accumulate=False)  # onto NaN: a kernel that read `out` regardless would return NaN
    assert got is out
    r0 = within(got, want, b1, dtype, "axis_taps", what)
    fresh = api.hl.axis_taps(xd, id_, cd, axis)
    assert torch.equal(fresh, got) and fresh.dtype == dtype and fresh.is_contiguous()
    whole_b, acc = guarded(want.shape, dtype)
    acc.copy_(dev(base, dtype))
    got = api.hl.axis_taps(xd, id_, cd, axis, out=acc, accumulate=True)
    assert got is acc
    r1 = within(got, want_b, b1_b, dtype, "axis_taps accumulate", what + " accumulate")
    assert guards_intact(whole) and guards_intact(whole_b), f"{what}: wrote outside its output"
    assert torch.equal(xd, keep), f"{what}: wrote to its input"
    return max(r0, r1)


def taps_shapes(axis, n_in, inner, outer):
    """2-D for outer = 1, 5-D for outer = 5 (and the 2-D [5, n_in] along the last axis)"""
    if axis == -2:
        return [(n_in, inner)] if outer == 1 else [(1, outer, 1, n_in, inner)]
    return [(1, n_in)] if outer == 1 else [(outer, n_in), (1, outer, 1, 1, n_in)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("taps", [1, 3, 10, 64])
@pytest.mark.parametrize("axis", [-2, -1])
def test_axis_taps_alone(api, axis, taps, dtype):
    """random tables: n_in in {1, 2, 7, 64}, n_out = n_in, 2 n_in, n_in // 2, inner in {1, 3, 64, 65} along axis -2 (1 along axis -1: lanes run
    along j), outer 1 (2-D) and 5 (5-D), onto a NaN output and onto a random base"""
    worst, ran = 0.0, 0
    for n_in, inner, outer in itertools.product((1, 2, 7, 64), (1, 3, 64, 65) if axis == -2 else (1,), (1, 5)):
        for n_out in (n_in, 2 * n_in, n_in // 2):
            if n_out < 1:
                continue
            for shape in taps_shapes(axis, n_in, inner, outer):
                what = f"axis_taps {name_of(dtype)} {shape} axis {axis} n_out {n_out} taps {taps}"
                worst = max(worst, run_taps(api, taps_case(shape, axis, n_out, taps), axis, dtype, what))
                ran += 1
    print(f"axis_taps {name_of(dtype)} axis {axis} taps {taps}: {ran} cases, largest error / bound {worst:.3f}")


# (shape, axis): just past one full-width grid's worth (a second trip for certain), and just past the cap on the grid (a third)
LOOP_TAPS = [((3, 352, 512), -2, False), ((1056, 512), -1, False), ((3, 704, 512), -2, True), ((2112, 512), -1, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,axis,past_cap", LOOP_TAPS, ids=[f"{'x'.join(map(str, s))}_axis{a}" for s, a, _ in LOOP_TAPS])
def test_grid_stride_loops_axis_taps(api, shape, axis, past_cap, dtype):
    total = int(np.prod(shape))  # n_out = n_in
    assert ONE_GRID < total < ONE_GRID + GRID_CAP and (total > GRID_CAP) == past_cap
    r = run_taps(api, taps_case(shape, axis, shape[axis], 3), axis, dtype, f"axis_taps {name_of(dtype)} {shape} axis {axis} ({total} elements)")
    print(f"axis_taps {name_of(dtype)} {shape} axis {axis}: {total} elements, error / bound {r:.3f}")


# ------------------------------------------------------------------------------------------------ q2c / c2q
@functools.lru_cache(maxsize=None)
def quad_case(planes, h, w):
    """(lh, hh, hl) [planes, 2h, 2w] of float32 values, their bands, both bounds for u = 1, and what c2q returns for the bands rounded to fp32"""
    rng = np.random.default_rng([7, planes, h, w])
    lh, hh, hl = (f32_values(rng, (planes, 2 * h, 2 * w)) for _ in range(3))
    bands = R.q2c(lh, hh, hl)
    z = f32_values(rng, (planes, 6, h, w, 2))  # bands of their own for c2q alone: float32 values
    return frozen(lh, hh, hl, bands, R.q2c_bound(lh, hh, hl, 1.0), z, *R.c2q(z), *R.c2q_bound(z, 1.0), *R.c2q_bound(bands, 1.0))


def raw_q2c(api, planes3, dtype, P, h, w):
    whole, out = guarded((P, 6, h, w, 2), dtype)
    rc = getattr(api.lib, f"sonar_dtcwt_q2c_{kind_of(dtype)}")(*(p.data_ptr() for p in planes3), out.data_ptr(), P, h, w, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, api.lib.sonar_last_error()
    return whole, out


def raw_c2q(api, bands, dtype, P, h, w):
    outs = [guarded((P, 2 * h, 2 * w), dtype) for _ in range(3)]
    rc = getattr(api.lib, f"sonar_dtcwt_c2q_{kind_of(dtype)}")(bands.data_ptr(), *(o.data_ptr() for _, o in outs), P, h, w, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, api.lib.sonar_last_error()
    return [wh for wh, _ in outs], [o for _, o in outs]


def run_quads(api, P, h, w, dtype, through_wrapper):
    lh, hh, hl, bands, qb1, z, *rest = quad_case(P, h, w)
    back_want, cb1, rb1 = rest[0:3], rest[3:6], rest[6:9]
    what = f"{name_of(dtype)} planes {P} {h} x {w}"
    planes3 = [dev(p, dtype) for p in (lh, hh, hl)]
    whole, got = raw_q2c(api, planes3, dtype, P, h, w)  # every element written: the output was NaN
    rq = within(got, bands, qb1, dtype, "q2c", "q2c " + what)
    assert guards_intact(whole), f"q2c {what}: wrote outside its output"
    zd = dev(z, dtype)
    wholes, outs = raw_c2q(api, zd, dtype, P, h, w)
    rc = max(within(o, wnt, b, dtype, "c2q", "c2q " + what) for o, wnt, b in zip(outs, back_want, cb1))
    assert all(guards_intact(wh) for wh in wholes), f"c2q {what}: wrote outside its outputs"
    # the round trip on the device's own bands: twice the c2q bound of the exact bands
    _, trip = raw_c2q(api, got, dtype, P, h, w)
    rt = max(within(o, src.astype(R.WIDE), 2 * b, dtype, "c2q(q2c)", "c2q(q2c) " + what) for o, src, b in zip(trip, (lh, hh, hl), rb1))
    if through_wrapper:  # the wrappers launch the same kernels on [B, C, ...] tensors: the same bits
        B = 2 if P % 2 == 0 else 1
        shaped = [p.view(B, P // B, 2 * h, 2 * w) for p in planes3]
        via = api.hl.dtcwt_q2c(*shaped)
        assert tuple(via.shape) == (B, P // B, 6, h, w, 2) and torch.equal(via.reshape(got.shape), got)
        for o, mine in zip(api.hl.dtcwt_c2q(zd.view(B, P // B, 6, h, w, 2)), outs):
            assert tuple(o.shape) == (B, P // B, 2 * h, 2 * w) and torch.equal(o.reshape(mine.shape), mine)
    return rq, rc, rt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("planes", [1, 6])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 1), (3, 5), (16, 33)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_q2c_c2q_alone(api, hw, planes, dtype):
    rq, rc, rt = run_quads(api, planes, *hw, dtype, through_wrapper=True)
    print(f"q2c / c2q {name_of(dtype)} planes {planes} {hw}: error / bound q2c {rq:.3f}, c2q {rc:.3f}, round trip {rt:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("planes", [3, 6])
def test_grid_stride_loops_q2c_c2q(api, planes, dtype):
    h = w = 256
    total = planes * 3 * h * w  # one quad per element
    assert total > ONE_GRID and (total > GRID_CAP) == (planes == 6)
    rq, rc, rt = run_quads(api, planes, h, w, dtype, through_wrapper=False)
    print(f"q2c / c2q {name_of(dtype)} planes {planes} {h} x {w}: {total} quads, error / bound q2c {rq:.3f}, c2q {rc:.3f}, round trip {rt:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(1, 1), (3, 5)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_q2c_places_each_plane_in_its_own_pair(api, hw, dtype):
    """with one of lh / hh / hl non-zero the four other orientations are exactly zero (pair p -> orientations p and 5 - p), and c2q of one
    pair of orientations leaves the two other planes exactly zero"""
    h, w = hw
    lh, hh, hl, bands, *_ = quad_case(6, h, w)
    zero = torch.zeros((2, 3, 2 * h, 2 * w), dtype=dtype, device="cuda")
    for p, plane in enumerate((lh, hh, hl)):
        args = [zero, zero.clone(), zero.clone()]
        args[p] = dev(plane, dtype).view(2, 3, 2 * h, 2 * w)
        got = api.hl.dtcwt_q2c(*args)
        lit = [o for o in range(6) if bool((got[:, :, o] != 0).any())]
        assert lit == [p, 5 - p], (p, lit)
        full = api.hl.dtcwt_q2c(*(dev(v, dtype).view(2, 3, 2 * h, 2 * w) for v in (lh, hh, hl)))
        assert torch.equal(got[:, :, p], full[:, :, p]) and torch.equal(got[:, :, 5 - p], full[:, :, 5 - p])
        only = torch.zeros_like(full)
        only[:, :, p], only[:, :, 5 - p] = full[:, :, p], full[:, :, 5 - p]
        back = api.hl.dtcwt_c2q(only)
        assert [bool((b != 0).any()) for b in back] == [q == p for q in range(3)]


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_what_they_cannot_run(api):
    hl, lib = api.hl, api.lib
    st = torch.cuda.current_stream().cuda_stream
    for dtype in (torch.float32, torch.float64):
        k = kind_of(dtype)
        taps_fn, q2c_fn, c2q_fn = (getattr(lib, f"sonar_{n}_{k}") for n in ("axis_taps", "dtcwt_q2c", "dtcwt_c2q"))
        x = torch.full((4 * 65,), 7.0, dtype=dtype, device="cuda")
        out = torch.full((4 * 65,), 5.0, dtype=dtype, device="cuda")
        idx = torch.zeros((4, 65), dtype=torch.int32, device="cuda")
        coef = torch.ones((4, 65), dtype=dtype, device="cuda")
        X, O, I, Cf = x.data_ptr(), out.data_ptr(), idx.data_ptr(), coef.data_ptr()

        def call(x=X, out=O, outer=1, n_in=4, n_out=4, inner=1, idx=I, coef=Cf, taps=3, acc=0):
            return taps_fn(x, out, outer, n_in, n_out, inner, idx, coef, taps, acc, st)

        name = f"sonar_axis_taps_{k}".encode()
        for bad in (dict(x=None), dict(out=None), dict(idx=None), dict(coef=None), dict(out=X), dict(taps=0), dict(taps=65), dict(taps=-1),
                    dict(n_in=0), dict(n_out=0), dict(inner=0), dict(outer=-1)):
            assert call(**bad) == hl.ERR_ARG and name in lib.sonar_last_error(), bad
        for bad in (dict(n_in=1 << 24), dict(n_out=1 << 24), dict(inner=1 << 24)):
            assert call(**bad) == hl.ERR_UNSUPPORTED and name in lib.sonar_last_error() and b"too long" in lib.sonar_last_error(), bad
        assert call(outer=0) == 0 and call(outer=0, acc=1) == 0
        torch.cuda.synchronize()
        assert bool((x == 7.0).all()) and bool((out == 5.0).all())  # nothing was launched
        assert call(taps=64) == 0  # 64 taps are accepted and computed: four rows of 64 ones times 7
        torch.cuda.synchronize()
        assert bool((out[:4] == 7.0 * 64).all()) and bool((out[4:] == 5.0).all())

        planes = [torch.full((2 * 4 * 6,), 7.0, dtype=dtype, device="cuda") for _ in range(3)]
        bands = torch.full((2 * 6 * 2 * 3 * 2,), 5.0, dtype=dtype, device="cuda")
        P3, Bd = [p.data_ptr() for p in planes], bands.data_ptr()
        for fn, nm, order in ((q2c_fn, f"sonar_dtcwt_q2c_{k}", lambda pl, b: (*pl, b)), (c2q_fn, f"sonar_dtcwt_c2q_{k}", lambda pl, b: (b, *pl))):
            for pl, b, P, h, w in (([None, *P3[1:]], Bd, 2, 2, 3), ([P3[0], None, P3[2]], Bd, 2, 2, 3), ([*P3[:2], None], Bd, 2, 2, 3), (P3, None, 2, 2, 3),
                                   (P3, Bd, 2, 1 << 15, 3), (P3, Bd, 2, 2, 1 << 15), (P3, Bd, 2, 0, 3), (P3, Bd, 2, 2, 0), (P3, Bd, -1, 2, 3)):
                assert fn(*order(pl, b), P, h, w, st) == hl.ERR_ARG and nm.encode() in lib.sonar_last_error(), (nm, P, h, w)
            assert fn(*order(P3, Bd), 0, 2, 3, st) == 0  # no planes: nothing to do
        torch.cuda.synchronize()
        assert all(bool((p == 7.0).all()) for p in planes) and bool((bands == 5.0).all())  # nothing was launched


def refused(hl, call, match):
    """a SonarHipError of the wrapper's own (not an entry point's error code: no launch was attempted)"""
    with pytest.raises(hl.SonarHipError, match=match) as e:
        call()
    assert "failed (code" not in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrappers_refuse_before_any_launch(api, dtype):
    hl = api.hl
    other = torch.float64 if dtype == torch.float32 else torch.float32
    x = torch.full((2, 6, 5), 7.0, dtype=dtype, device="cuda")
    idx = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    coef = torch.ones((4, 3), dtype=dtype, device="cuda")
    out = torch.full((2, 4, 5), 5.0, dtype=dtype, device="cuda")
    wide_i, wide_c = torch.zeros((4, 6), dtype=torch.int32, device="cuda"), torch.ones((4, 6), dtype=dtype, device="cuda")
    T = "axis_taps"
    refused(hl, lambda: hl.axis_taps(x.transpose(1, 2), idx, coef, -2, out=out), T)  # not contiguous
    for axis in (0, 1, 2, -3):
        refused(hl, lambda: hl.axis_taps(x, idx, coef, axis, out=out), T)
    refused(hl, lambda: hl.axis_taps(x[0, 0], idx, coef, -1), T)  # 1-D
    refused(hl, lambda: hl.axis_taps(x, idx, coef.to(other), -2, out=out), T)
    refused(hl, lambda: hl.axis_taps(x, idx.long(), coef, -2, out=out), T)
    refused(hl, lambda: hl.axis_taps(x.half(), idx, coef.half(), -2), "float32 or float64")
    refused(hl, lambda: hl.axis_taps(x, idx.cpu(), coef, -2, out=out), "idx")
    refused(hl, lambda: hl.axis_taps(x, idx, coef.cpu(), -2, out=out), "coef")
    refused(hl, lambda: hl.axis_taps(x, wide_i[:, ::2], coef, -2, out=out), "idx")  # [4, 3], strided
    refused(hl, lambda: hl.axis_taps(x, idx, wide_c[:, ::2], -2, out=out), "coef")
    refused(hl, lambda: hl.axis_taps(x, idx.reshape(-1), coef.reshape(-1), -2, out=out), T)  # not 2-D
    refused(hl, lambda: hl.axis_taps(x, idx[None], coef[None], -2, out=out), T)
    refused(hl, lambda: hl.axis_taps(x, idx, wide_c, -2, out=out), T)  # shapes differ: more coefficients than indices
    refused(hl, lambda: hl.axis_taps(x, wide_i, coef, -2, out=out), T)  # ... and fewer: the kernel would read coef past its end
    refused(hl, lambda: hl.axis_taps(x, idx[:3], coef, -2, out=out), T)
    refused(hl, lambda: hl.axis_taps(x, idx, coef, -2, out=out[:, :3]), T)  # output of the wrong shape
    refused(hl, lambda: hl.axis_taps(x, idx, coef, -2, out=torch.zeros((2, 5, 4), dtype=dtype, device="cuda").transpose(1, 2)), T)
    refused(hl, lambda: hl.axis_taps(x, idx, coef, -2, out=out.to(other)), T)
    refused(hl, lambda: hl.axis_taps(x[:, :0], idx, coef, -2), T)  # nothing along the axis
    with pytest.raises(hl.SonarHipError, match="code -1"):  # in place: the entry point's refusal
        hl.axis_taps(x, torch.zeros((6, 3), dtype=torch.int32, device="cuda"), torch.ones((6, 3), dtype=dtype, device="cuda"), -2, out=x)

    Q = "dtcwt_q2c"
    lh, hh, hl_ = (torch.full((1, 2, 4, 6), 7.0, dtype=dtype, device="cuda") for _ in range(3))
    refused(hl, lambda: hl.dtcwt_q2c(lh, hh[..., :2, :], hl_), Q)  # a smaller hh or hl would be read past its end
    refused(hl, lambda: hl.dtcwt_q2c(lh, hh, hl_[..., :4]), Q)
    refused(hl, lambda: hl.dtcwt_q2c(lh, hh[:, :1], hl_), Q)
    refused(hl, lambda: hl.dtcwt_q2c(lh[0], hh[0], hl_[0]), Q)  # not 4-D
    refused(hl, lambda: hl.dtcwt_q2c(lh[None], hh[None], hl_[None]), Q)
    odd = torch.zeros((1, 2, 5, 6), dtype=dtype, device="cuda")
    refused(hl, lambda: hl.dtcwt_q2c(odd, odd, odd), "odd side")
    refused(hl, lambda: hl.dtcwt_q2c(odd.transpose(2, 3).contiguous(), odd.transpose(2, 3).contiguous(), odd.transpose(2, 3).contiguous()), "odd side")
    tr = torch.zeros((1, 2, 6, 4), dtype=dtype, device="cuda").transpose(2, 3)  # [1, 2, 4, 6], strided
    refused(hl, lambda: hl.dtcwt_q2c(tr, hh, hl_), "contiguous")
    refused(hl, lambda: hl.dtcwt_q2c(lh, tr, hl_), "contiguous")
    refused(hl, lambda: hl.dtcwt_q2c(lh, hh, tr), "contiguous")
    refused(hl, lambda: hl.dtcwt_q2c(lh.half(), hh.half(), hl_.half()), "float32 or float64")
    refused(hl, lambda: hl.dtcwt_q2c(lh, hh.to(other), hl_), "expected")
    refused(hl, lambda: hl.dtcwt_q2c(lh, hh, hl_.cpu()), "hl")

    Cq = "dtcwt_c2q"
    for shape in ((1, 2, 6, 3, 2), (1, 2, 5, 2, 3, 2), (1, 2, 6, 2, 3, 3), (1, 1, 2, 6, 2, 3, 2), (6, 2, 3, 2)):
        refused(hl, lambda: hl.dtcwt_c2q(torch.zeros(shape, dtype=dtype, device="cuda")), Cq)
    refused(hl, lambda: hl.dtcwt_c2q(torch.zeros((1, 2, 6, 2, 3, 2), dtype=torch.float16, device="cuda")), "float32 or float64")
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((out == 5.0).all()) and all(bool((p == 7.0).all()) for p in (lh, hh, hl_))  # nothing was launched


# ------------------------------------------------------------------------------------------------ the whole transform at the edge shapes
EDGE_SHAPES = [((1, 1, 1, 1), 1), ((1, 1, 2, 2), 2), ((1, 2, 3, 5), 2), ((1, 1, 4, 4), 3), ((1, 1, 6, 10), 3), ((1, 2, 5, 12), 3), ((1, 1, 2, 64), 3),
               ((1, 1, 8, 8), 4)]
TOL = {torch.float64: 1e-12, torch.float32: 2e-5}


@functools.lru_cache(maxsize=None)
def oracle_case(shape, levels, bank):
    x = f32_values(np.random.default_rng([3, levels, *shape]), shape)
    yl, yh = dto.forward(x, levels, bank)
    return frozen(x, yl, *yh, dto.inverse(yl, yh, bank))


def distance(got, want):
    """max |got - want| / max(1, peak of want): what the project's tolerance for this transform is a bound on"""
    want = np.asarray(want)
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,levels", EDGE_SHAPES, ids=[f"{'x'.join(map(str, s))}_J{j}" for s, j in EDGE_SHAPES])
def test_whole_transform_at_the_edge_shapes(api, shape, levels, dtype):
    tol = TOL[dtype]
    for bank in BANKS:
        x, want_yl, *want_yh, want_back = oracle_case(shape, levels, bank)
        xd = dev(x, dtype)
        w = api.wavelet_functions.Wavelet(level=levels, mode="symmetric", use_dtcwt=True, biort=bank)
        yl, yh = w.forward(xd)
        assert len(yh) == levels and yl.dtype == dtype and all(h.dtype == dtype for h in yh)
        d_fwd = max(distance(yl, want_yl), *(distance(g, wnt) for g, wnt in zip(yh, want_yh)))
        crop = (Ellipsis, slice(0, shape[2]), slice(0, shape[3]))
        d_rec = max(distance(w.inverse(yl, yh)[crop], x), distance(w.inverse(yl, yh, two_step_inverse=True)[crop], x))
        oyl, oyh = dev(want_yl, dtype), tuple(dev(h, dtype) for h in want_yh)  # the inverse alone, from the oracle's coefficients
        d_inv = max(distance(w.inverse(oyl, oyh), want_back), distance(w.inverse(oyl, oyh, two_step_inverse=True), want_back))
        print(f"dtcwt {name_of(dtype)} {shape} J={levels} {bank}: forward {d_fwd:.3e} (tolerance {tol:.0e}), reconstruction {d_rec:.3e}, "
              f"inverse alone {d_inv:.3e} (tolerance {10 * tol:.0e})")
        assert d_fwd <= tol and d_rec <= 10 * tol and d_inv <= 10 * tol, (bank, d_fwd, d_rec, d_inv)
        # the DTCWT object underneath is the same computation
        t = api.dtcwt.DTCWT(level=levels, biort=bank)
        tyl, tyh = t.forward(xd)
        assert torch.equal(tyl, yl) and all(torch.equal(a, b) for a, b in zip(tyh, yh)) and torch.equal(t.inverse((yl, yh)), w.inverse(yl, yh))


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_inputs_give_the_bits_of_their_contiguous_copy(api, dtype):
    rng = np.random.default_rng(21)
    w = api.wavelet_functions.Wavelet(level=3, mode="symmetric", use_dtcwt=True)
    for shape in ((2, 3, 5, 12), (1, 2, 6, 10)):
        x = dev(f32_values(rng, shape), dtype)
        yl, yh = w.forward(x)
        back = w.inverse(yl, yh)
        cl = x.contiguous(memory_format=torch.channels_last)
        assert not cl.is_contiguous() and torch.equal(cl, x)
        big = torch.full((shape[0], shape[1] + 1, shape[2] + 3, shape[3] + 4), float("nan"), dtype=dtype, device="cuda")
        big[:, 1:, 1:-2, 3:-1] = x
        view = big[:, 1:, 1:-2, 3:-1]
        assert not view.is_contiguous()
        for other in (cl, view):
            oyl, oyh = w.forward(other)
            assert torch.equal(oyl, yl) and all(torch.equal(a, b) for a, b in zip(oyh, yh))
        # the inverse: a channels-last low-pass and bands that are views
        syl = yl.contiguous(memory_format=torch.channels_last)
        syh = tuple(torch.stack((h, torch.full_like(h, float("nan"))), dim=-1)[..., 0] for h in yh)
        assert all(not h.is_contiguous() for h in syh)
        assert torch.equal(w.inverse(syl, syh), back)


def test_level_zero_and_inverse_refusals(api):
    x = torch.randn((1, 2, 6, 8), device="cuda")
    w0 = api.wavelet_functions.Wavelet(level=0, mode="symmetric", use_dtcwt=True)
    yl, yh = w0.forward(x)
    assert yl is x and len(yh) == 0
    t = api.dtcwt.DTCWT(level=2)
    yl, yh = t.forward(x)
    for missing in ((None, yh[1]), (yh[0], None), (yh[0], yh[1][:0])):
        with pytest.raises(api.hl.SonarHipError, match="every level"):
            t.inverse((yl, missing))
    for wrong in (yl[..., :-1, :], yl[..., :, 1:], torch.cat((yl, yl), dim=-1)):
        with pytest.raises(api.hl.SonarHipError, match="does not match its bands"):
            t.inverse((wrong, yh))
    with pytest.raises(api.hl.SonarHipError, match="does not match its bands"):  # a finer level's bands of the wrong size
        t.inverse((yl, (yh[0][..., 1:, :, :], yh[1])))
    for bad in (x[0], x.half(), x.cpu()):
        with pytest.raises(api.hl.SonarHipError, match="DTCWT.forward"):
            t.forward(bad)
