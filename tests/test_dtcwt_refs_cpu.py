"""CPU: the plain statements of tests/dtcwt_refs.py (what tests/test_gpu_dtcwt_kernel_edges.py holds the kernels of csrc/dtcwt.hip to) against
the stages of oracle/dtcwt_oracle.py, their derived bounds against a float32 / float64 walk of the same arithmetic in numpy, and the tap
tables of py/dtcwt.py at the tiny lengths -- n shorter than the filter, where the half-sample extension folds more than once -- with every
index inside [0, n): a table with an index outside it would make the kernel read out of bounds, so this check stands before any device run."""
import importlib

import numpy as np
import pytest

from oracle import dtcwt_oracle as dto
from tests import dtcwt_refs as R

BANKS = ("near_sym_a", "legall", "antonini")
ODD_N = (1, 2, 3, 4, 5, 6, 7, 8)
DEC_N = (4, 8, 16)
INT_N = (2, 4, 6, 8, 16)


@pytest.fixture(scope="module")
def dt(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.dtcwt")


def dense_table(stage, n):
    """(idx, coef) of a linear stage of the oracle, read off its answer to the unit vectors: every row lists all n inputs"""
    m = stage(np.eye(n))  # [n_out, n]
    return np.broadcast_to(np.arange(n, dtype=np.int32), m.shape).copy(), m


STAGES = [("colfilter h0o", lambda X: dto.colfilter(X, dto.biort("near_sym_a")[0]), ODD_N),
          ("colfilter g1o", lambda X: dto.colfilter(X, dto.biort("antonini")[3]), ODD_N),
          ("coldfilt low", lambda X: dto.coldfilt(X, dto.qshift("qshift_a")[1], dto.qshift("qshift_a")[0]), DEC_N),
          ("coldfilt high", lambda X: dto.coldfilt(X, dto.qshift("qshift_a")[5], dto.qshift("qshift_a")[4]), DEC_N),
          ("colifilt low", lambda X: dto.colifilt(X, dto.qshift("qshift_a")[3], dto.qshift("qshift_a")[2]), INT_N),
          ("colifilt high", lambda X: dto.colifilt(X, dto.qshift("qshift_a")[7], dto.qshift("qshift_a")[6]), INT_N)]


@pytest.mark.parametrize("name,stage,lengths", STAGES, ids=[s[0].replace(" ", "_") for s in STAGES])
def test_axis_taps_statement_is_the_oracle_stage(name, stage, lengths):
    """sum_k coef[j, k] x[idx[j, k]] with the stage's own matrix as the table is the stage, along either axis, with and without a base"""
    rng = np.random.default_rng(11)
    for n in lengths:
        idx, coef = dense_table(stage, n)
        x = rng.standard_normal((2, n, 3))
        want = np.moveaxis(stage(np.moveaxis(x, 1, 0)), 0, 1)
        assert np.abs(R.axis_taps(x, idx, coef, -2) - want).max() < 1e-13, (name, n)
        base = rng.standard_normal(want.shape)
        assert np.abs(R.axis_taps(x, idx, coef, -2, base) - (want + base)).max() < 1e-13, (name, n)
        xt = np.ascontiguousarray(np.moveaxis(x, 1, 2))  # the same columns along the last axis
        assert np.abs(R.axis_taps(xt, idx, coef, -1) - np.moveaxis(want, 1, 2)).max() < 1e-13, (name, n)


def test_axis_taps_statement_refuses_a_bad_table():
    x = np.zeros((4, 3))
    with pytest.raises(ValueError):
        R.axis_taps(x, np.array([[0, 4]]), np.ones((1, 2)), -2)
    with pytest.raises(ValueError):
        R.axis_taps(x, np.array([[0, -1]]), np.ones((1, 2)), -2)
    with pytest.raises(ValueError):
        R.axis_taps(x, np.array([[0, 1]]), np.ones((1, 3)), -2)


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 1), (3, 5), (16, 33)])
def test_q2c_c2q_statements_are_the_oracle_shuffles(hw):
    rng = np.random.default_rng(12)
    h, w = hw
    lh, hh, hl = rng.standard_normal((3, 2, 3, 2 * h, 2 * w))
    got = R.q2c(lh, hh, hl)
    assert got.shape == (2, 3, 6, h, w, 2)
    assert np.abs(got - dto._bands(lh, hh, hl)).max() < 1e-15
    for (o1, o2), plane, back in zip(R.PAIRS, (lh, hh, hl), R.c2q(got)):
        z1, z2 = dto.q2c(plane)
        assert np.abs(got[:, :, o1] - z1).max() < 1e-15 and np.abs(got[:, :, o2] - z2).max() < 1e-15
        assert np.abs(back - dto.c2q(z1, z2)).max() < 1e-15 and np.abs(back - plane).max() < 1e-15
    # placement: one plane alone lights exactly its own pair of orientations
    zero = np.zeros_like(lh)
    for (o1, o2), planes in zip(R.PAIRS, ((lh, zero, zero), (zero, hh, zero), (zero, zero, hl))):
        only = R.q2c(*planes)
        assert all((only[:, :, o] == 0).all() for o in range(6) if o not in (o1, o2)) and (only[:, :, o1] != 0).any() and (only[:, :, o2] != 0).any()


def _walk_axis_taps(x, idx, coef, base, dtype):
    """the kernel's loop in ``dtype``, multiply and add rounded separately (numpy has no fma; the bound covers both)"""
    acc = np.zeros((idx.shape[0], *x.shape[1:]), dtype=dtype)
    for k in range(idx.shape[1]):
        acc = acc + (coef[:, k].reshape(-1, *([1] * (x.ndim - 1))) * x[idx[:, k]]).astype(dtype)
    return acc if base is None else base + acc


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounds_hold_for_the_arithmetic_they_describe(dtype):
    """The derived bounds against the same operations walked in numpy at the kernel's precision: the ratio of error to bound never passes 1.
    (fp64 is measured only where longdouble is wider than double; elsewhere the statement and the walk round alike.)"""
    if dtype is np.float64 and R.U_REF >= R.U["float64"]:
        return
    u = R.U[np.dtype(dtype).name]
    rng = np.random.default_rng(13)
    worst = {"axis_taps": 0.0, "axis_taps+base": 0.0, "q2c": 0.0, "c2q": 0.0, "round trip": 0.0}
    for taps, n_in, n_out in ((1, 1, 2), (3, 7, 14), (10, 64, 32), (64, 64, 64)):
        x = rng.standard_normal((n_in, 5)).astype(dtype)
        idx = rng.integers(0, n_in, (n_out, taps)).astype(np.int32)
        coef = rng.standard_normal((n_out, taps)).astype(dtype)
        base = rng.standard_normal((n_out, 5)).astype(dtype)
        for b, key in ((None, "axis_taps"), (base, "axis_taps+base")):
            r = R.ratio(_walk_axis_taps(x, idx, coef, b, dtype), R.axis_taps(x, idx, coef, 0, b), R.axis_taps_bound(x, idx, coef, 0, b, u))
            worst[key] = max(worst[key], r)
    s = dtype(0.70710678118654752440)
    lh, hh, hl = rng.standard_normal((3, 4, 6, 10)).astype(dtype)
    bands = np.zeros((4, 6, 3, 5, 2), dtype=dtype)
    for (o1, o2), y in zip(R.PAIRS, (lh, hh, hl)):
        a, b, c, d = y[..., 0::2, 0::2], y[..., 0::2, 1::2], y[..., 1::2, 0::2], y[..., 1::2, 1::2]
        bands[:, o1, ..., 0], bands[:, o1, ..., 1], bands[:, o2, ..., 0], bands[:, o2, ..., 1] = (a - d) * s, (b + c) * s, (a + d) * s, (b - c) * s
    assert bands.dtype == dtype
    worst["q2c"] = R.ratio(bands, R.q2c(lh, hh, hl), R.q2c_bound(lh, hh, hl, u))
    back = []
    for o1, o2 in R.PAIRS:
        z1, z2 = bands[:, o1], bands[:, o2]
        y = np.zeros((4, 6, 10), dtype=dtype)
        y[..., 0::2, 0::2], y[..., 0::2, 1::2] = (z1[..., 0] + z2[..., 0]) * s, (z1[..., 1] + z2[..., 1]) * s
        y[..., 1::2, 0::2], y[..., 1::2, 1::2] = (z1[..., 1] - z2[..., 1]) * s, -((z1[..., 0] - z2[..., 0]) * s)
        back.append(y)
    worst["c2q"] = max(R.ratio(g, w, b) for g, w, b in zip(back, R.c2q(bands), R.c2q_bound(bands, u)))
    worst["round trip"] = max(R.ratio(g, w, 2 * b) for g, w, b in zip(back, (lh, hh, hl), R.c2q_bound(R.q2c(lh, hh, hl), u)))
    print(f"{np.dtype(dtype).name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(0 < v <= 1 for v in worst.values()), worst


def test_ratio_counts_what_it_should():
    assert R.ratio(np.array([1.0, 2.0]), np.array([1.0, 2.5]), np.array([0.0, 1.0])) == 0.5
    assert R.ratio(np.array([1.0]), np.array([1.5]), np.array([0.0])) == np.inf  # an error where none is allowed
    assert R.ratio(np.array([np.nan]), np.array([1.0]), np.array([1.0])) == np.inf  # an element the kernel never wrote


def _dense(table, x):
    idx, coef = table
    return np.einsum("jk,jk...->j...", coef, x[idx])


def _inside(table, n, n_out, taps):
    idx, coef = table
    assert idx.dtype == np.int32 and idx.shape == coef.shape == (n_out, taps), (idx.shape, coef.shape)
    assert idx.min() >= 0 and idx.max() < n, (n, int(idx.min()), int(idx.max()))


def test_tap_tables_at_the_tiny_lengths(dt):
    """odd n = 1 .. 8 for the four filters of the three banks, decimate n = 4, 8, 16, interpolate n = 2, 4, 6, 8, 16: the stage of the
    oracle to 1e-13 and every index in [0, n)"""
    rng = np.random.default_rng(14)
    for n in ODD_N:
        x = rng.standard_normal((n, 3))
        for bank in BANKS:
            for mine, ref in zip(dt.biort_filters(bank), dto.biort(bank)):
                table = dt.table_odd(n, mine)
                _inside(table, n, n, len(ref))
                assert np.abs(_dense(table, x) - dto.colfilter(x, ref)).max() < 1e-13, (n, bank)
    h0a, h0b, g0a, g0b, h1a, h1b, g1a, g1b = dto.qshift("qshift_a")
    m0a, m0b, n0a, n0b, m1a, m1b, n1a, n1b = dt.qshift_filters("qshift_a")
    for n in DEC_N:
        x = rng.standard_normal((n, 3))
        for mine, ref in (((m0b, m0a), (h0b, h0a)), ((m1b, m1a), (h1b, h1a))):
            table = dt.table_decimate(n, *mine)
            _inside(table, n, n // 2, 10)
            assert np.abs(_dense(table, x) - dto.coldfilt(x, *ref)).max() < 1e-13, n
    for n in INT_N:
        x = rng.standard_normal((n, 3))
        for mine, ref in (((n0b, n0a), (g0b, g0a)), ((n1b, n1a), (g1b, g1a))):
            table = dt.table_interpolate(n, *mine)
            _inside(table, n, 2 * n, 5)
            assert np.abs(_dense(table, x) - dto.colifilt(x, *ref)).max() < 1e-13, n
    for bad in (0, 2, 6):
        with pytest.raises(ValueError):
            dt.table_decimate(bad + 1, m0b, m0a)
    with pytest.raises(ValueError):
        dt.table_interpolate(3, n0b, n0a)


EDGE_SHAPES = [((1, 1, 1, 1), 1), ((1, 1, 2, 2), 2), ((1, 2, 3, 5), 2), ((1, 1, 4, 4), 3), ((1, 1, 6, 10), 3), ((1, 2, 5, 12), 3), ((1, 1, 2, 64), 3),
               ((1, 1, 8, 8), 4)]


@pytest.mark.parametrize("shape,levels", EDGE_SHAPES)
def test_oracle_reconstructs_at_the_edge_shapes(shape, levels):
    """the reference of the device tests holds at each tiny shape they use (measured: 4e-15 at the worst)"""
    x = np.random.default_rng(15).standard_normal(shape)
    for bank in BANKS:
        yl, yh = dto.forward(x, levels, bank)
        assert len(yh) == levels
        back = dto.inverse(yl, yh, bank)
        assert np.abs(back[..., : shape[2], : shape[3]] - x).max() < 1e-13
