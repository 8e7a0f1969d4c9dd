"""GPU: the rejection-sampled Distro families (csrc/distro.hip: gamma_draw, poisson_draw, vonmises_draw and the ten families built on
them) against the fp64 statement of their streams, tests/distro_refs.py -- every element whose decisions the statement can call in
fp32, within a bound taken from the statement's own fp32 evaluation; the wide parameter range also against the exact laws; the key's
high words, odd offsets, short fills and their tails.  tests/test_distro_refs_cpu.py holds the statement itself and the grid.

Each comparison prints one line (run with -s): the largest device error, the fp32 statement's error it was bounded by, the share left out."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import distro_refs as R
from tests.test_distro_refs_cpu import (AMBIGUOUS_CAP, EXACT, LKJ, N_LAW, SCALAR, SEED, STREAM, WIDE, WISHART, idx_of, law_ok, lkj_params,
                                        wishart_params)

pytestmark = pytest.mark.gpu

N = (1 << 14) + 3   # 16 blocks of float4 groups and a 3-element tail
OFFSET = 12345      # odd: a group of four does not start on a multiple of 4 of the global index
SENTINEL = -777.25


@pytest.fixture(scope="module")
def hl(pkg):
    return pkg.hip_lib


def _fill(hl, n, params, seed=SEED, stream=STREAM, offset=OFFSET, guard=8):
    """``n`` device values in front of ``guard`` floats preset to a sentinel, which the fill must leave alone."""
    buf = torch.full((n + guard,), SENTINEL, device="cuda")
    if n:
        assert hl.distro_fill((n,), "cuda", seed, stream, offset, out=buf[:n], **params).data_ptr() == buf.data_ptr()
    else:  # an empty tensor has no address to hand over: the C entry point itself, on the guard's
        p = hl.DistroParams(params["family"], 0, 0, 0, params.get("a", 0.0), params.get("b", 0.0), params.get("c", 0.0))
        assert hl.load().sonar_distro_fill_f32(buf.data_ptr(), 0, seed, stream, offset, ctypes.byref(p), None) == 0
    host = buf.cpu().numpy()
    assert np.all(host[n:] == np.float32(SENTINEL)), "wrote past the end"
    return host[:n]


def _scale(family, params):
    """von Mises errors are taken relative to the distribution's scale 1 / sqrt(kappa) where that is below 1."""
    return min(1.0, 1.0 / math.sqrt(params["b"])) if family == "vonmises" else None


def _check(hl, label, family, params, *, n=N, seed=SEED, stream=STREAM, offset=OFFSET, cap=AMBIGUOUS_CAP, scale=None, caches=(None, None)):
    idx = idx_of(n, offset)
    r64 = R.distro_ref(family, params, seed, stream, idx, cache=caches[0])
    r32 = R.distro_ref(family, params, seed, stream, idx, np.float32, cache=caches[1])
    bound, own = R.tolerance(r64, r32, scale)
    got = _fill(hl, n, params, seed, stream, offset)
    ok, worst, left, where = R.compare(got, r64, bound, scale, exact=family == "poisson")
    print(f"\nDISTRO-STREAMS | {label} | device {worst:.3g} | fp32 statement {own:.3g} | bound {bound:.3g} | left out {left:.2g}")
    if cap is not None:
        assert left <= cap, (label, left)
    assert ok, (label, worst, bound, where, got[where], r64.value[where])
    return got


# ------------------------------------------------------------------------------------------------ 3a: element-exact
@pytest.mark.parametrize("name", EXACT)
def test_scalar_families_match_the_statement(hl, name):
    case = SCALAR[name]
    _check(hl, name, case.family, case.params, scale=_scale(case.family, case.params))


@pytest.mark.parametrize("d,eta", LKJ)
def test_lkjcholesky_matches_the_statement(hl, d, eta):
    caches = ({}, {})
    for row in range(d):
        for col in range(d):
            got = _check(hl, f"lkjcholesky-{d}-{eta:g}-({row},{col})", "lkjcholesky", lkj_params(d, eta, row, col), caches=caches)
            if col > row:
                assert np.all(got == 0.0)
            if row == col == 0:
                assert np.all(got == 1.0)


@pytest.mark.parametrize("d,df", WISHART)
def test_wishart_matches_the_statement(hl, d, df):
    caches = ({}, {})
    for row in range(d):
        for col in range(row + 1):
            _check(hl, f"wishart-{d}-{df:g}-({row},{col})", "wishart", wishart_params(d, df, row, col), caches=caches)
    assert np.array_equal(_fill(hl, N, wishart_params(d, df, d - 2, d - 1)), _fill(hl, N, wishart_params(d, df, d - 1, d - 2)))
    _check(hl, f"wishart-{d}-{df:g}-({d - 2},{d - 1})", "wishart", wishart_params(d, df, d - 2, d - 1), caches=caches)


# ------------------------------------------------------------------------------------------------ 3b: the wide range
@pytest.mark.parametrize("name", WIDE)
def test_wide_range_matches_the_statement_and_the_law(hl, name):
    """No cap on the ambiguous share here; the device's own 2^18 values also pass the one-sample test against the exact law."""
    case = SCALAR[name]
    _check(hl, name, case.family, case.params, cap=None, scale=_scale(case.family, case.params))
    dev = _fill(hl, N_LAW, case.params, offset=0)
    assert np.isfinite(dev).all(), (name, int((~np.isfinite(dev)).sum()))
    ok, stat, bound = law_ok(case.law, dev)
    print(f"\nDISTRO-STREAMS | {name} law | statistic {stat:.3g} | bound {bound:.3g}")
    assert ok, (name, stat, bound)


# ------------------------------------------------------------------------------------------------ 3c: keys and geometry
KEYED = ("gamma-0.4", "poisson-30", "vonmises-4")


@pytest.mark.parametrize("name", KEYED)
def test_high_words_of_index_stream_and_seed(hl, name):
    case = SCALAR[name]
    scale = _scale(case.family, case.params)
    for n, offset in ((11, 2**32 - 5), (7, 2**47)):
        _check(hl, f"{name} offset {offset}", case.family, case.params, n=n, offset=offset, cap=None, scale=scale)
    for stream in (1, 2**32 + 7, 2**48 - 1):
        _check(hl, f"{name} stream {stream}", case.family, case.params, n=259, stream=stream, cap=None, scale=scale)
    for seed in (1, 2**63 + 5, 0xFFFFFFFF00000000):
        _check(hl, f"{name} seed {seed:#x}", case.family, case.params, n=259, seed=seed, cap=None, scale=scale)
    a, b = _fill(hl, 259, case.params, stream=7), _fill(hl, 259, case.params, stream=2**32 + 7)
    assert not np.array_equal(a, b)  # the stream's high word is in the key


@pytest.mark.parametrize("name", KEYED)
def test_short_fills_and_their_tails(hl, name):
    case = SCALAR[name]
    long = _fill(hl, N + 64, case.params, offset=0)
    for n in (0, 1, 2, 3, 4, 5, 7):
        if n:
            _check(hl, f"{name} n {n}", case.family, case.params, n=n, cap=None, scale=_scale(case.family, case.params))
        assert np.array_equal(_fill(hl, n, case.params, offset=3), long[3:3 + n])
    assert np.array_equal(_fill(hl, N, case.params, offset=37), long[37:37 + N])  # a fill at offset o is [o, o + n) of the fill at 0, bit for bit


def test_refusals_of_the_key_range(hl):
    p = SCALAR["gamma-0.4"].params
    for kw in (dict(offset=2**48 - 3), dict(stream=2**48)):
        with pytest.raises(hl.SonarHipError):
            _fill(hl, 7, p, **kw)
