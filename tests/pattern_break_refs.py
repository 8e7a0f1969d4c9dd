"""utils.pattern_break (py/utils.py:575-596) stated on the host in numpy (tests only), in two precisions:

  ``fp32``  every step rounded to fp32, in the reference's order -- the kernel's own number format;
  ``fp64``  the same fp32-exact front half (everything up to the argument ``a`` of erfinv is a chain of correctly rounded fp32 operations plus
            a min, a max and an fmod, which are exact), then everything from erfinv on in fp64.

The front half is chaotic (one ulp in it moves outputs by more than the output range), so it is stated once, bit-exactly; the back half is
smooth, so the distance of the two statements measures what fp32 rounding can do to a correct implementation: the yardstick of the
tolerance.  The scalars (1 + detail_level / 10, sqrt 2, 0.2, eps, the percentage) are the fp32 values the reference's tensors see in both.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pattern_break_cases as cases  # noqa: E402

F = np.float32
EPS = F(1e-7)

_erf = np.vectorize(math.erf, otypes=[np.float64])


def newton_erfinv(a):
    """erfinv by Newton's iteration on math.erf, in fp64 (rounded to the argument's dtype at the end).  The start lies beyond the root
    (1 - erf(z)^2 <= exp(-z^2)), the first step lands before it, and from there the iteration on the concave branch climbs monotonically;
    convergence is quadratic, 60 steps are far more than needed."""
    a64 = np.asarray(a, dtype=np.float64)
    out = np.where(a64 <= -1, -np.inf, np.where(a64 >= 1, np.inf, np.where(np.isnan(a64), np.nan, 0.0)))
    inner = np.abs(a64) < 1
    y = np.abs(a64[inner])
    z = np.sqrt(-np.log1p(-y))
    for _ in range(60):
        z = z - (_erf(z) - y) / (2.0 / math.sqrt(math.pi) * np.exp(-z * z))
    out[inner] = np.copysign(z, a64[inner])
    return out.astype(np.asarray(a).dtype)


try:
    from scipy.special import erfinv as _erfinv
except ImportError:
    _erfinv = newton_erfinv


def remainder11_exact_form(m):
    """fmod(m, 11) for fp32 m >= 0 the way the kernel forms it, mirrored in numpy fp32: q = floor(m / 11), r = fma(-q, 11, m) corrected by
    +-11 where it left [0, 11).  The fused step is exact here (r is a multiple of m's last place, below 22 in magnitude), so evaluating it in
    fp64 and rounding is the same value."""
    m = np.asarray(m, dtype=F)
    q = np.floor(m / F(11))
    r64 = m.astype(np.float64) - q.astype(np.float64) * 11.0
    r = r64.astype(F)
    assert np.array_equal(r.astype(np.float64), r64, equal_nan=True), "the fused remainder step is not exact"
    r = np.where(r < 0, r + F(11), np.where(r >= F(11), r - F(11), r))
    return r.astype(F)


def minmax(x):
    """(lo, hi) ignoring NaN, as the kernels' fminf / fmaxf do."""
    return np.fmin.reduce(x, axis=None), np.fmax.reduce(x, axis=None)


def front(x):
    """(a, lo, hi): the argument of erfinv in fp32, bit for bit the reference's, and the input's extremes."""
    x = np.ascontiguousarray(x, dtype=F)
    lo, hi = minmax(x)
    denom = F(F(hi - lo) + EPS)
    v = ((x - lo) / denom) * F(2) + F(-1)
    v = np.where(np.isnan(v), v, np.clip(v, F(-1), F(1)))
    m = np.abs(v) * F(1000000)
    r = np.fmod(m.astype(np.float64), 11.0).astype(F) / F(11)
    a = F(2) * r - F(1)
    assert a.dtype == F
    return a, lo, hi


def _clip(v, lo, hi):
    return np.where(np.isnan(v), v, np.clip(v, lo, hi))


def _blend(mode, a, b, t):
    if mode == "lerp":
        return a + t * (b - a) if a.dtype == np.float64 else _lerp32(a, b, t)
    if mode == "inject":
        return b * t + a
    if mode == "subtract_b":
        return a - b * t
    raise ValueError(mode)


def _lerp32(a, b, t):
    """torch.lerp on fp32 as ATen's CPU kernel evaluates it: fma(|t| < 0.5 ? t : t - 1, b - a, |t| < 0.5 ? a : b), the fma exact in fp64
    here and rounded once (two fp32 factors multiply exactly in fp64; the sum's double rounding is beyond what the bound resolves)."""
    small = abs(float(t)) < 0.5
    coeff = t if small else F(t - F(1))
    base = a if small else b
    return (np.float64(coeff) * (b - a).astype(np.float64) + base.astype(np.float64)).astype(F)


def pattern_break(x, *, percentage=0.5, detail_level=0.0, restore_scale=True, mode="lerp", dtype=np.float32):
    """The filter on a numpy array in ``dtype`` (np.float32: the fp32 statement; np.float64: the fp64 statement)."""
    T = dtype
    x32 = np.ascontiguousarray(x, dtype=F)
    a, lo, hi = front(x32)
    scale, sqrt2, fifth, p = (T(F(v)) for v in (1 + detail_level / 10, 2**0.5, 0.2, percentage))
    with np.errstate(invalid="ignore", over="ignore"):
        e = _erfinv(a.astype(T))
        assert e.dtype == T
        y = _clip(((scale * e) * sqrt2) * fifth, T(-1), T(1))
        if restore_scale:
            rlo, rhi = minmax(y)
            span = T(np.float64(hi) - np.float64(lo))  # the targets go through .item(): a double's difference, rounded once in fp32
            y = (y - rlo) / ((rhi - rlo) + T(EPS))
            y = _clip(y * span + T(lo), T(lo), T(hi))
        out = _blend(mode, x32.astype(T), y, p)
    assert out.dtype == T
    return out


def out_range(out):
    """The scale an output's error is measured against: its range, or its magnitude where the range is degenerate (a constant tensor, a
    single value)."""
    out = np.asarray(out, dtype=np.float64)
    fin = out[np.isfinite(out)]
    if fin.size == 0:
        return 1.0
    span = float(fin.max() - fin.min())
    return span if span > 0 else float(max(np.abs(fin).max(), np.finfo(np.float32).tiny))


# the margin over the fp32 statement's own measured error (the Voronoi tests' construction): covers an erfinv that differs from the one
# used here by a few ulp
MARGIN = 8.0


def load_goldens():
    g = {}
    for stem in ("pattern_break", *cases.LARGE.values()):
        g.update(np.load(os.path.join(ROOT, "tests", "golden", stem + ".npz"), allow_pickle=False))
    return g


_STATEMENTS = {}


def statements():
    """name -> (reference output, fp32 statement, fp64 statement, output range) and E, computed once and shared (the CPU and the GPU tests)."""
    if not _STATEMENTS:
        g = load_goldens()
        table, worst = {}, 0.0
        for name, inp, p, d, r, m in cases.function_cases():
            kw = dict(percentage=p, detail_level=d, restore_scale=r, mode=m)
            s32 = pattern_break(g[f"in_{inp}"], dtype=np.float32, **kw)
            s64 = pattern_break(g[f"in_{inp}"], dtype=np.float64, **kw)
            scale = out_range(s64)
            worst = max(worst, float(np.abs(s32 - s64).max()) / scale)
            table[name] = (g[f"out_{name}"], s32, s64, scale)
        _STATEMENTS.update(table=table, E=worst, g=g)
    return _STATEMENTS
