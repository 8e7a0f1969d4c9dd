"""The rejection-sampled families of csrc/distro.hip restated on the host in numpy, vectorised over the elements (tests only).

The ten families that draw through ``gamma_draw``, ``poisson_draw`` and ``vonmises_draw`` -- beta, dirichlet, fisher_snedecor, gamma,
inverse_gamma, lkjcholesky, poisson, studentt, vonmises, wishart -- as a function of (seed, stream id, global element index), from the
key / counter layout and word conversions of tests/test_distro_cpu.py.  Block and word use is the kernel's:

  gamma slot s, proposal j   block 64 + 64 s + j: words 0, 1 the normal, word 2 the acceptance uniform, word 3 of the accepted block the
                             boost uniform (alpha < 1)
  matrix normal (i, c)       block 8 i + c, words 0, 1 (lkjcholesky, wishart); studentt's normal is block 0
  poisson proposal j         block j, words 0 and 1 (inversion below rate 10: block 0, word 0)
  von Mises proposal j       block j, words 0, 1 and 2

  gamma_ref(seed, stream, idx, slot, alpha)      Gamma(alpha, 1), clamped to FLT_MIN
  poisson_ref(seed, stream, idx, rate)
  vonmises_ref(seed, stream, idx, loc, conc)     wrapped to [-pi, pi)
  distro_ref(family, params, seed, stream, idx)  ``params`` as DistroNoiseGenerator.kernel_params returns them (= hip_lib.distro_fill's)

Each returns ``Draw(value, ambiguous, path)``.  Parameters are rounded to fp32 first, where the kernel receives a float; the arithmetic
after that is ``dtype``: float64 is the statement, float32 evaluates the same formulas with every operation rounded once to fp32 and
every libm function rounded correctly (computed in double, then rounded).  That is not the device's libm; it measures, on the host, what
plain fp32 rounding of this arithmetic costs, and the GPU tests bound the kernel's error by a multiple of it.

``path`` is the trail of decisions as an integer (the accepted proposal, Poisson's k); ``ambiguous`` marks the elements where a decision on
the way was too close to call in fp32: ``t <= 0`` and the acceptance inequality of Marsaglia-Tsang, PTRS's branches, its ``floorf`` and
its slow-path inequality, the inversion's ``u >= cdf``, von Mises' two acceptance tests and the ``floorf`` of its wrap.  Too close: the two sides differ
by less than ``GUARD`` = 64 * 2^-24 times the largest magnitude among the terms of that comparison.  A comparison holds at most about ten
fp32 operations, each within 2 ulp of its largest term on the device's libm; the guard is about three times that sum.  The kernel
takes ``lgamma`` in double (PTRS's right side), so no fp32 ``lgammaf`` error enters and the guard is not widened.  (von Mises' sign, ``u_half(w) - 1/2``, is exact in fp32 and is never ambiguous.)

The finite fallbacks after 64 rejections (gamma: d; poisson: floor(rate); von Mises: the mode) are stated below and are UNTESTED: no
seed reaches them (probability below 1e-25), and none is searched for.
"""
from collections import namedtuple

import numpy as np
from scipy import special

from tests.test_distro_cpu import distro_block

f64 = np.float64
f32 = np.float32
GUARD = 64 * 2.0**-24
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_EPSILON = float(np.finfo(np.float32).eps)
MAX_PROPOSALS = 64
GAMMA_BLOCK0 = 64  # gamma slot s proposes from blocks 64 + 64 s + j
ROW_BLOCKS = 8     # matrix normal (i, c) is block 8 i + c
CODES = dict(beta=5, dirichlet=7, fisher_snedecor=8, gamma=9, inverse_gamma=11, lkjcholesky=14, poisson=18, studentt=21, vonmises=23,
             wishart=25)  # hip_lib.DISTRO_*

Draw = namedtuple("Draw", "value ambiguous path")


# ------------------------------------------------------------------------------------------------ arithmetic in ``ft``
def _fn(fun, ft, *xs):
    """A libm function rounded correctly to ``ft``."""
    with np.errstate(all="ignore"):
        return fun(*(np.asarray(x, dtype=f64) for x in xs)).astype(ft)


def _log(x, ft):
    return _fn(np.log, ft, x)


def _cospi(x, ft):
    return _fn(lambda v: np.cos(np.pi * v), ft, x)


def _sinpi(x, ft):
    return _fn(lambda v: np.sin(np.pi * v), ft, x)


def _u_open(w, ft):
    return (((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(f64) + 0.5) * 2.0**-23).astype(ft)  # exact in fp32


def _u_half(w, ft):
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(f64) * 2.0**-24).astype(ft)  # exact in fp32


def _normal(words, ft):
    """Box-Muller, cosine branch, of words 0 and 1."""
    return np.sqrt(ft(-2.0) * _log(_u_open(words[0], ft), ft)) * _cospi(ft(2.0) * _u_half(words[1], ft), ft)


def _close(diff, *terms):
    """|diff| < GUARD * the largest |term|."""
    big = np.maximum.reduce(np.broadcast_arrays(*(np.abs(np.asarray(t, dtype=f64)) for t in terms)))
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(diff, dtype=f64)) < GUARD * big


def normal_ref(seed, stream, idx, block, dtype=f64):
    return _normal(distro_block(seed, stream, idx, block), dtype)


# ------------------------------------------------------------------------------------------------ the three samplers
def gamma_ref(seed, stream, idx, slot, alpha, dtype=f64, *, block0=None, boost_word=3):
    """Marsaglia-Tsang; alpha < 1 boosted as Gamma(alpha + 1) U^(1 / alpha) in log space.  ``block0`` / ``boost_word`` are the contract's
    (first block of the slot, word 3); a test passes others to show that its comparison sees a wrong allotment."""
    ft = dtype
    idx = np.asarray(idx, dtype=np.uint64).ravel()
    first = GAMMA_BLOCK0 + slot * MAX_PROPOSALS if block0 is None else block0
    alpha = ft(f32(alpha))
    boost = alpha < 1
    a = alpha + ft(1) if boost else alpha
    d = a - ft(1) / ft(3)
    c = ft(1) / np.sqrt(ft(9) * d)
    g, ub = np.full(idx.size, d, dtype=ft), np.full(idx.size, 0.5, dtype=ft)  # the fallback after 64 rejections: untested
    amb, path = np.zeros(idx.size, dtype=bool), np.full(idx.size, MAX_PROPOSALS, dtype=np.int64)
    act = np.arange(idx.size)
    with np.errstate(all="ignore"):
        for j in range(MAX_PROPOSALS):
            if act.size == 0:
                break
            w = distro_block(seed, stream, idx[act], first + j)
            x = _normal(w, ft)
            t = ft(1) + c * x
            amb[act] |= _close(t, 1.0, c * x)
            pos = t > 0
            v = np.where(pos, t * t * t, ft(1))
            lhs = _log(_u_open(w[2], ft), ft)
            hx2, dv, dlv = ft(0.5) * x * x, d * v, d * _log(v, ft)
            rhs = hx2 + d - dv + dlv
            amb[act] |= pos & _close(rhs - lhs, lhs, hx2, d, dv, dlv)
            acc = pos & (lhs < rhs)
            g[act[acc]], ub[act[acc]], path[act[acc]] = dv[acc], _u_open(w[boost_word], ft)[acc], j
            act = act[~acc]
        if boost:
            g = _fn(np.exp, ft, _log(g, ft) + _log(ub, ft) / alpha)
    return Draw(np.maximum(g, ft(FLT_MIN)), amb, path)


def poisson_ref(seed, stream, idx, rate, dtype=f64, *, block0=0):
    """Inversion of one uniform below rate 10, Hoermann's PTRS above.  The CDF sum, PTRS's k = floor(lin + rate + 0.43) and the right side
    of its slow-path inequality are double whatever ``dtype``, as in the kernel; their guards take the fp32 terms alone."""
    ft = dtype
    idx = np.asarray(idx, dtype=np.uint64).ravel()
    rate = ft(f32(rate))
    amb = np.zeros(idx.size, dtype=bool)
    if rate < 10:
        u = _u_half(distro_block(seed, stream, idx, block0)[0], f64)
        pk = cdf = np.exp(-f64(rate))
        k = np.zeros(idx.size, dtype=np.int64)
        for step in range(MAX_PROPOSALS):  # the cap: P(X > 64) < 1e-25 at rate 10
            amb |= (k == step) & _close(u - cdf, u, cdf)
            k += (k == step) & (u >= cdf)
            pk = pk * f64(rate) / (step + 1)
            cdf = cdf + pk
        return Draw(k.astype(ft), amb, k * 128)
    slam, drate = np.sqrt(rate), f64(rate)
    b = ft(0.931) + ft(2.53) * slam
    a = ft(-0.059) + ft(0.02483) * b
    inv_alpha = ft(1.1239) + ft(1.1328) / (b - ft(3.4))
    vr_t = ft(3.6224) / (b - ft(2.0))
    vr = ft(0.9277) - vr_t
    out = np.full(idx.size, np.floor(rate), dtype=ft)  # the fallback after 64 rejections: untested
    path = np.full(idx.size, MAX_PROPOSALS, dtype=np.int64)
    act = np.arange(idx.size)
    with np.errstate(all="ignore"):
        for j in range(MAX_PROPOSALS):
            if act.size == 0:
                break
            w = distro_block(seed, stream, idx[act], block0 + j)
            U, V = _u_open(w[0], ft) - ft(0.5), _u_open(w[1], ft)
            us = ft(0.5) - np.abs(U)
            lin = (ft(2.0) * a / us + b) * U
            arg = lin.astype(f64) + drate + 0.43
            k = np.floor(arg)
            near = _close(arg - np.rint(arg), lin, 0.43)
            wide, wide_near = us >= ft(0.07), _close(us - ft(0.07), 0.5, U)
            fast = wide & (V <= vr)
            near |= wide_near | (wide & _close(V - vr, V, 0.9277, vr_t))
            edge = us < ft(0.013)
            skip = (k < 0) | (edge & (V > us))
            near |= ~fast & (_close(us - ft(0.013), 0.5, U) | (edge & _close(V - us, V, us)))
            terms = (_log(V, ft), _log(inv_alpha, ft), _log(a / (us * us) + b, ft))
            lhs = (terms[0] + terms[1] - terms[2]).astype(f64)
            rhs = -drate + k * np.log(drate) - special.gammaln(k + 1.0)
            slow = ~fast & ~skip
            near |= slow & _close(rhs - lhs, *terms)
            acc = fast | (slow & (lhs <= rhs))
            amb[act] |= near
            out[act[acc]], path[act[acc]] = k[acc].astype(ft), k[acc].astype(np.int64) * 128 + j
            act = act[~acc]
    return Draw(out, amb, path)


def vonmises_rm1(conc):
    """The proposal's r (torch's _proposal_r) less 1, in double as DistroNoiseGenerator.kernel_params computes it."""
    kappa = float(f32(conc))
    tau = 1.0 + np.sqrt(1.0 + 4.0 * kappa * kappa)
    rho = (tau - np.sqrt(2.0 * tau)) / (2.0 * kappa)
    return 1.0 / kappa + kappa - 1.0 if kappa < 1e-5 else (1.0 - rho) ** 2 / (2.0 * rho)


def vonmises_ref(seed, stream, idx, loc, conc, dtype=f64, *, block0=0):
    """Best-Fisher (torch's _rejection_sample), with z = cos(pi u), f = (1 + r z) / (r + z), formed as the kernel forms it from the host's
    rm1 = r - 1 (rounded to fp32 as the kernel receives it), 1 - z = 2 sin^2(pi u / 2) and 1 + z = 2 cos^2(pi u / 2)."""
    ft = dtype
    idx = np.asarray(idx, dtype=np.uint64).ravel()
    loc, conc, rm1 = ft(f32(loc)), ft(f32(conc)), ft(f32(vonmises_rm1(conc)))
    x = np.zeros(idx.size, dtype=ft)  # the fallback after 64 rejections: the mode, untested
    amb, path = np.zeros(idx.size, dtype=bool), np.full(idx.size, MAX_PROPOSALS, dtype=np.int64)
    act = np.arange(idx.size)
    with np.errstate(all="ignore"):
        for j in range(MAX_PROPOSALS):
            if act.size == 0:
                break
            w = distro_block(seed, stream, idx[act], block0 + j)
            h = ft(0.5) * _u_half(w[0], ft)
            sh, ch = _sinpi(h, ft), _cospi(h, ft)
            omz, opz = ft(2) * sh * sh, ft(2) * ch * ch
            omf = rm1 * omz / (rm1 + opz)  # 1 - f
            c = conc * (rm1 + omf)         # conc (r - f)
            u2 = _u_open(w[1], ft)
            t1 = c * (ft(2) - c) - u2
            first = t1 > 0
            lg = _log(c / u2, ft)
            t2 = lg + ft(1) - c
            amb[act] |= _close(t1, 2 * c, c * c, u2) | (~first & _close(t2, lg, 1.0, c))
            acc = first | (t2 >= 0)
            sign = np.where(np.signbit(_u_half(w[2], ft) - ft(0.5)), ft(-1), ft(1))
            x[act[acc]], path[act[acc]] = (sign * (ft(2) * _fn(np.arctan2, ft, np.sqrt(rm1 * omz), np.sqrt((rm1 + ft(2)) * opz))))[acc], j
            act = act[~acc]
        pi, two_pi = ft(np.pi), ft(2 * np.pi)
        t = x + pi + loc
        q = t / two_pi
        amb |= _close(q - np.rint(q), 1.0, q)
        return Draw(t - two_pi * np.floor(q) - pi, amb, path)


# ------------------------------------------------------------------------------------------------ the ten families
def distro_ref(family, params, seed, stream, idx, dtype=f64, cache=None, **mutate):
    """Element values of ``family`` at global indices ``idx``.  ``cache`` (a dict, one per (seed, stream, idx, dtype)) keeps the gamma
    slots and normals between calls that differ only in the selected component.  ``mutate`` reaches the samplers' keywords."""
    ft = dtype
    assert params.get("family", CODES[family]) == CODES[family]
    cache = {} if cache is None else cache
    pa, pb, pc = (ft(f32(params.get(k, 0.0))) for k in "abc")
    row, col, dim = params.get("row", 0), params.get("col", 0), params.get("k", 0)
    ambs, paths = [], []

    def gamma(slot, alpha, **kw):
        key = ("gamma", slot, float(alpha), ft)
        res = gamma_ref(seed, stream, idx, slot, alpha, ft, **kw) if kw or key not in cache else cache[key]
        if not kw:
            cache[key] = res
        ambs.append(res.ambiguous)
        paths.append(res.path)
        return res.value

    def normal(block):
        if ("normal", block, ft) not in cache:
            cache["normal", block, ft] = normal_ref(seed, stream, idx, block, ft)
        return cache["normal", block, ft]

    def done(value):
        path = np.zeros(np.asarray(idx).size, dtype=np.int64)
        for p in paths:
            path = path * (MAX_PROPOSALS + 1) + p
        return Draw(value, np.logical_or.reduce(ambs) if ambs else np.zeros(path.size, dtype=bool), path)

    with np.errstate(all="ignore"):
        if family == "poisson":
            return poisson_ref(seed, stream, idx, params["a"], ft, **mutate)
        if family == "vonmises":
            return vonmises_ref(seed, stream, idx, params["a"], params["b"], ft, **mutate)
        if family == "gamma":
            return done(gamma(0, pa, **mutate) / pb)
        if family == "inverse_gamma":
            return done(pb / gamma(0, pa, **mutate))
        if family == "beta":
            g1, g0 = gamma(0, pa), gamma(1, pb, **mutate)
            return done(g1 / (g1 + g0))
        if family == "fisher_snedecor":
            g1, g2 = gamma(0, ft(0.5) * pa), gamma(1, ft(0.5) * pb, **mutate)
            return done((g1 / pa) / (g2 / pb))
        if family == "studentt":
            chi2 = ft(2.0) * gamma(0, ft(0.5) * pc, **mutate)
            return done(pa + pb * (normal(0) * np.sqrt(pc / chi2)))
        if family == "dirichlet":
            gs = [gamma(i, ft(f32(params["v"][i]))) for i in range(dim)]
            total = gs[0]
            for g in gs[1:]:
                total = total + g
            return done(gs[row] / total)
        if family == "lkjcholesky":  # the onion method: row i >= 1 is sqrt(y_i) times a unit direction, y_i ~ Beta(i - 1/2, eta + (d - 2) / 2 - (i - 1) / 2)
            n = np.asarray(idx).size
            if col > row:
                return done(np.zeros(n, dtype=ft))
            if row == 0:
                return done(np.ones(n, dtype=ft))
            g1 = gamma(0, ft(row) - ft(0.5))
            g0 = gamma(1, pa + ft(0.5) * ft(dim - 2) - ft(0.5) * ft(row - 1))
            y = g1 / (g1 + g0)
            if col == row:
                return done(np.sqrt(np.maximum(ft(1) - y, ft(FLT_MIN))))
            ss = np.zeros(n, dtype=ft)
            for c in range(row):
                ss = ss + normal(row * ROW_BLOCKS + c) ** 2
            return done(np.sqrt(y) * normal(row * ROW_BLOCKS + col) / np.sqrt(ss))
        if family == "wishart":  # Bartlett: entry (row, col) of cov_multiplier * A A^T
            lo, hi = min(row, col), max(row, col)
            s = np.zeros(np.asarray(idx).size, dtype=ft)
            for c in range(lo):
                s = s + normal(lo * ROW_BLOCKS + c) * normal(hi * ROW_BLOCKS + c)
            a_lo = np.maximum(np.sqrt(ft(2.0) * gamma(lo, ft(0.5) * (pa - ft(lo)))), ft(FLT_EPSILON))
            s = s + a_lo * (a_lo if hi == lo else normal(hi * ROW_BLOCKS + lo))
            return done(pb * s)
    raise KeyError(family)


# ------------------------------------------------------------------------------------------------ comparing values with the statement
def errors(got, want, scale=None):
    """|got - want| / (1 + |want|) per element (the fixed-word families' measure), or / ``scale`` where one is given."""
    got, want = np.asarray(got, dtype=f64), np.asarray(want, dtype=f64)
    with np.errstate(invalid="ignore"):
        return np.abs(got - want) / ((1.0 + np.abs(want)) if scale is None else scale)


def tolerance(ref64, ref32, scale=None, factor=8.0, floor=1e-6):
    """``factor`` times the largest error of the statement's fp32 evaluation against its fp64 one over the elements that neither calls
    ambiguous and that took the same decisions, at least ``floor``.  Returns (bound, fp32-statement error)."""
    keep = ~ref64.ambiguous & ~ref32.ambiguous & (ref64.path == ref32.path)
    own = float(errors(ref32.value, ref64.value, scale)[keep].max()) if keep.any() else 0.0
    return max(factor * own, floor), own


def compare(got, ref64, bound, scale=None, exact=False):
    """(ok, largest error over the non-ambiguous elements, share of elements left out, first offending indices)."""
    keep = ~ref64.ambiguous
    err = errors(got, ref64.value, scale)
    bad = keep & ~((err == 0) if exact else (err <= bound))
    worst = float(np.nanmax(np.where(keep, err, 0.0))) if keep.any() else 0.0
    return not bad.any(), worst, float(1.0 - keep.mean()) if keep.size else 0.0, np.flatnonzero(bad)[:4]
