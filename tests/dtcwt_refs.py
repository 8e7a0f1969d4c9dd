"""Plain numpy statements of the three kernels of csrc/dtcwt.hip, with the rounding-error bound of each, for tests/test_dtcwt_refs_cpu.py
(held to oracle/dtcwt_oracle.py there) and tests/test_gpu_dtcwt_kernel_edges.py.  Nothing here imports the product.

Inputs are taken as they are stored in the kernel's dtype (fp32 values are exact in fp64), so the rounding of the inputs and of the
coefficient table is not part of any bound.  Sums run in ``WIDE`` = numpy's longdouble (a 64-bit significand on x86-64; plain fp64 elsewhere):
``U_REF`` is its unit roundoff, and every ``*_bound(..., u)`` below, called with ``u = U_REF``, bounds the statement's own error too, so a
test allows ``bound(u of the kernel) + bound(U_REF)`` and stays honest on a machine whose longdouble is no wider than double.

The bounds (u = 2^-24 for fp32, 2^-53 for fp64: the largest relative error of one rounded operation):

axis_taps   acc_k = fma(coef[k], x[idx[k]], acc_{k-1}), acc_{-1} = 0: ``taps`` rounded operations, each result a partial sum of the
            terms t_k = coef[k] x[idx[k]], so |error| <= gamma_taps S with S = sum_k |t_k| and gamma_n = n u / (1 - n u) (Higham,
            "Accuracy and Stability of Numerical Algorithms", 2nd ed., section 3.1).  (taps + 1) u exceeds gamma_taps for every
            taps <= 64 in both dtypes ((taps + 1) / taps >= 65 / 64, 1 / (1 - 64 u) <= 1 + 4e-6), and covers a kernel that multiplies and
            adds separately (taps products + taps - 1 sums, still gamma_taps per term).  With a base the kernel adds once more:
            fl(base + acc) errs by at most u |base + acc| <= u (|base| + S) on top.
q2c / c2q   every output is fl(fl(p +- q) * s_T), s_T the constant 1 / sqrt 2 rounded to the dtype: one rounded sum, one rounded product,
            the rounded constant -> |error| <= ((1 + u)^2 (1 + |delta|) - 1) (|p| + |q|) / sqrt 2 with delta the constant's relative
            error: 0.29 u in fp32 (0.70710677) and 0.62 u in fp64, so the factor is below 2.7 u and ``3 u`` holds with the u^2 terms.
round trip  c2q(q2c(.)): a' = s^2 [(a - d)(1 + e1) + (a + d)(1 + e2)] (1 + e3) with |e_i| <= 3 u as above, so
            |a' - a| <= 3 u (|a - d| + |a + d|) / 2 + 3 u |a| <= 2 * [3 u (|z1| + |z2|) / sqrt 2], z1, z2 the exact bands (a -+ d) / sqrt 2
            (|a| <= (|a - d| + |a + d|) / 2): twice ``c2q_bound`` of the bands, and likewise for b, c, d.
"""
import numpy as np

WIDE = np.longdouble
U_REF = float(np.finfo(WIDE).eps) / 2
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
SQRT_HALF = np.sqrt(WIDE(0.5))
PAIRS = ((0, 5), (1, 4), (2, 3))  # pair p (lh, hh, hl) -> orientations p and 5 - p of 15, 45, 75, 105, 135, 165 degrees


def _terms(x, idx, coef, axis):
    """t[j, k, ...] = coef[j, k] * x[idx[j, k], ...] with ``axis`` of x moved to the front; exact products are not needed: WIDE rounds them"""
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape != np.shape(coef):
        raise ValueError("idx and coef are [n_out, taps] tables of one shape")
    xm = np.moveaxis(np.asarray(x).astype(WIDE), axis, 0)
    if idx.size and (idx.min() < 0 or idx.max() >= xm.shape[0]):
        raise ValueError("an index outside [0, n_in)")
    c = np.asarray(coef).astype(WIDE)
    return c.reshape(c.shape + (1,) * (xm.ndim - 1)) * xm[idx]


def axis_taps(x, idx, coef, axis, base=None):
    """sum_k coef[j, k] * x[..., idx[j, k], ...] along ``axis``, plus ``base`` where given (WIDE)"""
    out = np.moveaxis(_terms(x, idx, coef, axis).sum(axis=1), 0, axis)
    return out if base is None else out + np.asarray(base).astype(WIDE)


def axis_taps_bound(x, idx, coef, axis, base, u):
    """(taps + 1) u sum_k |coef[j, k]| |x[idx[j, k]]|, and u (|base| + that sum) more with a base"""
    taps = np.shape(idx)[1]
    s = np.moveaxis(np.abs(_terms(x, idx, coef, axis)).sum(axis=1), 0, axis)
    bound = (taps + 1) * u * s
    return bound if base is None else bound + u * (np.abs(np.asarray(base).astype(WIDE)) + s)


def _quad(y):
    y = np.asarray(y).astype(WIDE)
    return y[..., 0::2, 0::2], y[..., 0::2, 1::2], y[..., 1::2, 0::2], y[..., 1::2, 1::2]


def q2c(lh, hh, hl):
    """Three [..., 2h, 2w] planes -> [..., 6, h, w, 2]: quad (a b / c d) of pair p -> ((a - d) + i (b + c)) / sqrt 2 at orientation p
    and ((a + d) + i (b - c)) / sqrt 2 at orientation 5 - p"""
    first = np.shape(lh)
    out = np.zeros((*first[:-2], 6, first[-2] // 2, first[-1] // 2, 2), dtype=WIDE)
    for (o1, o2), plane in zip(PAIRS, (lh, hh, hl)):
        a, b, c, d = _quad(plane)
        out[..., o1, :, :, 0], out[..., o1, :, :, 1] = (a - d) * SQRT_HALF, (b + c) * SQRT_HALF
        out[..., o2, :, :, 0], out[..., o2, :, :, 1] = (a + d) * SQRT_HALF, (b - c) * SQRT_HALF
    return out


def q2c_bound(lh, hh, hl, u):
    """3 u (|a| + |d|) / sqrt 2 for both real parts, 3 u (|b| + |c|) / sqrt 2 for both imaginary parts"""
    first = np.shape(lh)
    out = np.zeros((*first[:-2], 6, first[-2] // 2, first[-1] // 2, 2), dtype=WIDE)
    for pair, plane in zip(PAIRS, (lh, hh, hl)):
        a, b, c, d = (np.abs(v) for v in _quad(plane))
        for o in pair:
            out[..., o, :, :, 0], out[..., o, :, :, 1] = 3 * u * (a + d) * SQRT_HALF, 3 * u * (b + c) * SQRT_HALF
    return out


def _c2q(bands, bound_u=None):
    z = np.asarray(bands).astype(WIDE)
    if z.ndim < 4 or z.shape[-4] != 6 or z.shape[-1] != 2:
        raise ValueError("bands are [..., 6, h, w, 2]")
    planes = []
    for o1, o2 in PAIRS:
        z1, z2 = z[..., o1, :, :, :], z[..., o2, :, :, :]
        if bound_u is None:
            p, q = (z1 + z2) * SQRT_HALF, (z1 - z2) * SQRT_HALF  # p = a + i b, q = -d + i c
            parts = (p[..., 0], p[..., 1], q[..., 1], -q[..., 0])
        else:
            m = 3 * bound_u * (np.abs(z1) + np.abs(z2)) * SQRT_HALF
            parts = (m[..., 0], m[..., 1], m[..., 1], m[..., 0])
        y = np.zeros((*z1.shape[:-3], 2 * z1.shape[-3], 2 * z1.shape[-2]), dtype=WIDE)
        y[..., 0::2, 0::2], y[..., 0::2, 1::2], y[..., 1::2, 0::2], y[..., 1::2, 1::2] = parts
        planes.append(y)
    return tuple(planes)


def c2q(bands):
    """[..., 6, h, w, 2] -> (lh, hh, hl), each [..., 2h, 2w]: with z1, z2 the bands at orientations p and 5 - p,
    a + i b = (z1 + z2) / sqrt 2 and -d + i c = (z1 - z2) / sqrt 2"""
    return _c2q(bands)


def c2q_bound(bands, u):
    """3 u (|re z1| + |re z2|) / sqrt 2 for a and d, the same of the imaginary parts for b and c"""
    return _c2q(bands, bound_u=u)


def ratio(got, want, bound):
    """Largest |got - want| / bound over the elements (0 / 0 counts as 0, anything over a zero bound and every NaN as inf)."""
    err = np.abs(np.asarray(got).astype(WIDE) - want)
    bound = np.broadcast_to(np.asarray(bound, dtype=WIDE), err.shape)
    r = np.where(err == 0, WIDE(0), err / np.where(bound > 0, bound, WIDE(1)))
    r = np.where((bound <= 0) & (err != 0), np.inf, r)
    r = np.where(np.isnan(err), np.inf, r)
    return float(r.max()) if r.size else 0.0
