"""VoronoiNoiseGenerator stated on the host in numpy (tests only): ``generate``, the mode strings and every built mode, written from the
reference's definition (py/noise_generation.py:1291-1904) by evaluating the expressions the way voronoi_call_mode does -- not by
flattening them as the package does.  Two modes: ``dtype=np.float64`` (the statement) and ``dtype=np.float32`` (the same operations in
the kernel's number format, whose distance to the fp64 statement is the yardstick of the tolerances).  The inputs are the same in both: the
drawn feature points and the scalars (scale, z, amplitude, the modes' arguments) as fp32 values, as the reference's fp32 tensors hold them.

The fp64 mode also returns ``ambiguous`` [B, C, H, W]: the elements whose value is decided by a comparison or an ill-conditioned step
whose fp64 margin is below the fp32 error of its operands, so that a correct fp32 evaluation may land elsewhere:
  * WRAP_TOL: a direction-sensitive distance (``angle*``, or a ``fractal_norm`` transform with ``cos``: not even in d) where a component
    of (g - f + 0.5) % 1 of ANY point lies within WRAP_TOL of 0 or 1 -- d flips between -0.5 and +0.5 there.  The operands g and f are
    below 1 with up to three roundings of relative 2^-24 each, scaled by at most 4 in the cases: 2e-6.  Even metrics see |d| and are
    continuous across the wrap.
  * ACOS_TOL: ``angle`` with the clamped component of any point within ACOS_TOL of +-1 (acos' slope is 1 / sqrt(1 - t^2): above 70 there).
  * RANK_TOL: ``cellid`` where the two smallest distances differ by less than RANK_TOL * max(1, |distance|): the index flips.
f1..f4, inv_f*, diff, diff2, ridge, softmin and the result fractal_norm are continuous in the distances (order statistics of continuous
functions are continuous) and take no flag for rank swaps.
``variant`` switches one deliberate error on (negative controls): "no_wrap", "swap_f1_f2", "true_l1"."""
from __future__ import annotations

import numpy as np

WRAP_TOL = 2e-6
ACOS_TOL = 1e-4
RANK_TOL = 1e-5

DEFAULTS = {"n_points": (32,), "distance_mode": ("euclidean",), "z_initial": 0.0, "z_increment": 1.0, "z_max": 100000, "z_max_mode": "reset",
            "z_range": None, "result_mode": ("f1",), "octaves": 1, "octave_mode": "same_features", "lacunarity": 2.0, "gain": 0.5,
            "initial_amplitude": 1.0, "initial_scale": 1.0}
DISTANCE_MODES = frozenset(("angle_sigmoid", "angle_tanh", "angle", "chebyshev", "euclidean", "fractal_norm", "fuzz", "manhatten", "minkowski",
                            "quadratic", "weight"))
RESULT_MODES = frozenset(("cellid", "diff", "diff2", "f", "f1", "f2", "f3", "f4", "fractal_norm", "fuzz", "inv_f", "inv_f1", "inv_f2", "inv_f3",
                          "inv_f4", "gradient_magnitude", "median_distance", "ridge", "softmin"))
NOT_BUILT = {False: frozenset(), True: frozenset(("median_distance",))}  # by `result`


def f32(v):
    return float(np.float32(v))


def rem1(x):
    """torch.remainder(x, 1)"""
    r = np.fmod(x, x.dtype.type(1))
    return np.where((r != 0) & (r < 0), r + x.dtype.type(1), r)


class Octave:
    """One generate_octave: the expressions evaluated on d [B, C, H, W, N, 3]."""

    def __init__(self, dtype, variant, draw=None):
        self.T, self.variant, self.draw = dtype, variant, draw
        self.amb = None          # [B, C, H, W], fp64 mode
        self.directional = False

    def c(self, v):
        return self.T(np.float32(float(v)))  # a mode argument as the fp32 value the reference's tensors hold

    def flag(self, mask):
        self.amb = mask if self.amb is None else self.amb | mask

    def call(self, name, result, args, kwargs):
        name = name.strip().lower()
        if name not in (RESULT_MODES if result else DISTANCE_MODES):
            raise ValueError(f"Bad Voronoi {'result' if result else 'distance'} mode {name}")
        if name in NOT_BUILT[result]:
            raise NotImplementedError(name)
        kwargs = {k[1:] if k.startswith("_") and len(k) > 1 else k: v for k, v in kwargs.items()}
        return getattr(self, ("r_" if result else "d_") + name)(*args, **kwargs)

    # ---- distance modes
    def _sq(self, d):
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    def d_euclidean(self, d, **_):
        return np.sqrt(self._sq(d))

    def d_manhatten(self, d, **_):  # the reference's manhatten IS its euclidean
        if self.variant == "true_l1":
            return (np.abs(d[..., 0]) + np.abs(d[..., 1])) + np.abs(d[..., 2])
        return np.sqrt(self._sq(d))

    def d_chebyshev(self, d, **_):
        return np.abs(d).max(axis=-1)

    def d_minkowski(self, d, *, p=3.0, **_):
        p = float(p)
        a = np.abs(d) ** self.c(p)
        return ((a[..., 0] + a[..., 1]) + a[..., 2]) ** self.T(np.float32(1 / p))

    def d_quadratic(self, d, **_):
        return self._sq(d)

    def _component(self, d, idx):
        self.directional = True
        return d[..., int(idx)] / np.maximum(np.sqrt(self._sq(d)), self.T(1e-12))

    def d_angle(self, d, *, idx=2, **_):
        t = np.clip(self._component(d, idx), -1, 1)
        self.flag((np.abs(t) > 1 - ACOS_TOL).any(axis=-1))
        return np.arccos(t)

    def d_angle_tanh(self, d, *, idx=2, **_):
        return np.arccos(np.tanh(self._component(d, idx)))

    def d_angle_sigmoid(self, d, *, idx=2, **_):
        one = self.T(1)
        return np.arccos(one / (one + np.exp(-self._component(d, idx))) * self.T(2) - one)

    def d_weight(self, d, *args, name="euclidean", h=1.0, w=1.0, z=0.25, **kwargs):
        weights = np.array([self.c(h), self.c(w), self.c(z)], dtype=self.T)
        return self.call(name, False, (d * weights, *args), kwargs)

    def d_fractal_norm(self, d, *args, name="euclidean", mode="sin", scale=0.1, multiplier=10.0, **kwargs):
        if mode not in ("sin", "cos"):
            raise ValueError("Bad mode parameter for fractal_norm distance mode, must be one of: sin, cos")
        if mode == "cos":
            self.directional = True
        fun = np.sin if mode == "sin" else np.cos
        return self.call(name, False, (d + self.c(scale) * fun(d * self.c(multiplier)), *args), kwargs)

    def _fuzzed(self, result, fuzz):
        """Both fuzz modes: whole-tensor extremes, one drawn tensor of uniforms added in place, utils.normalize_to_scale(dim=(-2, -1)) with
        the extremes as targets.  Every step is continuous in its operands -- the element that attains a group's minimum or maximum lands
        on the clamp's edge from either side, and the selection that follows the distance fuzz is an order statistic of continuous
        functions -- so nothing here is flagged."""
        T = self.T
        rmin, rmax = float(result.min()), float(result.max())
        fz = max(abs(rmin), abs(rmax)) * float(fuzz)
        result += self.draw(result.shape).astype(T) * self.c(fz * 2) - self.c(fz)
        lo, hi = result.min(axis=(-2, -1), keepdims=True), result.max(axis=(-2, -1), keepdims=True)
        out = (result - lo) / ((hi - lo) + self.c(1e-07))
        out = out * T(np.float32(rmax - rmin)) + self.c(rmin)
        return np.clip(out, self.c(rmin), self.c(rmax))

    def d_fuzz(self, *args, name="euclidean", fuzz=0.25, **kwargs):
        return self._fuzzed(self.call(name, False, args, kwargs), fuzz)  # [B, C, H, W, N]: the groups are (W, N)

    # ---- result modes
    def r_f(self, _d, *, get_sorted, idx=0, **_):
        idx = int(idx)
        if not 0 <= idx <= 3:
            raise NotImplementedError("idx")
        s = get_sorted()
        if self.variant == "swap_f1_f2" and idx < 2:
            idx = 1 - idx
        return s[..., idx]

    def r_f1(self, *a, **k):
        return self.r_f(*a, idx=0, **k)

    def r_f2(self, *a, **k):
        return self.r_f(*a, idx=1, **k)

    def r_f3(self, *a, **k):
        return self.r_f(*a, idx=2, **k)

    def r_f4(self, *a, **k):
        return self.r_f(*a, idx=3, **k)

    def r_inv_f(self, *a, eps=1e-06, **k):
        return self.T(1) / (self.r_f(*a, **k) + self.c(eps))

    def r_inv_f1(self, *a, **k):
        return self.r_inv_f(*a, idx=0, **k)

    def r_inv_f2(self, *a, **k):
        return self.r_inv_f(*a, idx=1, **k)

    def r_inv_f3(self, *a, **k):
        return self.r_inv_f(*a, idx=2, **k)

    def r_inv_f4(self, *a, **k):
        return self.r_inv_f(*a, idx=3, **k)

    def r_diff(self, *a, idx1=0, idx2=1, **k):
        v1, v2 = (self.r_f(*a, idx=i, **k) for i in (idx1, idx2))
        return v2 - v1

    def r_diff2(self, *a, idx1=0, idx2=1, **k):
        v1, v2 = (self.r_f(*a, idx=i, **k) for i in (idx1, idx2))
        return (v2 - v1) / (v2 + v1 + self.c(1e-06))

    def r_cellid(self, d, *_a, **_k):
        ids = d.argmin(axis=-1).astype(self.T)
        two = np.partition(d, 1, axis=-1)[..., :2]
        self.flag((two[..., 1] - two[..., 0]) < RANK_TOL * np.maximum(1, np.abs(two[..., 0])))
        return ids / ids.max() + self.T(1)

    def r_ridge(self, *a, name="diff", exp=-10.0, **k):
        return self.T(1) - self.c(exp) * self.call(name, True, a, k)

    def r_softmin(self, d, *_a, temperature=50.0, use_sorted=None, d_orig, **_k):
        if use_sorted is not None:
            raise NotImplementedError("use_sorted")
        logits = -np.sqrt(self._sq(d_orig)) * self.c(temperature)
        e = np.exp(logits - logits.max(axis=-1, keepdims=True))
        return (d * (e / e.sum(axis=-1, keepdims=True))).sum(axis=-1)

    def r_gradient_magnitude(self, *a, name1="f4", name2="f4", pad_mode="replicate", **k):
        if pad_mode != "replicate":
            raise NotImplementedError("pad_mode")
        r1 = self.call(name1, True, a, k)
        p1 = np.pad(r1, [(0, 0)] * (r1.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
        p2 = p1 if name2 == name1 else np.pad(self.call(name2, True, a, k), [(0, 0)] * (r1.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
        dx = p1[..., 1:-1, 2:] - p2[..., 1:-1, :-2]
        dy = p1[..., 2:, 1:-1] - p2[..., :-2, 1:-1]
        return np.sqrt(dx * dx + dy * dy)

    def r_fuzz(self, *a, name="f1", fuzz=0.25, **k):
        return self._fuzzed(self.call(name, True, a, k), fuzz)  # an f term is a view: the sorted distances move with the in-place add

    def r_fractal_norm(self, d, *a, name="diff", mode="sin", scale=0.1, multiplier=10.0, **k):
        if mode not in ("sin", "cos"):
            raise ValueError("Bad mode parameter for fractal_norm result mode, must be one of: sin, cos")
        adj = self.c(scale) * (np.sin if mode == "sin" else np.cos)(d * self.c(multiplier))
        own = np.sort(adj, axis=-1)  # this call's own sorted tensor: what its inner terms do in place stays in here
        return self.call(name, True, (adj, *a), k | {"get_sorted": lambda: own})

    # ---- the two expression levels
    @staticmethod
    def split(expr, scale_key):
        modes = expr.split("+")
        base = 1.0 / len(modes)
        for mode in modes:
            if ":" in mode:
                name, *rest = mode.split(":")
                kwargs = dict(tuple(v.strip() for v in di.split("=", 1)) for di in rest)
                yield name, kwargs, base * float(kwargs.pop(scale_key, 1.0))
            else:
                yield mode, {}, base

    def distance(self, d, expr):
        total = None
        for name, kwargs, scale in self.split(expr, "dscale"):
            cur = self.call(name, False, (d,), kwargs) * self.c(scale)
            total = cur if total is None else total + cur
        return total

    def result(self, d, d_orig, expr):
        """The reference scales and sums the terms IN PLACE (``.mul_``, ``.add_``), and an f term is a view of the one sorted tensor the
        terms of an expression share: a later term that reads the sorted distances sees the earlier f term's scaling, and a sum that
        starts with an f term keeps accumulating into that column.  numpy views behave the same, so the same statements are made."""
        total, cache = None, {}

        def get_sorted():
            if "s" not in cache:
                cache["s"] = np.sort(d, axis=-1)
            return cache["s"]

        base = {"d_orig": d_orig, "get_sorted": get_sorted}
        for name, kwargs, scale in self.split(expr, "rscale"):
            cur = self.call(name, True, (d,), kwargs | base)
            cur *= self.c(scale)
            if total is None:
                total = cur
            else:
                total += cur
        return total.copy()

    def run(self, fp, H, W, z_norm, scale, dmode, rmode):
        T = self.T
        B, C, N, _ = fp.shape
        s = self.c(scale)
        gy = np.arange(H, dtype=T) / T(H)
        gx = np.arange(W, dtype=T) / T(W)
        grid = np.empty((H, W, 3), dtype=T)
        grid[..., 0], grid[..., 1], grid[..., 2] = gy[:, None], gx[None, :], self.c(z_norm)
        grid = rem1(grid * s)[None, None, :, :, None, :]
        pts = rem1(fp.astype(T) * s)[:, :, None, None, :, :]
        pre = rem1(grid - pts + T(0.5))
        d = (grid - pts) if self.variant == "no_wrap" else pre - T(0.5)
        dist = self.distance(d.copy(), dmode)
        if self.directional:
            self.flag(((pre < WRAP_TOL) | (pre > 1 - WRAP_TOL)).any(axis=(-1, -2)))
        out = self.result(dist, d, rmode)
        amb = np.zeros(out.shape, bool) if self.amb is None else self.amb
        return out, amb


class Generator:
    """The generator's state over consecutive calls.  ``draw(shape)``: the next uniforms of the call order (fp32)."""

    def __init__(self, latent, params, draw, dtype=np.float64, variant=None):
        self.__dict__.update(DEFAULTS | params)
        self.B, self.C, self.H, self.W = latent
        self.draw, self.T, self.variant = draw, dtype, variant
        self.n_points = tuple(max(2, v) for v in self.n_points)
        self.features = None

    def reset(self):
        self.z_curr = self.z_initial
        self.features = [self.draw((self.B, self.C, self.n_points[o % len(self.n_points)], 3))
                         for o in range(self.octaves if self.octave_mode == "new_features" else 1)]

    def points(self, octave):
        pts, om, odd = self.features[octave % len(self.features)], self.octave_mode, octave % 2 == 1
        if (om == "same_invert_odd" and odd) or (om == "same_invert_even" and not odd):
            return np.float32(1.0) - pts
        if octave > 0 and om in ("same_roll_chan_up", "same_roll_chan_down"):
            return np.roll(pts, (-1 if om == "same_roll_chan_up" else 1) * (octave % 3), axis=1)
        if octave > 0 and om in ("same_roll_dir_up", "same_roll_dir_down"):
            return np.roll(pts, (-1 if om == "same_roll_dir_up" else 1) * (octave % 3), axis=3)
        return pts

    def generate(self):
        """(out [B, C, H, W] in dtype, ambiguous)"""
        if self.features is None or self.z_max == 0:
            self.reset()
        elif abs(self.z_initial - self.z_curr) > abs(self.z_max):
            if self.z_max_mode == "reset":
                self.reset()
            elif self.z_max_mode == "bounce":
                self.z_increment = -self.z_increment
                self.z_curr += self.z_increment
            # (any other mode: the reference assigns a name nothing reads)
        z_range = self.z_range if self.z_range is not None else max(self.H, self.W)
        z_norm = (self.z_curr % z_range) / z_range
        self.z_curr += self.z_increment
        T = self.T
        out = np.zeros((self.B, self.C, self.H, self.W), T)
        amb = np.zeros(out.shape, bool)
        amplitude, scale, total = self.initial_amplitude, self.initial_scale, 0.0
        for o in range(self.octaves):
            octv = Octave(T, self.variant, self.draw)
            val, a = octv.run(self.points(o), self.H, self.W, z_norm, scale, self.distance_mode[o % len(self.distance_mode)],
                              self.result_mode[o % len(self.result_mode)])
            out = out + val * T(np.float32(amplitude))
            amb |= a
            total += abs(amplitude)
            amplitude *= self.gain
            scale *= self.lacunarity
        return out / T(np.float32(total if total != 0 else 1.0)), amb


def error(got, want, ambiguous):
    """The largest distance over the elements that are not ambiguous."""
    keep = ~ambiguous
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64))[keep].max()) if keep.any() else 0.0


def bound(err32, want):
    """8 x the fp32 statement's own distance to the fp64 statement, floor 1e-6 of the case's output range."""
    return max(8.0 * err32, 1e-6 * float(want.max() - want.min()))
