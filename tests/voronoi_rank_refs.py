"""tests/voronoi_refs.py with the modes that read past f4 in the sorted row (tests only): ``f`` / ``inv_f`` / ``diff`` / ``diff2`` with any
index numpy accepts on the last axis (Python's negative indices included), ``median_distance`` (torch.median: the lower middle value,
rank (n - 1) // 2) and ``softmin`` with ``use_sorted`` (the weight of point j multiplies the j-th smallest distance), written from the
reference's definitions (py/noise_generation.py:1606-1704).  The three NotImplementedErrors of the base statement are lifted; everything
else is inherited.  These modes are order statistics of continuous functions, so they raise no ambiguity flag of their own.
``variant`` "upper_median" takes rank n // 2 instead (a negative control: it differs where n is even)."""
from __future__ import annotations

import numpy as np

from tests import voronoi_refs as R


class Octave(R.Octave):
    def call(self, name, result, args, kwargs):
        name = name.strip().lower()
        if name not in (R.RESULT_MODES if result else R.DISTANCE_MODES):
            raise ValueError(f"Bad Voronoi {'result' if result else 'distance'} mode {name}")
        kwargs = {k[1:] if k.startswith("_") and len(k) > 1 else k: v for k, v in kwargs.items()}
        return getattr(self, ("r_" if result else "d_") + name)(*args, **kwargs)

    def r_f(self, _d, *, get_sorted, idx=0, **_):
        idx = int(idx)
        s = get_sorted()
        n = s.shape[-1]
        if not -n <= idx < n:
            raise IndexError(f"index {idx} is out of bounds for dimension 5 with size {n}")
        if self.variant == "swap_f1_f2" and 0 <= idx < 2:
            idx = 1 - idx
        return s[..., idx]

    def r_median_distance(self, *_a, get_sorted, **_k):
        s = get_sorted()
        n = s.shape[-1]
        return s[..., n // 2 if self.variant == "upper_median" else (n - 1) // 2].copy()  # .values of a reduction: no view

    def r_softmin(self, d, *_a, temperature=50.0, use_sorted=None, d_orig, get_sorted, **_k):
        logits = -np.sqrt(self._sq(d_orig)) * self.c(temperature)
        e = np.exp(logits - logits.max(axis=-1, keepdims=True))
        eff = get_sorted() if use_sorted is not None else d
        return (eff * (e / e.sum(axis=-1, keepdims=True))).sum(axis=-1)


class Generator(R.Generator):
    def generate(self):
        """R.Generator.generate with this module's Octave (the base names its own class)."""
        if self.features is None or self.z_max == 0:
            self.reset()
        elif abs(self.z_initial - self.z_curr) > abs(self.z_max):
            if self.z_max_mode == "reset":
                self.reset()
            elif self.z_max_mode == "bounce":
                self.z_increment = -self.z_increment
                self.z_curr += self.z_increment
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


def golden_draws(g, name):
    """``draw(shape)`` over the case's recorded uniforms, in call order."""
    flat, at = g[f"draws_{name}"], [0]

    def draw(shape):
        n = int(np.prod(shape))
        part = flat[at[0]:at[0] + n]
        at[0] += n
        assert part.size == n
        return part.reshape(shape)

    draw.used = lambda: at[0]
    return draw


_statements = {}


def statements(g, name, latent, params, calls, variant=None):
    """Per call of the case: (fp64 statement, ambiguous, fp32 statement); computed once per case and variant, shared and left unchanged."""
    key = (name, variant)
    if key not in _statements:
        g64 = Generator(latent, params, golden_draws(g, name), np.float64, variant)
        g32 = Generator(latent, params, golden_draws(g, name), np.float32, variant)
        rows = []
        for _ in range(calls):
            want, amb = g64.generate()
            got32, _ = g32.generate()
            assert got32.dtype == np.float32
            rows.append((want, amb, got32))
        assert g64.draw.used() == g[f"draws_{name}"].size  # every recorded draw was taken, none twice
        _statements[key] = (rows, g64)
    return _statements[key]
