"""The two kernels of csrc/collatz.hip restated on the host in numpy fp32, one operation per line, vectorised over the chains (tests only).

Every array below is float32 and every binary operation takes two float32 operands, so numpy rounds each result once to fp32 -- the
arithmetic the kernels spell with __fmul_rn / __fadd_rn / __fdiv_rn.  Python scalars are rounded to fp32 first (``f32``), the way torch
rounds a Python scalar against an fp32 tensor.

  view(shape, dim, flatten, chain_length)  (outer, len, inner, cl, n_chunks, len_p) of the three-index view
  chain(seeds, ...)                        seeds [outer][n_chunks][inner] -> the kept values, padded layout [outer][len_p][inner]
  mix(acc, out1, second, ...)              acc + (out1 * second) * scale on [outer][len][inner], the padding cropped by indexing
  generate(shape, params, draw)            the generator's loop over iterations with quantile normalisation off
"""
import math

import numpy as np

f32 = np.float32
OUTPUT_MODES = {"values": ("ratios", "seeds"), "ratios": ("ratios", "one"), "mults": ("mults", "one"), "adds": ("adds", "one"),
                "seed_x_ratios": ("ratios", "seeds"), "seed_x_mults": ("mults", "seeds"), "seed_x_adds": ("adds", "seeds"),
                "noise_x_ratios": ("ratios", "mix"), "noise_x_mults": ("mults", "mix"), "noise_x_adds": ("adds", "mix")}
DEFAULTS = dict(adjust_scale=False, iteration_sign_flipping=True, chain_length=(1, 1, 2, 2, 3, 3), iterations=10, rmin=-8000.0, rmax=8000.0,
                flatten=False, dims=(-1, -1, -2, -2), output_mode="values", quantile=0.5, quantile_strategy="clamp", integer_math=True,
                even_multiplier=0.5, even_addition=0.0, odd_multiplier=3.0, odd_addition=1.0, add_preserves_sign=True, chain_offset=5,
                break_loops=True, seed_mode="default")


def view(shape, dim, flatten, chain_length):
    outer = math.prod(shape[:dim])
    length = math.prod(shape[dim:]) if flatten else shape[dim]
    inner = 1 if flatten else math.prod(shape[dim + 1:])
    cl = min(length, chain_length)
    n_chunks = -(-length // cl)
    return outer, length, inner, cl, n_chunks, n_chunks * cl


def rem2(x):
    """torch.remainder(x, 2): fmod, then the divisor's sign."""
    r = np.fmod(x, f32(2.0))
    return np.where((r != 0) & (r < 0), r + f32(2.0), r)


def trunc2(x):
    """utils.trunc_decimals(x, 2)."""
    xi = np.trunc(x)
    xf = x - xi
    return xi + np.trunc(xf * f32(100.0)) * f32(1.0 / 100)


def chain(seeds, cl, chain_offset, *, rmin, rmax, even_multiplier, even_addition, odd_multiplier, odd_addition, integer_math, break_loops,
          add_preserves_sign, seed_mode, output, **_unused):
    """``seeds`` [outer][n_chunks][inner] float32 -> [outer][n_chunks * cl][inner]."""
    assert seeds.dtype == np.float32 and seeds.ndim == 3
    with np.errstate(all="ignore"):
        span = f32(rmax - rmin + 1)
        noise = seeds * span + f32(rmin)
        noise = np.where(noise == 0, noise.max() / f32(noise.size), noise)
        if seed_mode != "default":
            even = rem2(noise) < 1
            noise = np.where(even if seed_mode == "force_odd" else rem2(noise) >= 1, noise + f32(1.0), noise)
        emul, eadd, omul, oadd = f32(even_multiplier), f32(even_addition), f32(odd_multiplier), f32(odd_addition)
        result, muls, adds = noise.copy(), np.ones_like(noise), np.zeros_like(noise)
        kept = []
        for t in range(cl + chain_offset):
            if t > 0:
                prev = result
                reset = np.zeros(noise.shape, dtype=bool)
                if break_loops:
                    pt = trunc2(prev)
                    reset = ((pt >= f32(1.0)) & (pt < f32(1.001))) | (np.abs(pt) < f32(0.001))
                even = rem2(prev) < 1
                m = muls
                if even_multiplier != 1 or odd_multiplier != 1:
                    m = np.where(even, m if even_multiplier == 1 else m * emul, m if odd_multiplier == 1 else m * omul)
                m = np.where(reset, f32(1.0), m)
                a = adds * m
                if even_addition != 0 or odd_addition != 0:
                    sgn = np.sign(prev) if add_preserves_sign else np.ones_like(prev)
                    a = np.where(even, a if even_addition == 0 else a + eadd * sgn, a if odd_addition == 0 else a + oadd * sgn)
                a = np.where(reset, f32(0.0), a)
                r = noise * m + a
                if integer_math:
                    r = np.trunc(r)
                result, muls, adds = np.where(reset, noise, r), m, a
            if t >= chain_offset:
                kept.append(muls if output == "mults" else (adds if output == "adds" else result) / noise)
        out = np.stack(kept, axis=2)  # [outer][n_chunks][cl][inner]
        assert out.dtype == np.float32
        return np.ascontiguousarray(out.reshape(seeds.shape[0], seeds.shape[1] * cl, seeds.shape[2]))


def mix(acc, out1, second, second_mode, length, cl, scale):
    """``acc`` [outer][len][inner] + (out1[:, :len] * second) * scale; ``second`` the seeds [outer][n_chunks][inner] or the mix noise."""
    with np.errstate(all="ignore"):
        v = out1[:, :length]
        if second_mode == "seeds":
            v = np.repeat(second, cl, axis=1)[:, :length] * v
        elif second_mode == "mix":
            v = second.reshape(acc.shape) * v
        return acc + v * f32(scale)


def generate(shape, params, draw, raw=None):
    """The generator with quantile normalisation off.  ``draw(kind, shape)`` hands out the float32 draws in call order: kind "seeds" with
    the chunk shape, kind "mix" with the latent's.  ``raw`` (a list) receives every iteration's kept values, cropped, in the latent's shape."""
    p = DEFAULTS | params
    assert p["quantile"] in (0, 1) and not p["adjust_scale"]
    nd = len(shape)
    dims = tuple(d if d >= 0 else nd + d for d in p["dims"])
    kept, second = OUTPUT_MODES[p["output_mode"]]
    acc = None
    for it in range(p["iterations"]):
        dim, chain_length = dims[it % len(dims)], p["chain_length"][it % len(p["chain_length"])]
        outer, length, inner, cl, n_chunks, len_p = view(shape, dim, p["flatten"], chain_length)
        chunk_shape = (*shape[:dim], n_chunks) if p["flatten"] else (*shape[:dim], n_chunks, *shape[dim + 1:])
        seeds = np.ascontiguousarray(draw("seeds", chunk_shape), dtype=np.float32).reshape(outer, n_chunks, inner)
        out1 = chain(seeds, cl, **(p | dict(output=kept)))
        if raw is not None:
            raw.append(out1[:, :length].reshape(shape).copy())
        other = seeds if second == "seeds" else np.asarray(draw("mix", tuple(shape)), dtype=np.float32) if second == "mix" else None
        scale = (1.0 / p["iterations"]) * (-1 if p["iteration_sign_flipping"] and it & 1 else 1)
        acc = mix(np.zeros((outer, length, inner), np.float32) if acc is None else acc.reshape(outer, length, inner), out1, other, second,
                  length, cl, scale)
    return acc.reshape(shape)
