"""The generate-mode value streams (device draws, ``cpu=False``) restated in numpy: an executable form of INTEGRATION.md 3b.

Every generate-mode value is a pure function of (seed, stream id, global element index).  This module computes those functions on
the host from the stream contract alone -- the same Philox4x32-10 blocks, multiply-with-carry bursts, tile walk and word conversions
the kernels use -- with vectorised ``uint64`` arithmetic and fp64 transcendentals.  No torch, no GPU, and nothing from the product:
tests compare the kernels against it, so a wrong lane, tile, stream word or conversion shows up as an O(1) difference.

``STREAM_VERSION`` is the ``sonar_noise_stream_version()`` this statement describes.  A change to generate-mode values bumps the
library's version and updates this file in the same change (tests/test_gpu_generate_oracle.py checks that the two agree).

The pyramid family (tests/test_gpu_pyramid_oracle.py holds the kernels to it) rests on three rules:
  pyramid_level_grid  the grid the plane kernel draws for a level passed with a NULL pointer: the burst rng_stream(seed, stream_id + 2 +
                      level index in the CALLER's list, tile = global plane elem_offset / (H W) + p, lane = slot); slot t of
                      min(256, ceil(h w / 4)) owns the elements 4t .. 4t + 3, then 4(t + 256) .., one normal4 per group.
  level_normal        the level value of sonar_levels_sampled_f32 / sonar_level_normal_f32 at the global element index
                      e = (plane_offset + p) h w + y w + x: slot e % 4 of philox_normal4(seed, stream, e // 4); level l uses stream_id + l.
  pyramid_planes      normal_fill * sqrt(1 + w0^2) (fp32; 1 without a NULL level of the latent's own size) + sum_l w_l resize(grid_l), the
                      grids drawn as above or supplied.  The resampler is the caller's (tests/pyramid_refs.py: ATen's index rules, fp64 sums).

The Perlin family (tests/test_gpu_perlin_oracle.py holds the kernels to it) rests on three rules:
  perlin_lattice_revolutions  the corner angles, in revolutions: lattice point p = (c (H + 1) + gy)(W + 1) + gx of iteration `it` is u01 of
                      word it % 4 of Philox4x32-10 with counter (p lo, p hi, it // 4, stream id TRUNCATED to 32 bits), key = seed.  The
                      lattice is shared by every latent and every shard: no element offset enters it.
  perlin_lattice      the summed cell-centre terms [C, H, W]: gradient (cos 2 pi u, sin 2 pi u), corner offsets (+-0.5, +-0.5), the blend of
                      common.h at t = 0.5 over the rows first, then the columns, summed over the iterations (none: zeros).
  perlin_values       output index i of a call is u01(stream word of the global element elem_offset + i) / div_fac + sum_t terms[t][i % chw]:
                      the uniform fill's word per element (stream_words), the term tables repeating per latent of the CALL (a shard starts
                      on a latent boundary).  Its float32_steps restates the roundings; perlin_rounding_bound derives the fp32 error bound.
PerlinOldNoiseGenerator takes two stream ids (device_key(2)): the base draw uses `stream`, the lattice `stream + 1`; a shard's elem_offset is
its first latent times C H W.

Kernel sources cited below are under comfyui-sonar_amd/csrc/.
"""
from __future__ import annotations

import math

import numpy as np

STREAM_VERSION = 7

U32 = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
MWC_A = 4294883355

TILE_ITERS = 16                  # common.h kTileIters
TILE_ELEMS = TILE_ITERS * 256    # common.h kTileElems: 16 steps x 64 lanes x 4 slots
BROWN_ITERS = 4                  # noise_brownian.hip kBrownIters
BROWN_TILE = BROWN_ITERS * 256   # noise_brownian.hip kBrownTile
BROWN_STREAM = 0xB0B000000001    # noise_brownian.hip kBrownStream
BROWNIAN_MAX_NODES = 96          # noise_brownian.hip kMaxBrownianNodes


def _u64(v):
    return np.asarray(v, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ Philox4x32 (common.h:43-62)
def philox4x32(c0, c1, c2, c3, k0, k1, rounds: int = 10):
    """Philox4x32 with ``rounds`` rounds (Salmon et al. 2011) on uint64 arrays holding 32-bit words; returns the four output words.
    ``rounds`` = 12 states the power spectrum's edge stream (power_core.h:224-238: a block of ten rounds run for two more)."""
    c0, c1, c2, c3 = (_u64(v) & U32 for v in (c0, c1, c2, c3))
    k0, k1 = _u64(k0) & U32, _u64(k1) & U32
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & U32, p1 >> np.uint64(32), p1 & U32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(_W0)) & U32, (k1 + np.uint64(_W1)) & U32
    return c0, c1, c2, c3


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    return philox4x32(c0, c1, c2, c3, k0, k1, 10)


def philox_group(seed: int, stream, group):
    """common.h philox_group: counter = (group (64 bit), stream id (64 bit)), key = seed."""
    group, stream = _u64(group), _u64(stream)
    seed = int(seed) & (2**64 - 1)
    return philox4x32_10(group & U32, group >> np.uint64(32), stream & U32, stream >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)


# ------------------------------------------------------------------------------------------------ MWC64X bursts (common.h:100-132)
class Mwc:
    """Multiply-with-carry, state (x, c) of 32-bit words in uint64 arrays: out = x ^ c, then x : c = A x + c."""

    def __init__(self, x, c):
        self.x, self.c = _u64(x) & U32, _u64(c) & U32

    @classmethod
    def seeded(cls, a, b):
        """Mwc::seeded: (a, (b >> 1) | 1) -- c in [1, 2^31)."""
        return cls(a, (_u64(b) >> np.uint64(1)) | np.uint64(1))

    def next(self):
        r = self.x ^ self.c
        t = np.uint64(MWC_A) * self.x + self.c  # < 2^64: A < 2^32, x, c < 2^32
        self.x, self.c = t & U32, t >> np.uint64(32)
        return r

    def words(self, count: int):
        """The next ``count`` words, stacked on a new last axis."""
        return np.stack([self.next() for _ in range(count)], axis=-1)


def rng_stream(seed: int, stream: int, tile, lane) -> Mwc:
    """common.h rng_stream: Philox4x32-10 of counter (tile lo, tile hi, stream lo, ((stream >> 32) << 16) ^ lane truncated to 32 bits),
    key = seed; the burst is seeded with (w0 ^ w2, w1 ^ w3).  Bits 48..63 of a stream id do not reach the key."""
    tile, lane = _u64(tile), _u64(lane)
    stream, seed = int(stream) & (2**64 - 1), int(seed) & (2**64 - 1)
    hi = np.uint64((((stream >> 32) << 16) & 0xFFFFFFFF))
    w = philox4x32_10(tile & U32, tile >> np.uint64(32), np.full_like(tile, stream & 0xFFFFFFFF), (hi ^ lane) & U32,
                      seed & 0xFFFFFFFF, seed >> 32)
    return Mwc.seeded(w[0] ^ w[2], w[1] ^ w[3])


# ------------------------------------------------------------------------------------------------ word conversions (common.h:78-94, 134-142)
def u01(w):
    """24-bit uniform in [0, 1) -- exact in fp32 (returned as float64)."""
    return (_u64(w) >> np.uint64(8)).astype(np.float64) * 2.0**-24


def u01_open(w):
    """24-bit uniform plus 2^-25, in (0, 1]: the sum is rounded to fp32 as the kernel rounds it (above 1/2 it is a tie, to even; the
    largest words give 1.0, a zero radius)."""
    return (u01(w).astype(np.float32) + np.float32(2.0**-25)).astype(np.float64)


def box_muller(ra, rb):
    """common.h box_muller in fp64: r = sqrt(-2 ln u01_open(ra)), angle u01(rb) revolutions; returns (r cos, r sin)."""
    r = np.sqrt(-2.0 * np.log(u01_open(ra)))
    a = 2.0 * math.pi * u01(rb)
    return r * np.cos(a), r * np.sin(a)


def unit_mantissa_radius(w):
    """u = 2 - unit_mantissa(w): bits 31..9 of w in the mantissa of a float in [1, 2), so u = 1 - (w >> 9) 2^-23 in (0, 1]."""
    return 1.0 - (_u64(w) >> np.uint64(9)).astype(np.float64) * 2.0**-23


def angle_lo(w):
    """angle_lo: the low 16 bits of w as a fraction of a revolution (the float is 128 + bits 0..22 / 2^16; v_sin / v_cos are periodic)."""
    return (_u64(w) & np.uint64(0xFFFF)).astype(np.float64) * 2.0**-16


def angle_hi(w):
    """angle_hi: the high 16 bits of w as a fraction of a revolution."""
    return (_u64(w) >> np.uint64(16)).astype(np.float64) * 2.0**-16


# ------------------------------------------------------------------------------------------------ the tile walk (common.h kTileIters / kTileElems, noise_stream.h for_each_group)
def tile_position(e):
    """Global element e -> (tile, lane, step, slot): tile e // 4096, lane (e % 256) // 4, burst step (e % 4096) // 256, slot e % 4.
    One step of a lane takes four words, one per slot."""
    e = np.asarray(e, dtype=np.int64)
    return e // TILE_ELEMS, (e % 256) // 4, (e % TILE_ELEMS) // 256, e % 4


def _tile_words(seed: int, stream: int, first: int, last: int):
    """Burst words of tiles first..last: [tiles, 16 steps, 64 lanes, 4 slots] (uint64), in global element order once flattened."""
    tiles = np.arange(first, last + 1, dtype=np.uint64)
    rng = rng_stream(seed, stream, tiles[:, None], np.arange(64, dtype=np.uint64)[None, :])
    w = rng.words(TILE_ITERS * 4)                               # [tiles, lanes, 64]
    return w.reshape(len(tiles), 64, TILE_ITERS, 4).transpose(0, 2, 1, 3)


def _tile_values(seed: int, stream: int, n: int, elem_offset: int, convert):
    """Elements elem_offset .. elem_offset + n - 1 of the flat tile-walked stream; ``convert`` maps [..., 4] words to [..., 4] values."""
    if n == 0:
        return np.zeros(0)
    first, last = elem_offset // TILE_ELEMS, (elem_offset + n - 1) // TILE_ELEMS
    out = np.empty(n, dtype=np.float64)
    chunk = 256  # tiles per pass: bounded host memory for cfg2-sized tensors
    for t0 in range(first, last + 1, chunk):
        t1 = min(last, t0 + chunk - 1)
        vals = convert(_tile_words(seed, stream, t0, t1)).reshape(-1)
        lo, hi = max(elem_offset, t0 * TILE_ELEMS), min(elem_offset + n, (t1 + 1) * TILE_ELEMS)
        out[lo - elem_offset:hi - elem_offset] = vals[lo - t0 * TILE_ELEMS:hi - t0 * TILE_ELEMS]
    return out


def _normal4(w):
    z = np.empty(w.shape, dtype=np.float64)
    z[..., 0], z[..., 1] = box_muller(w[..., 0], w[..., 1])
    z[..., 2], z[..., 3] = box_muller(w[..., 2], w[..., 3])
    return z


def stream_words(seed: int, stream: int, n: int, elem_offset: int = 0):
    """The raw burst word of every element (uint64 holding 32 bits): Perlin's draw and the uniform fill convert one word per value."""
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    first, last = elem_offset // TILE_ELEMS, (elem_offset + n - 1) // TILE_ELEMS
    w = _tile_words(seed, stream, first, last).reshape(-1)
    return w[elem_offset - first * TILE_ELEMS:elem_offset - first * TILE_ELEMS + n]


def normal_fill(seed: int, stream: int, n: int, elem_offset: int = 0):
    """sonar_philox_normal_f32 in fp64: each lane step's four words are two Box-Muller pairs (Mwc::normal4)."""
    return _tile_values(seed, stream, n, elem_offset, _normal4)


def uniform_fill(seed: int, stream: int, n: int, elem_offset: int = 0, sub: float = 0.0, mul: float = 1.0, add: float = 0.0):
    """sonar_philox_uniform_f32: u01 of each word, then (u - sub) * mul + add in fp32 (Affine; skipped when it is the identity).
    Returned as float32; without contraction -- the kernel may fuse the multiply-add (one ulp)."""
    u = _tile_values(seed, stream, n, elem_offset, u01).astype(np.float32)
    if sub == 0.0 and mul == 1.0 and add == 0.0:
        return u
    return (u - np.float32(sub)) * np.float32(mul) + np.float32(add)


def philox_normal4(seed: int, stream: int, group):
    """common.h philox_normal4: the four normals of one Philox block, counter (group, stream), key seed -> [..., 4] fp64."""
    w = philox_group(seed, stream, group)
    return _normal4(np.stack(w, axis=-1))


# ------------------------------------------------------------------------------------------------ Perlin (noise_stream.h perlin_lattice_cells; noise_perlin.hip perlin_generate_kernel, perlin_fast_tiles; common.h Divider)
PERLIN_BLENDS = ("lerp", "inject", "subtract_b")  # common.h blend, SONAR_BLEND_* 0 / 1 / 2


def perlin_lattice_revolutions(seed: int, stream: int, iters: int, C: int, H: int, W: int):
    """The corner angles of perlin_lattice_cells as fractions of a revolution, [iters, C, H + 1, W + 1] fp64 (exact 24-bit values).  Lattice
    point p = (c (H + 1) + gy)(W + 1) + gx of iteration ``it`` is u01(word it % 4) of Philox4x32-10 with counter (p lo, p hi, it // 4, stream)
    and key ``seed``.  Only the low 32 bits of the stream id reach the counter (its fourth word): the streams s and s + 2^32 give one
    lattice.  That is what the kernel does; the tile-keyed draws (rng_stream) use 48 bits."""
    seed, stream = int(seed) & (2**64 - 1), int(stream) & 0xFFFFFFFF
    pts = int(C) * (int(H) + 1) * (int(W) + 1)
    p = np.arange(pts, dtype=np.uint64)
    out = np.zeros((int(iters), pts), dtype=np.float64)
    for g in range(0, int(iters), 4):
        w = philox4x32_10(p & U32, p >> np.uint64(32), np.full_like(p, g >> 2), np.full_like(p, stream), seed & 0xFFFFFFFF, seed >> 32)
        for k in range(min(4, int(iters) - g)):
            out[g + k] = u01(w[k])
    return out.reshape(int(iters), int(C), int(H) + 1, int(W) + 1)


def perlin_blend(mode: str, a, b, t: float = 0.5):
    """common.h blend in fp64: lerp a + t (b - a), inject b t + a, subtract_b a - b t."""
    if mode == "lerp":
        return a + t * (b - a)
    if mode == "inject":
        return b * t + a
    if mode == "subtract_b":
        return a - b * t
    raise KeyError(mode)


def perlin_cell_terms(revolutions, blend_mode: str):
    """Cell-centre terms [..., H, W] of corner angles [..., H + 1, W + 1] in revolutions: gradient (cos, sin) of 2 pi u, dot products with the
    offsets TL (0.5, 0.5), TR (-0.5, 0.5), BL (0.5, -0.5), BR (-0.5, -0.5), blended at t = 0.5 over the rows (TL-TR, BL-BR), then the columns."""
    a = 2.0 * math.pi * np.asarray(revolutions, dtype=np.float64)
    gx, gy = np.cos(a), np.sin(a)
    tl = gx[..., :-1, :-1] * 0.5 + gy[..., :-1, :-1] * 0.5
    tr = gx[..., :-1, 1:] * -0.5 + gy[..., :-1, 1:] * 0.5
    bl = gx[..., 1:, :-1] * 0.5 + gy[..., 1:, :-1] * -0.5
    br = gx[..., 1:, 1:] * -0.5 + gy[..., 1:, 1:] * -0.5
    return perlin_blend(blend_mode, perlin_blend(blend_mode, tl, tr), perlin_blend(blend_mode, bl, br))


def perlin_lattice(seed: int, stream: int, iters: int, C: int, H: int, W: int, blend_mode: str):
    """sonar_perlin_lattice_f32 in fp64: the sum over the iterations of the cell-centre terms, [C, H, W]; no iterations give zeros."""
    if int(iters) <= 0:
        return np.zeros((int(C), int(H), int(W)), dtype=np.float64)
    return perlin_cell_terms(perlin_lattice_revolutions(seed, stream, iters, C, H, W), blend_mode).sum(axis=0)


def divisor_is_power_of_two(div_fac) -> bool:
    """common.h Divider: frexpf(d) == +-0.5 -- the divisor's fp32 value is a power of two of either sign (x / d is then x * (1 / d), exact)."""
    m, _ = math.frexp(float(np.float32(div_fac)))
    return abs(m) == 0.5


def _perlin_parts(seed, stream, terms, chw, div_fac, n, elem_offset, first, count):
    chw, n = int(chw), int(n)
    count = n - int(first) if count is None else int(count)
    assert 0 <= first and first + count <= n
    t = np.zeros((0, chw)) if terms is None else np.asarray(terms)
    t = np.zeros((0, chw)) if t.size == 0 else t.reshape(1, -1) if t.ndim == 1 else t.reshape(t.shape[0], -1)
    assert t.shape[1] == chw, "a term table is one latent"
    u = _tile_values(seed, stream, count, int(elem_offset) + int(first), u01)  # (u01 of stream_words, tile chunks at a time)
    pos = (np.arange(int(first), int(first) + count, dtype=np.int64)) % chw
    return u, t, pos


def perlin_values(seed: int, stream: int, terms, chw: int, div_fac: float, n: int, elem_offset: int = 0, first: int = 0, count=None):
    """sonar_perlin_generate_f32's values for the output indices first .. first + count - 1 (default: all) of a call of ``n`` elements whose
    first element is the global element ``elem_offset``: u01(stream word of elem_offset + i) / div_fac + sum_t terms[t][i % chw], with
    ``terms`` [iters, chw] or [chw] (iters = 0: no table) and ``div_fac`` rounded to fp32 as the C ABI takes it.  Returns
    (values fp64, float32_steps): float32_steps(fused=False) is the same sequence rounded as the kernels round it, in np.float32 --
      power-of-two divisor: u / d is exact; the general route adds the tables in order, one rounding each; the fast route (one table) forms
        the exact u / d + term and rounds once (``fused``: the same bits, u / d being exact);
      any other divisor: fl(u / d), then the adds in table order, one rounding each -- with the division correctly rounded."""
    u, t, pos = _perlin_parts(seed, stream, terms, chw, div_fac, n, elem_offset, first, count)
    d32 = np.float32(div_fac)
    d = float(d32)
    value = u / d
    for row in t:
        value = value + row.astype(np.float64)[pos]

    def float32_steps(fused: bool = False):
        if fused and divisor_is_power_of_two(d32) and t.shape[0] == 1:
            return (u / d + t[0].astype(np.float32).astype(np.float64)[pos]).astype(np.float32)  # exact in fp64 (24 + 24 bits), one rounding
        v = u.astype(np.float32) / d32  # (numpy divides correctly rounded; exact for a power of two)
        for row in t:
            v = v + row.astype(np.float32)[pos]
        return v

    return value, float32_steps


def perlin_rounding_bound(seed: int, stream: int, terms, chw: int, div_fac: float, n: int, elem_offset: int = 0, first: int = 0, count=None):
    """Per value, the bound on |fp32 kernel - fp64 value| of perlin_values: (1 + 0.5 max(iters, 1)) spacing32(M), M the largest of |u / d|
    and the running partial sums -- one ulp for the division, correctly rounded or not, and half an ulp per add."""
    u, t, pos = _perlin_parts(seed, stream, terms, chw, div_fac, n, elem_offset, first, count)
    run = u / float(np.float32(div_fac))
    mag = np.abs(run)
    for row in t:
        run = run + row.astype(np.float64)[pos]
        mag = np.maximum(mag, np.abs(run))
    return (1.0 + 0.5 * max(t.shape[0], 1)) * np.spacing(mag.astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ pyramid streams (noise_pyramid.hip: pyramid_plane_body, fill_levels, level_normal)
PYRAMID_SLOTS = 256        # common.h kBlock: generator slots of one drawn level grid
PYRAMID_MAX_LEVELS = 12    # noise_pyramid.hip kMaxLevels


def pyramid_level_grid(seed: int, stream_id: int, level_index: int, plane: int, h: int, w: int):
    """The [h, w] grid the plane kernel draws for the level at ``level_index`` of the CALLER's list (a level passed with a NULL pointer; a
    full-resolution level folded into the base draw still takes its index) and the global plane ``plane`` = elem_offset / (H W) + p.
    Slot t of min(256, ceil(h w / 4)) runs the burst rng_stream(seed, stream_id + 2 + level_index, tile = plane, lane = t) and owns the
    elements 4t .. 4t + 3, then 4(t + 256) .., one normal4 (four words, two Box-Muller pairs) per group; a cut last group drops its tail."""
    n = int(h) * int(w)
    slots = min(PYRAMID_SLOTS, -(-n // 4))
    rounds = -(-n // (4 * PYRAMID_SLOTS))
    stream = (int(stream_id) + 2 + int(level_index)) & (2**64 - 1)
    rng = rng_stream(seed, stream, np.full(slots, int(plane), dtype=np.uint64), np.arange(slots, dtype=np.uint64))
    z = _normal4(rng.words(4 * rounds).reshape(slots, rounds, 4))     # [slot, round, 4]: element 4 slot + 1024 round + k
    return z.transpose(1, 0, 2).reshape(-1)[:n].reshape(int(h), int(w))


def level_normal(seed: int, stream: int, e):
    """noise_pyramid.hip level_normal: the level value at the global element index e = (plane_offset + p) h w + y w + x is slot e % 4 of
    philox_normal4(seed, stream, e // 4).  Level l of a sonar_levels_sampled_f32 call uses the stream id stream_id + l."""
    e = np.asarray(e, dtype=np.int64)
    z = philox_normal4(seed, int(stream) & (2**64 - 1), (e // 4).astype(np.uint64))
    return np.take_along_axis(z, (e % 4)[..., None], axis=-1)[..., 0]


def pyramid_base_scale(levels, H: int, W: int) -> float:
    """fill_levels: sqrt(1 + w0^2) in fp32 when a level (grid None) of the latent's own size is present -- it is folded into the base draw,
    the sum of two independent normals drawn as one -- else 1."""
    for grid, h, w, wt in levels:
        if grid is None and (h, w) == (H, W):
            w0 = np.float32(wt)
            return float(np.sqrt(np.float32(1.0) + w0 * w0, dtype=np.float32))
    return 1.0


def pyramid_planes(seed: int, stream_id: int, planes: int, H: int, W: int, levels, mode: str, elem_offset: int, resize, magnitude: bool = False):
    """sonar_pyramid_generate_f32 in fp64, [planes, H, W]: normal_fill(seed, stream_id, planes H W, elem_offset) * base_scale
    + sum_l w_l resize(grid_l), with ``levels`` = [(grid or None, h, w, weight), ...] as the caller lists them: a supplied grid is a
    [planes, h, w] array, None at the latent's own size is the folded level (pyramid_base_scale), None at any other size is drawn
    (pyramid_level_grid with the level's index in this list and the global plane elem_offset / (H W) + p: whole planes only).
    ``resize(grids [planes, h, w], H, W, mode)`` -> [planes, H, W] is the caller's fp64 resampler; weights are rounded to fp32 as the C ABI
    takes them.  ``magnitude``: also the per-value scale base_scale |z| + sum_l |w_l| max |grid_l| that fp32 rounding errors are relative to."""
    n = planes * H * W
    base = pyramid_base_scale(levels, H, W)
    out = normal_fill(seed, stream_id, n, elem_offset).reshape(planes, H, W) * base
    mag = np.abs(out)
    folded = False
    for l, (grid, h, w, wt) in enumerate(levels):
        if grid is None and (h, w) == (H, W) and not folded:
            folded = True
            continue
        if grid is None:
            assert elem_offset % (H * W) == 0, "drawn level grids are keyed by whole global planes"
            grid = np.stack([pyramid_level_grid(seed, stream_id, l, elem_offset // (H * W) + p, h, w) for p in range(planes)])
        grid = np.asarray(grid, dtype=np.float64).reshape(planes, h, w)
        wt = float(np.float32(wt))
        out = out + wt * resize(grid, H, W, mode)
        mag = mag + abs(wt) * np.abs(grid).max()
    return (out, mag) if magnitude else out


# ------------------------------------------------------------------------------------------------ Brownian z(node, e) (noise_brownian.hip: brownian_burst_kernel, brownian_burst_add, brownian_kernel, brownian_launch)
def splitmix64(v) -> int:
    """splitmix64 finaliser of v (brownian_launch: the node id's (hx, hc) = low / high word)."""
    h = (int(v) + 0x9E3779B97F4A7C15) & (2**64 - 1)
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return h ^ (h >> 31)


def fmix32(h):
    """MurmurHash3's 32-bit finaliser on uint64 arrays holding 32-bit words."""
    h = _u64(h) & U32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & U32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & U32
    h ^= h >> np.uint64(16)
    return h


def brownian_burst_z(seed: int, nodes, n: int, elem_offset: int = 0):
    """Burst family, z[k, e] for the global elements elem_offset .. + n - 1 (multiples of 1024 in the kernel's use).  A sub-tile of
    1024 elements (4 steps x 64 lanes x 4 slots) has one base state per lane, rng_stream(seed, kBrownStream, e // 1024, lane); node k's
    burst is Mwc::seeded(fmix32(x ^ hx), fmix32(c ^ hc)) with (hx, hc) = splitmix64(node) and (x, c) the base state.  Per step 3 words
    (ra, rb, t): radii sqrt(-2 ln u) of u = 2 - unit_mantissa(ra / rb), angles angle_lo(t) (slots 0, 1) and angle_hi(t) (slots 2, 3)."""
    nodes = [int(v) for v in nodes]
    e = np.arange(elem_offset, elem_offset + n, dtype=np.int64)
    sub = e // BROWN_TILE
    lane, step, slot = (e % 256) // 4, (e % BROWN_TILE) // 256, e % 4
    subs = np.unique(sub)
    base = rng_stream(seed, BROWN_STREAM, subs.astype(np.uint64)[:, None], np.arange(64, dtype=np.uint64)[None, :])
    si = np.searchsorted(subs, sub)
    z = np.empty((len(nodes), n), dtype=np.float64)
    for k, node in enumerate(nodes):
        h = splitmix64(node)
        rng = Mwc.seeded(fmix32(base.x ^ np.uint64(h & 0xFFFFFFFF)), fmix32(base.c ^ np.uint64(h >> 32)))
        w = rng.words(3 * BROWN_ITERS).reshape(len(subs), 64, BROWN_ITERS, 3)[si, lane, step]  # [n, 3]
        ra_rb = np.where(slot < 2, w[:, 0], w[:, 1])
        r = np.sqrt(-2.0 * np.log(unit_mantissa_radius(ra_rb)))
        ang = 2.0 * math.pi * np.where(slot < 2, angle_lo(w[:, 2]), angle_hi(w[:, 2]))
        z[k] = r * np.where(slot % 2 == 0, np.cos(ang), np.sin(ang))
    return z


def brownian_philox_z(seed: int, nodes, n: int, elem_offset: int = 0, latent_seeds=None, latent_elems: int = 0):
    """Philox family, z[k, e]: Philox4x32-10 of counter (e // 4 (64 bit), node (64 bit)), key = seed, then two Box-Muller pairs.  With
    ``latent_seeds`` (one per latent of THIS call) the key is the latent's seed and the counter restarts in each latent."""
    e = np.arange(elem_offset, elem_offset + n, dtype=np.int64)
    if latent_seeds is None:
        keys = [int(seed)]
        key_of = np.zeros(n, dtype=np.int64)
        ctr = e // 4
    else:
        local = e - elem_offset
        key_of = local // latent_elems
        keys = [int(s) for s in latent_seeds]
        ctr = (local - key_of * latent_elems) // 4
    z = np.empty((len(nodes), n), dtype=np.float64)
    for k, node in enumerate(nodes):
        for li, key in enumerate(keys):
            m = key_of == li
            vals = philox_normal4(key, int(node), ctr[m].astype(np.uint64))  # [m, 4]
            z[k, m] = vals[np.arange(m.sum()), (e[m] % 4)]
    return z


def brownian_family(n: int, elem_offset: int, latent_elems: int, latent_seeds=None) -> str:
    """Which family a call's values come from: "burst" for one seed and latents of a multiple of 4096 elements with the call on whole
    latents, "philox" otherwise.  A function of the shape and the seed kind only -- never of buffer addresses."""
    if (latent_seeds is None and latent_elems > 0 and latent_elems % TILE_ELEMS == 0 and n % latent_elems == 0
            and elem_offset % latent_elems == 0):
        return "burst"
    return "philox"


def brownian_z(seed: int, nodes, n: int, elem_offset: int = 0, latent_elems: int = 0, latent_seeds=None):
    """z[k, e] of the family the call gets (brownian_family)."""
    if brownian_family(n, elem_offset, latent_elems, latent_seeds) == "burst":
        return brownian_burst_z(seed, nodes, n, elem_offset)
    return brownian_philox_z(seed, nodes, n, elem_offset, latent_seeds, latent_elems)


def brownian_expansion(seed: int, nodes, coefs, n: int, elem_offset: int = 0, latent_elems: int = 0, latent_seeds=None):
    """sum_k coefs[k] z(nodes[k], e) in fp64 (sonar_brownian_f32's value)."""
    if len(nodes) == 0:
        return np.zeros(n)
    z = brownian_z(seed, nodes, n, elem_offset, latent_elems, latent_seeds)
    return np.asarray(coefs, dtype=np.float64) @ z


# ------------------------------------------------------------------------------------------------ the virtual Brownian tree
def tree_grid_time(t_lo: float, t_hi: float, depth: int, g: int) -> float:
    cells = 1 << depth
    return t_lo if g <= 0 else t_hi if g >= cells else t_lo + g * ((t_hi - t_lo) / cells)


def tree_point(t_lo: float, t_hi: float, depth: int, g: int) -> dict:
    """{node: coefficient} of W at grid index g in [0, 2^depth]: W(t_lo) = 0, W(t_hi) = sqrt(t_hi - t_lo) z(0), and each midpoint of a
    dyadic interval (a, b) is the Brownian bridge ((b - t) W(a) + (t - a) W(b)) / (b - a) + sqrt((t - a)(b - t) / (b - a)) z(h), h the
    heap number of the interval (1 for the whole range, children 2h and 2h + 1)."""
    cells = 1 << depth
    w_lo, w_hi = {}, {0: math.sqrt(t_hi - t_lo)}
    if g <= 0:
        return w_lo
    if g >= cells:
        return w_hi
    lo, hi, h = 0, cells, 1
    while True:
        m = (lo + hi) // 2
        a, b, tm = (tree_grid_time(t_lo, t_hi, depth, i) for i in (lo, hi, m))
        fb = (tm - a) / (b - a)
        w_m = {k: (1.0 - fb) * w_lo.get(k, 0.0) + fb * w_hi.get(k, 0.0) for k in w_lo.keys() | w_hi.keys()}
        w_m[h] = math.sqrt((tm - a) * (b - tm) / (b - a))
        if m == g:
            return w_m
        if g < m:
            hi, w_hi, h = m, w_m, 2 * h
        else:
            lo, w_lo, h = m, w_m, 2 * h + 1


def tree_increment(t_lo: float, t_hi: float, depth: int, g0: int, g1: int) -> dict:
    """{node: coefficient} of (W(t1) - W(t0)) / sqrt(t1 - t0) for grid indices g0 != g1 (in either order)."""
    ga, gb = min(g0, g1), max(g0, g1)
    ta, tb = tree_grid_time(t_lo, t_hi, depth, ga), tree_grid_time(t_lo, t_hi, depth, gb)
    ca, cb = tree_point(t_lo, t_hi, depth, ga), tree_point(t_lo, t_hi, depth, gb)
    s = 1.0 / math.sqrt(tb - ta)
    return {k: (cb.get(k, 0.0) - ca.get(k, 0.0)) * s for k in ca.keys() | cb.keys()}


# ------------------------------------------------------------------------------------------------ half-spectrum draws (power_core.h:162-300, power_any_core.h:237-266, power_block.h:10-16)
FFT_THREADS = 512    # power_core.h kFftThreads
ANY_SLOTS = 512      # power_any_core.h kAnySlots
BLOCK_SLOTS = 512    # power_block.h kBlockSlots
BLOCK_COLS_MAX = 32  # power_block.h kBlockColsMax
FIXED_PLANES = ((128, 128), (64, 64), (32, 32), (16, 16), (256, 128), (128, 256), (128, 64), (64, 128), (64, 32), (32, 64),
                (256, 64), (64, 256))  # power_fft.hip sonar_power_plane_kind: kind 1


def plane_threads(H: int, W: int) -> int:
    """Thread slots of a fixed-size plane's workgroup (power_core.h plane_threads)."""
    return FFT_THREADS if H * W >= 8192 else 256 if H * W >= 2048 else 128 if H * W >= 1024 else 64


def rng_group(C: int) -> int:
    """Planes per RNG group: 4 when the channel count is a multiple of 4, else 1 (hip_lib.rng_group_for)."""
    return 4 if C % 4 == 0 else 1


def unit_complex_normal(r, angle):
    """unit_complex_normal in fp64: sqrt(-ln u) e^{2 pi i angle}, u = 2 - unit_mantissa(r) -- E|z|^2 = 1."""
    return np.sqrt(-np.log(unit_mantissa_radius(r))) * np.exp(2j * math.pi * angle)


def spectrum_streams(seed: int, stream: int, ggroup: int, slots, edge):
    """spectrum_seed: one Philox4x32 block of counter (4 ggroup, stream id, slot), key seed.  R = Mwc::seeded(w0, w1) and
    T = Mwc::seeded(w2, w3) after 10 rounds; E = Mwc::seeded of the first two words after 2 more rounds (edge slots only)."""
    slots = _u64(slots)
    tile = int(ggroup) << 2
    stream, seed = int(stream) & (2**64 - 1), int(seed) & (2**64 - 1)
    args = (np.full_like(slots, tile & 0xFFFFFFFF), np.full_like(slots, tile >> 32), np.full_like(slots, stream & 0xFFFFFFFF),
            (np.uint64(((stream >> 32) << 16) & 0xFFFFFFFF) ^ slots) & U32, seed & 0xFFFFFFFF, seed >> 32)
    w = philox4x32(*args, rounds=10)
    e = philox4x32(*args, rounds=12) if edge else None
    return Mwc.seeded(w[0], w[1]), Mwc.seeded(w[2], w[3]), (Mwc.seeded(e[0], e[1]) if edge else None)


def _slot_pairs(nslots: int, pairs: int):
    """Slot s draws pairs p = s, s + nslots, ...: per slot the count, and the (slot, k) -> p table as flat arrays."""
    cnt = np.array([(pairs - s + nslots - 1) // nslots if s < pairs else 0 for s in range(nslots)], dtype=np.int64)
    p = np.arange(pairs, dtype=np.int64)
    return cnt, p % nslots, p // nslots, p


def _draw_group(seed, stream, ggroup, slot_ids, pairs, nplanes, H, edge_rows):
    """Words of the first ``nplanes`` planes a group's slots draw: per plane j, (ra, rb, t) of every pair p (in p order) and (r0, rm, t)
    of the edge rows.  A slot's R / T / E streams run on from plane to plane (a unit that starts inside a group fast-forwards)."""
    nslots = len(slot_ids)
    cnt, s_of, k_of, _ = _slot_pairs(nslots, pairs)
    R, T, E = spectrum_streams(seed, stream, ggroup, slot_ids, edge_rows > 0)
    kmax = int(cnt.max()) if pairs else 0
    rw, tw = R.words(2 * kmax * nplanes), T.words(kmax * nplanes)       # [slots, words]: enough for the longest slot
    ew = E.words(3 * nplanes) if edge_rows else None
    out = []
    for j in range(nplanes):
        base = j * cnt[s_of]
        ra, rb = rw[s_of, 2 * base + 2 * k_of], rw[s_of, 2 * base + 2 * k_of + 1]
        t = tw[s_of, base + k_of]
        edges = None if not edge_rows else (ew[:edge_rows, 3 * j], ew[:edge_rows, 3 * j + 1], ew[:edge_rows, 3 * j + 2])
        out.append((ra, rb, t, edges))
    return out


def spectrum_kind(H: int, W: int) -> int:
    """1 fixed-size, 2 general-size LDS plane, 4 column blocks -- the draw orders stated here (not the size limits of kinds 2 / 4)."""
    if (H, W) in FIXED_PLANES:
        return 1
    return 4 if H * (W // 2 + 1) * 8 + (H + W) * 8 > 160 * 1024 else 2


def spectrum_draws(seed: int, stream: int, planes: int, H: int, W: int, plane_offset: int = 0, group: int = 1, kind: int = 0):
    """The unit complex-normal half-spectra [planes, H, W/2 + 1] (complex128) that generate mode draws for the global planes
    plane_offset .. plane_offset + planes - 1.  RNG group g = global plane // group owns the streams; its planes are drawn back to back.
      kind 1 / 2 (fixed / general size): NT = plane_threads(H, W) or 512 slots; slot ky < H draws the edge columns kx = 0 and M from E
        (words r0, rm, t); slot s draws pairs p = s, s + NT, ..., pair p = element (p // M, 1 + p % M) and its partner H/2 rows below
        (words ra, rb from R, t from T); the kx = M pair slot is drawn and discarded.
      kind 4 (column blocks): S = M + 1 columns in nblk = ceil(S / 32) blocks of bw = ceil(S / nblk); block d uses the slots
        d * 512 + tid, no E stream; pair p of a block of ncd columns = element (p // ncd, c0 + p % ncd) and its partner.
    Radius words through unit_mantissa, angle words as angle_lo (the element) / angle_hi (its partner)."""
    kind = kind or spectrum_kind(H, W)
    M, S = W // 2, W // 2 + 1
    z = np.zeros((planes, H, S), dtype=np.complex128)
    gplanes = np.arange(plane_offset, plane_offset + planes)
    for g in np.unique(gplanes // group):
        need = int(gplanes[gplanes // group == g].max() - g * group + 1)
        local = [(int(p - plane_offset), int(p - g * group)) for p in gplanes if p // group == g]
        if kind in (1, 2):
            nt = plane_threads(H, W) if kind == 1 else ANY_SLOTS
            pairs = (H // 2) * M
            p = np.arange(pairs)
            ky, kx = p // M, 1 + p % M
            keep = kx < M
            draws = _draw_group(seed, stream, int(g), np.arange(nt), pairs, need, H, H)
            for li, j in local:
                ra, rb, t, (r0, rm, te) = draws[j]
                z[li, ky[keep], kx[keep]] = unit_complex_normal(ra[keep], angle_lo(t[keep]))
                z[li, ky[keep] + H // 2, kx[keep]] = unit_complex_normal(rb[keep], angle_hi(t[keep]))
                z[li, :, 0] = unit_complex_normal(r0, angle_lo(te))
                z[li, :, M] = unit_complex_normal(rm, angle_hi(te))
        else:
            nblk = -(-S // BLOCK_COLS_MAX)
            bw = -(-S // nblk)
            for d in range(nblk):
                c0 = d * bw
                ncd = min(bw, S - c0)
                pairs = (H // 2) * ncd
                p = np.arange(pairs)
                ky, c = p // ncd, c0 + p % ncd
                draws = _draw_group(seed, stream, int(g), d * BLOCK_SLOTS + np.arange(BLOCK_SLOTS), pairs, need, H, 0)
                for li, j in local:
                    ra, rb, t, _ = draws[j]
                    z[li, ky, c] = unit_complex_normal(ra, angle_lo(t))
                    z[li, ky + H // 2, c] = unit_complex_normal(rb, angle_hi(t))
    return z


def spectrum_draw_order(H: int, W: int, kind: int = 0):
    """How often each half-spectrum element is drawn by one plane's draw order, and how many drawn words are discarded: (counts [H, S],
    discarded pairs).  Every element must be drawn exactly once; the only waste is the kx = M pair slot of kinds 1 and 2."""
    kind = kind or spectrum_kind(H, W)
    M, S = W // 2, W // 2 + 1
    counts = np.zeros((H, S), dtype=np.int64)
    if kind in (1, 2):
        nt = plane_threads(H, W) if kind == 1 else ANY_SLOTS
        assert H <= nt, "edge rows are slots"
        counts[:, 0] += 1
        counts[:, M] += 1
        pairs = (H // 2) * M
        cnt, s_of, k_of, p = _slot_pairs(nt, pairs)
        assert np.array_equal(s_of + k_of * nt, p)
        ky, kx = p // M, 1 + p % M
        keep = kx < M
        np.add.at(counts, (ky[keep], kx[keep]), 1)
        np.add.at(counts, (ky[keep] + H // 2, kx[keep]), 1)
        return counts, int((~keep).sum())
    nblk = -(-S // BLOCK_COLS_MAX)
    bw = -(-S // nblk)
    for d in range(nblk):
        c0, ncd = d * bw, min(bw, S - d * bw)
        p = np.arange((H // 2) * ncd)
        np.add.at(counts, (p // ncd, c0 + p % ncd), 1)
        np.add.at(counts, (p // ncd + H // 2, c0 + p % ncd), 1)
    return counts, 0
