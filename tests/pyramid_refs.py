"""What the pyramid oracle tests share: an fp64 resampler with ATen's index rules, the budget arithmetic that routes a pyramid call to
one of its kernels, and the case tables (tests/test_pyramid_refs_cpu.py checks the resampler and the tables without a GPU,
tests/test_gpu_pyramid_oracle.py compares the kernels with oracle/device_streams.py through them).

The resampler: index selection as F.interpolate does it for float32 tensors -- the scale in / out and the source coordinate in float32,
then floor, the clamps and lambda -- and everything after that (weights from lambda, taps times weights, the sums) in float64.  Modes
bilinear, nearest-exact, nearest, area and bicubic (A = -0.75), align_corners=False.  Area takes the exact integer windows
[floor(i in / out), ceil((i + 1) in / out)).

One known difference: a compiler may contract scale * (dst + 0.5) - 0.5 into a fused multiply-add -- one rounding of the source
coordinate where the written code has two.  hipcc does so by default; the library is built with contraction off (``fused=False``, what
the GPU tests use), ATen's vectorised CPU kernels are built with it on where the CPU has FMAs (``fused=True``).  The coordinate moves by
at most an ulp, lambda with it; at a coordinate that lands exactly on a sample this moves i0 by one with lambda ~ 0 or ~ 1.  Bilinear and
bicubic are continuous there, so the value moves by rounding only (an ulp of the coordinate times the slope of the grid).  The nearest
modes use a single multiply and are unaffected.
"""
from __future__ import annotations

import numpy as np

MODES = ("bilinear", "nearest-exact", "nearest", "area", "bicubic")
_F = np.float32


def _scale(n_in: int, n_out: int):
    return _F(n_in) / _F(n_out)


def _source(n_in: int, n_out: int, fused: bool):
    """The float32 source coordinate of every output index (align_corners=False), the product rounded on its own or not."""
    half = np.arange(n_out).astype(_F) + _F(0.5)
    if fused:
        return (np.float64(_scale(n_in, n_out)) * half.astype(np.float64) - 0.5).astype(_F)   # (the fp64 product of two floats is exact)
    return (_scale(n_in, n_out) * half - _F(0.5)).astype(_F)


def _linear_matrix(n_in: int, n_out: int, fused: bool):
    d = np.arange(n_out)
    src = _source(n_in, n_out, fused)
    src = np.where(src < 0, _F(0), src).astype(_F)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    lam = np.clip(src - i0.astype(_F), _F(0), _F(1)).astype(np.float64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (d, i0), 1.0 - lam)
    np.add.at(m, (d, i1), lam)
    return m


def _select_matrix(idx, n_in: int):
    m = np.zeros((len(idx), n_in))
    m[np.arange(len(idx)), idx] = 1.0
    return m


def nearest_exact_index(n_in: int, n_out: int):
    d = np.arange(n_out).astype(_F)
    return np.minimum(np.floor((d + _F(0.5)) * _scale(n_in, n_out)).astype(np.int64), n_in - 1)


def nearest_index(n_in: int, n_out: int):
    d = np.arange(n_out).astype(_F)
    return np.minimum(np.floor(d * _scale(n_in, n_out)).astype(np.int64), n_in - 1)


def area_windows(n_in: int, n_out: int):
    d = np.arange(n_out, dtype=np.int64)
    return (d * n_in) // n_out, -((-(d + 1) * n_in) // n_out)


def _area_matrix(n_in: int, n_out: int):
    lo, hi = area_windows(n_in, n_out)
    m = np.zeros((n_out, n_in))
    for d in range(n_out):
        m[d, lo[d]:hi[d]] = 1.0 / (hi[d] - lo[d])
    return m


def _cubic_matrix(n_in: int, n_out: int, fused: bool):
    A = -0.75
    d = np.arange(n_out)
    src = _source(n_in, n_out, fused)
    fl = np.floor(src)
    t = (src - fl).astype(np.float64)
    i0 = fl.astype(np.int64)

    def inner(x):   # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0

    def outer(x):   # 1 < |x| < 2
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A

    coef = (outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t))
    m = np.zeros((n_out, n_in))
    for k in range(4):
        np.add.at(m, (d, np.clip(i0 - 1 + k, 0, n_in - 1)), coef[k])
    return m


def axis_matrix(n_in: int, n_out: int, mode: str, fused: bool = False):
    """[n_out, n_in] fp64: output = matrix @ input along one axis (every mode is separable)."""
    if mode == "bilinear":
        return _linear_matrix(n_in, n_out, fused)
    if mode == "nearest-exact":
        return _select_matrix(nearest_exact_index(n_in, n_out), n_in)
    if mode == "nearest":
        return _select_matrix(nearest_index(n_in, n_out), n_in)
    if mode == "area":
        return _area_matrix(n_in, n_out)
    if mode == "bicubic":
        return _cubic_matrix(n_in, n_out, fused)
    raise ValueError(mode)


def resize(grids, H: int, W: int, mode: str, fused: bool = False):
    """[..., h, w] -> [..., H, W] in fp64.  ``fused``: the source coordinate of bilinear / bicubic rounded once (module docstring)."""
    g = np.asarray(grids, dtype=np.float64)
    h, w = g.shape[-2:]
    return np.einsum("yi,...ij,xj->...yx", axis_matrix(h, H, mode, fused), g, axis_matrix(w, W, mode, fused), optimize=True)


# ------------------------------------------------------------------------------------------------ the route (noise_pyramid.hip pyramid_route)
LDS_BUDGET = 64 * 1024   # kPyramidLdsBudget
LIN_BYTES = 16           # sizeof(Lin): one coordinate-table entry
FLAT, PLANE, STRETCHED = 0, 1, 2


def budget(H: int, W: int, levels, mode: str):
    """(lds, lds_x) in bytes for the grids of ``levels`` = [(grid or None, h, w, weight), ...]: the grids (rounded up to 16 bytes), a
    coordinate-table entry per (level, row) and (level, column) for bilinear and area, and for lds_x every level's rows stretched to W."""
    sizes = grid_sizes(H, W, levels)
    floats = (sum(h * w for h, w in sizes) + 3) & ~3
    lds = floats * 4 + (len(sizes) * (H + W) * LIN_BYTES if mode in ("bilinear", "area") else 0)
    return lds, lds + sum(h for h, _ in sizes) * W * 4


def grid_sizes(H: int, W: int, levels):
    """The (h, w) of the levels that take a grid: all but the first drawn level of the latent's own size (folded into the base draw)."""
    sizes, folded = [], False
    for grid, h, w, _ in levels:
        if grid is None and (h, w) == (H, W) and not folded:
            folded = True
            continue
        sizes.append((h, w))
    return sizes


def route(H: int, W: int, levels, mode: str, elem_offset: int = 0) -> int:
    lds, lds_x = budget(H, W, levels, mode)
    if W % 4 != 0 or elem_offset % (H * W) != 0 or lds > LDS_BUDGET:
        return FLAT
    return STRETCHED if mode == "bilinear" and lds_x <= LDS_BUDGET else PLANE


# ------------------------------------------------------------------------------------------------ case tables
SEEDS = (2**64 - 1, 2**32 + 5)
STREAMS = (2**32 + 3, 2**47 + 1)
S = "supplied"   # a level whose grid the test passes in (torch.randn on the host); None: drawn in the kernel

TWELVE = [(None, h, w, 0.9 - 0.07 * i) for i, (h, w) in enumerate(
    [(1, 1), (2, 2), (3, 3), (1, 2), (2, 1), (3, 2), (1, 3), (2, 3), (1, 4), (2, 4), (1, 5), (2, 5)])]

# (name, shape, levels, mode, route, statistics, shard offsets in planes): the plane kernel with drawn grids
PLANE_CASES = [
    # route 2, bilinear
    ("tile_per_plane", (2, 4, 64, 64), [(None, 64, 64, 1.0), (None, 21, 20, 0.7), (None, 3, 3, 0.49)], "bilinear", 2, True, (0, 1, 5)),
    ("four_planes_per_tile", (3, 4, 32, 32), [(None, 33, 33, 0.8), (None, 5, 7, -0.6), (None, 1, 1, 0.3)], "bilinear", 2, False, (0,)),
    ("sub_tile_4x4", (5, 3, 4, 4), [(None, 9, 9, 0.7), (None, 4, 4, 1.0), (None, 3, 3, 0.49)], "bilinear", 2, True, (0, 1, 5)),
    ("sub_tile_8x12", (3, 2, 8, 12), [(None, 3, 10, 0.6), (None, 1, 1, 0.3)], "bilinear", 2, False, (0,)),
    ("straddling_40x36", (4, 1, 40, 36), [(None, 40, 36, 0.8), (S, 21, 20, 0.7), (None, 5, 7, 0.5), (S, 3, 3, -0.4)], "bilinear", 2, True,
     (0, 1, 5)),
    ("tiles_3_86", (2, 1, 104, 152), TWELVE, "bilinear", 2, False, (0,)),
    ("five_tiles", (1, 2, 128, 160), [(None, 128, 160, 1.0), (None, 21, 20, 0.5), (None, 8, 10, 0.25)], "bilinear", 2, True, (0,)),
    ("one_row_per_round", (2, 1, 8, 512), [(None, 3, 3, 0.7), (None, 8, 512, 0.9), (None, 2, 5, 0.4)], "bilinear", 2, False, (0,)),
    ("wider_than_a_round", (2, 1, 4, 1024), [(None, 1, 1, 0.5), (None, 3, 3, 0.7)], "bilinear", 2, False, (0,)),
    ("more_planes_than_workgroups", (1027, 1, 4, 8), [(None, 3, 3, 0.7), (None, 2, 5, 0.5)], "bilinear", 2, True, (0,)),
    # route 1: the stretched rows do not fit (lds 37,920 B, lds_x 70,688 B)
    ("rows_do_not_fit", (2, 2, 64, 64), [(None, 63, 63, 0.7), (None, 63, 63, 0.5), (None, 2, 3, 0.3)], "bilinear", 1, True, (0,)),
    # route 1: nearest-exact and area
    ("nearest_64", (2, 4, 64, 64), [(None, 64, 64, 1.0), (None, 21, 20, 0.7), (None, 5, 7, 0.49)], "nearest-exact", 1, True, (0,)),
    ("nearest_40x36", (4, 1, 40, 36), [(None, 21, 20, 0.7), (None, 33, 33, 0.5), (None, 5, 7, 0.3)], "nearest-exact", 1, False, (0,)),
    ("area_64", (2, 4, 64, 64), [(None, 21, 20, 0.7), (None, 64, 64, 1.0), (None, 5, 7, 0.49)], "area", 1, False, (0,)),
    ("area_40x36", (4, 1, 40, 36), [(None, 21, 20, 0.7), (None, 50, 45, 0.5), (None, 5, 7, 0.3)], "area", 1, True, (0,)),
]
THIRTEEN = TWELVE + [(None, 1, 6, 0.05)]   # refused: ERR_UNSUPPORTED

# (name, shape, levels, elem_offset, route per mode): the flat kernel, supplied grids.  The 127 x 127 grid alone takes 64,516 B: with the
# coordinate tables of bilinear and area that is over the budget; nearest-exact keeps no tables, so there the pair fits (64,656 B) and
# the plane kernel runs -- the third level of the next case puts every mode over.
FLAT_MODES = ("bilinear", "nearest-exact", "area")
FLAT_CASES = [
    ("over_budget", (2, 2, 64, 64), [(S, 127, 127, 0.7), (S, 5, 7, 0.5)], 0, {"bilinear": 0, "nearest-exact": 1, "area": 0}),
    ("over_budget_every_mode", (1, 2, 64, 64), [(S, 127, 127, 0.7), (S, 5, 7, 0.5), (S, 16, 15, 0.3)], 0,
     {"bilinear": 0, "nearest-exact": 0, "area": 0}),
    ("part_plane_shard", (1, 3, 32, 36), [(S, 9, 9, 0.7), (S, 33, 35, 0.6), (S, 5, 7, 0.5)], 4 * 77, {"bilinear": 0, "nearest-exact": 0, "area": 0}),
]

# sonar_level_normal_f32: (shape, plane_offset, sd)
LEVEL_NORMAL_CASES = [((3, 1, 5, 7), 1, 0.5), ((1, 2, 16, 16), 0, 1.75), ((2, 1, 5, 7), 2**34 // 35 + 1, 0.25), ((2, 1, 5, 7), 1, 3.0)]

# sonar_levels_sampled_f32: levels (h, w, weight, sd)
SAMPLED_SHAPE, SAMPLED_PLANE_OFFSET = (1, 3, 24, 40), 8
SAMPLED_LEVELS = [(48, 80, 1.0, 0.5), (96, 160, 0.7, 0.25), (50, 70, -0.6, 1.5), (24, 40, 0.49, 0.8), (7, 5, 0.3, 2.0)]
SAMPLED_AREA_LEVELS = SAMPLED_LEVELS[:2]
SAMPLED_MODES = ("bilinear", "nearest-exact", "nearest", "bicubic")
SAMPLED_FAR_SHAPE, SAMPLED_FAR_PLANE_OFFSET = (1, 2, 4, 8), 2**34 // 35 + 1   # the Philox group index of the 5 x 7 level is >= 2^32
SAMPLED_FAR_LEVELS = [(8, 16, 0.7, 0.5), (5, 7, 0.5, 1.5)]
SAMPLED_SIXTEEN_SHAPE = (1, 2, 8, 12)
SAMPLED_SIXTEEN = [(1 + i % 5, 2 + i % 7, 0.9 - 0.05 * i, 0.5 + 0.1 * i) for i in range(16)]


def resize_pairs():
    """Every (source size, destination size, mode) a GPU case resamples."""
    pairs = set()
    for _, shape, levels, mode, *_ in PLANE_CASES:
        pairs |= {((h, w), shape[-2:], mode) for h, w in grid_sizes(*shape[-2:], levels)}
    for _, shape, levels, _, routes in FLAT_CASES:
        pairs |= {((h, w), shape[-2:], mode) for _, h, w, _ in levels for mode in routes}
    for mode in SAMPLED_MODES:
        pairs |= {((h, w), SAMPLED_SHAPE[-2:], mode) for h, w, *_ in SAMPLED_LEVELS}
        pairs |= {((h, w), SAMPLED_FAR_SHAPE[-2:], mode) for h, w, *_ in SAMPLED_FAR_LEVELS}
    pairs |= {((h, w), SAMPLED_SIXTEEN_SHAPE[-2:], "bilinear") for h, w, *_ in SAMPLED_SIXTEEN}
    return sorted(pairs)
