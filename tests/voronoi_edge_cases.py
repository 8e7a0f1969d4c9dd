"""The launches that pin csrc/voronoi.hip at its tile, grid, wave and stream edges: shared by tests/test_voronoi_edges_cpu.py (which shows
on the host that every shape reaches the edge it is named for and tells a wrong kernel from a right one) and tests/test_gpu_voronoi_edges.py
(which runs them).  Plain data, no imports.  The fp64 statements of tests/voronoi_refs.py and tests/voronoi_rank_refs.py are the reference at
these shapes; there is no golden file.

A shape is the smallest that reaches its edge:
  T3     1 x 2 x 9 x 67    603 pixels a plane: three 256-pixel tiles, the last ragged (ten ragged 64-pixel tiles on the row instantiation of
                           the rank kernel); nine waves in ten straddle rows; 6030 fuzz uniforms on 5 points, past one 4096-element stream tile
  R192   1 x 2 x 3 x 192   every wave inside one row (the wave-aggregated statistics of fuzz pass 1); the tile boundary at pixel 256 falls
                           inside row 1, whose extremes two workgroups merge through the atomics
  R64    1 x 2 x 5 x 64    each row exactly one wave
  G2100  3 x 700 x 2 x 2   2100 units for at most 2048 workgroups: the grid-stride loop takes a second unit; 4200 statistics rows
  N4096  1 x 1 x 5 x 7     with 4096 points: 16 full staging chunks
  N257F  1 x 1 x 5 x 7     with 257 points and a fuzz distance: chunk base 256 in the uniform's index, 8995 uniforms over three stream tiles
  P      1 x 3 x 419 x 421 529197 elements for the plane kernels' 2048 x 256 threads: their grid-stride loops take a second trip"""

SHAPES = {"T3": (1, 2, 9, 67), "R192": (1, 2, 3, 192), "R64": (1, 2, 5, 64), "G2100": (3, 700, 2, 2), "N4096": (1, 1, 5, 7),
          "N257F": (1, 1, 5, 7), "P": (1, 3, 419, 421)}
# what each tag must reach, by the names tests/test_voronoi_edges_cpu.py gives the facts; (tag, points) for the facts that depend on them
REACHES = (
    ("T3", 5, ("tiles", "ragged_tile", "row_tiles_ragged", "waves_straddle_rows", "stream_tile")),
    ("R192", 5, ("tiles", "ragged_tile", "waves_inside_rows", "row_in_two_tiles")),
    ("R192", 33, ("waves_inside_rows", "row_in_two_tiles", "stream_tile")),
    ("R64", 5, ("tiles", "row_is_a_wave")),
    ("G2100", 2, ("second_unit", "row_second_unit")),
    ("G2100", 5, ("second_unit", "row_second_unit")),
    ("N4096", 4096, ("full_chunks",)),
    ("N257F", 257, ("chunks", "stream_tile", "stream_two_boundaries")),
    ("P", 0, ("plane_second_trip",)),
)

Z_NORM = 0.25
AMPLITUDE, FINAL_DIV = 0.75, 1.75     # every launch accumulates into a random base: out = (base + result * amplitude) / final_div
SEED_TOP, SEED_RANK = 5, 6            # numpy.random.default_rng: the feature points of the top-four and of the rank route's cases
SEED_BASE, SEED_U = 7, 8              # ... the base the launch accumulates into, the uniforms of replay mode
CAP, CAP_WIDE = 1e-3, 1e-2            # the flagged share: conditions on the cases, not measurements

SIMPLE = ("euclidean", "diff2")       # voronoi_octave_kernel<true, -1>
GENERAL = ("chebyshev+quadratic:dscale=0.5", "f1+ridge:rscale=0.25+softmin")
FUZZ = ("fuzz:fuzz=0.1", "f2")
FUZZ_SUM = ("chebyshev+fuzz:name=weight:h=0.5:fuzz=0.1:dscale=0.5", "diff2")   # the fuzz term is term 1
FUZZ_ANGLE = ("fuzz:name=angle_tanh:fuzz=0.1", "diff2")
# the last feature point is placed beside (NEAR) or half a period away in every direction from (FAR) pixel (y, x) of every plane, so that a
# launch that drops it is out of bound there whatever the other points are
NEAR, FAR = ("near", 2, 3), ("far", 2, 3)
PLACE = {("N4096", False): NEAR, ("N257F", False): NEAR, ("N4096", True): FAR, ("N257F", True): NEAR}   # by (tag, rank route)

# ---- 1. one launch of the top-four kernel: (id, tag, points, distance mode, result mode, scale)
OCTAVE = tuple(
    (f"{tag}_{kind}_s{scale}", tag, n, *modes, scale)
    for tag, n in (("T3", 5), ("R192", 5), ("G2100", 2), ("N4096", 4096))
    for kind, modes in (("simple", SIMPLE), ("general", GENERAL))
    for scale in (1.0, 1.7)
) + (
    ("N4096_f4_s1.0", "N4096", 4096, "euclidean", "f4", 1.0),
    ("N4096_f4_s1.7", "N4096", 4096, "euclidean", "f4", 1.7),
    ("T3_cellid_s1.0", "T3", 5, "euclidean", "cellid", 1.0),
    ("T3_cellid_s1.7", "T3", 257, "euclidean", "cellid", 1.7),   # the first-smallest index across tiles AND chunks
)

# ---- 2. the three fuzz launches in replay mode: (id, tag, points, distance mode, result mode, scale, exact)
# exact: the term's inner distance is one correctly rounded operation per step, so the statistics words equal numpy's fp32 reductions bit
# for bit (the angle distances go through acosf / tanhf: their statistics are held through pass 2 only)
FUZZ_REPLAY = (
    ("T3_fuzz", "T3", 5, *FUZZ, 1.0, True),
    ("T3_fuzz_sum_s1.7", "T3", 5, *FUZZ_SUM, 1.7, True),
    ("R192_fuzz", "R192", 5, *FUZZ, 1.0, True),
    ("R192_fuzz_sum_s1.7", "R192", 5, *FUZZ_SUM, 1.7, True),
    ("R192_fuzz_angle", "R192", 33, *FUZZ_ANGLE, 1.0, False),
    ("R64_fuzz", "R64", 5, *FUZZ, 1.0, True),
    ("G2100_fuzz", "G2100", 2, *FUZZ, 1.0, True),
    ("N257F_fuzz_sum", "N257F", 257, *FUZZ_SUM, 1.0, True),
)

# ---- 3. stream mode is replay mode on the host-stated stream: (id, tag, points, distance mode, result mode), at every offset
STREAM_SEED, STREAM_ID = 2**40 + 7, 2**33 + 5
OFFSETS = (0, 175, 4093, 2**33 + 3)
STREAM = tuple((f"{tag}_{kind}", tag, n, *modes)
               for tag, n in (("T3", 5), ("N257F", 257), ("R192", 33))
               for kind, modes in (("fuzz", FUZZ), ("fuzz_sum", FUZZ_SUM))) + (("R192_fuzz_angle", "R192", 33, *FUZZ_ANGLE),)
RANK_STREAM = (
    ("T3_median", "T3", 5, FUZZ[0], "median_distance"),
    ("N257F_median", "N257F", 257, FUZZ_SUM[0], "median_distance"),
    ("R192_median", "R192", 33, FUZZ[0], "median_distance"),
    ("R192_softsorted", "R192", 33, FUZZ_SUM[0], "softmin:use_sorted=1:temperature=20"),   # the row instantiation, 64-pixel tiles
    ("T3_softsorted", "T3", 5, FUZZ[0], "softmin:use_sorted=1:temperature=20"),
)

# ---- 4. one launch of the rank kernel: (id, tag, points, distance mode, result mode, scale)
SOFTSORTED = "softmin:use_sorted=1:temperature=20"
RANK = (
    ("T3_median_n6", "T3", 6, "euclidean", "median_distance", 1.0),
    ("T3_median_n6_s1.7", "T3", 6, "euclidean", "median_distance", 1.7),
    ("G2100_diff", "G2100", 5, "chebyshev+quadratic", "diff:idx1=2:idx2=4", 1.0),
    ("G2100_diff_s1.7", "G2100", 5, "chebyshev+quadratic", "diff:idx1=2:idx2=4", 1.7),
    ("T3_softsorted_n33", "T3", 33, "euclidean", SOFTSORTED, 1.0),
    ("T3_softsorted_n33_s1.7", "T3", 33, "euclidean", SOFTSORTED, 1.7),
    ("G2100_softsorted", "G2100", 5, "euclidean", SOFTSORTED, 1.0),
    ("N4096_last", "N4096", 4096, "euclidean", "f:idx=-1", 1.0),
)
# ranks inside 0..3 on the rank route: the top-four kernel's bits (tag, points, distance mode, result mode)
TOP_FOUR = (
    ("T3", 33, "euclidean", "diff2"),
    ("T3", 257, "chebyshev+quadratic:dscale=0.5", "diff:idx1=1:idx2=3"),
    ("T3", 33, "weight:name=fractal_norm:__name=chebyshev:_mode=sin:h=0.7", "inv_f3+ridge:rscale=0.25+softmin:temperature=20"),
    ("G2100", 5, "euclidean", "f1"),
    ("G2100", 5, "chebyshev+quadratic:dscale=0.5", "diff:idx1=1:idx2=3"),
    ("G2100", 5, "angle_tanh:idx=0", "cellid+inv_f:idx=2"),
)

# ---- 5. the generator under shard_offset(1), generate mode: (id, rank route, latent, parameters)
GENERATOR = (
    ("top_four", False, SHAPES["T3"], dict(n_points=(5,), distance_mode=(FUZZ[0],), result_mode=("f2",))),
    ("rank", True, SHAPES["T3"], dict(n_points=(5,), distance_mode=(FUZZ[0],), result_mode=("median_distance",))),
)
GENERATOR_CALLS = 2

# the cases whose flagged share may reach CAP_WIDE (cellid, the angle distance); CAP for every other
WIDE = frozenset(("T3_cellid_s1.0", "T3_cellid_s1.7", "R192_fuzz_angle"))
