"""The cases of tests/golden/voronoi_rank.npz: VoronoiNoiseGenerator's modes that read past f4 in the sorted row (the rank route,
csrc/voronoi.hip: voronoi_rank_kernel).  Shared by the generator (make_voronoi_rank_golden.py, which runs the reference) and by
tests/test_voronoi_rank_cpu.py and tests/test_gpu_voronoi_rank.py (which read only the file).  Plain data, no imports.

Every case is three consecutive calls of one generator, as in voronoi_cases.py.  Shapes: 2 x 3 x 8 x 12 and the ragged 1 x 1 x 5 x 7;
n_points 5 and 6 (odd and even: torch.median takes the lower middle value), 33, 256 (the longest row softmin:use_sorted is built for) and
257 (one past the staging chunk)."""

SEED = 20262
CALLS = 3
A = (2, 3, 8, 12)
B = (1, 1, 5, 7)
ROW_N = 256

MEDIAN = (
    ("median_n5", A, dict(n_points=(5,), result_mode=("median_distance",))),
    ("median_n6", A, dict(n_points=(6,), result_mode=("median_distance",))),
    ("median_n33", B, dict(n_points=(33,), result_mode=("median_distance",))),
    ("median_n257", B, dict(n_points=(257,), result_mode=("median_distance",))),
)
INDEX = (
    ("f_idx4", A, dict(n_points=(33,), result_mode=("f:idx=4",))),
    ("f_idx_last", A, dict(n_points=(33,), result_mode=("f:idx=-1",))),
    ("f_idx_m5_n5", B, dict(n_points=(5,), result_mode=("f:idx=-5",))),    # lands on rank 0
    ("inv_f_idx7", A, dict(n_points=(33,), result_mode=("inv_f:idx=7",))),
    ("diff_2_9", A, dict(n_points=(33,), result_mode=("diff:idx1=2:idx2=9",))),
    ("diff2_m2_m1", A, dict(n_points=(33,), result_mode=("diff2:idx1=-2:idx2=-1",))),
)
SORTED = (
    ("softsorted_n5", B, dict(n_points=(5,), result_mode=("softmin:use_sorted=1:temperature=20",))),
    ("softsorted_n33", A, dict(n_points=(33,), result_mode=("softmin:use_sorted=1:temperature=20",))),
    ("softsorted_n256", A, dict(n_points=(ROW_N,), result_mode=("softmin:use_sorted=1:temperature=20",))),
)
WRAPPED = (
    ("ridge_median", A, dict(n_points=(33,), result_mode=("ridge:name=median_distance",))),
    ("fractal_f6", A, dict(n_points=(33,), result_mode=("fractal_norm:name=f:idx=6",))),
    ("gradient_median", A, dict(n_points=(33,), result_mode=("gradient_magnitude:name1=median_distance",))),
    ("fuzz_f5", A, dict(n_points=(33,), result_mode=("fuzz:name=f:idx=5",))),
    ("sum_rscale", A, dict(n_points=(33,), result_mode=("diff2+median_distance:rscale=0.5+softmin",))),
    ("oct2_new", A, dict(n_points=(5, 33), octaves=2, octave_mode="new_features", result_mode=("median_distance", "diff:idx2=4"))),
)
DISTANCE = (
    ("d_sum_f4", A, dict(n_points=(33,), distance_mode=("chebyshev+quadratic",), result_mode=("f:idx=4",))),
    ("d_fuzz_median", B, dict(n_points=(5,), distance_mode=("fuzz",), result_mode=("median_distance",))),  # the fuzz distance's pass 2 on this route
)
# the one-octave cases that are one launch (no plane mode, no fuzz distance: those take more than one)
KERNEL = tuple(n for n, _l, _p in (*MEDIAN, *INDEX, *SORTED, *WRAPPED[:2], WRAPPED[4], DISTANCE[0]))


def cases():
    return [*MEDIAN, *INDEX, *SORTED, *WRAPPED, *DISTANCE]
