"""The cases of tests/golden/voronoi.npz: shared by the generator (make_voronoi_golden.py, which runs the reference) and by
tests/test_voronoi_cpu.py and tests/test_gpu_voronoi.py (which read only the file).  Plain data, no imports.

Every case is three consecutive calls of one generator.  Shapes are the smallest that reach the edges: 2 x 3 x 8 x 12 (not square, sides no
powers of two: y / H * scale % 1 wraps inexactly; 1 x 2 x 8 x 12 and 1 x 2 x 5 x 7 where the draws are large) and 1 x 1 x 5 x 7 (a ragged tile); n_points 1 (clamps to 2), 5, 33 and 257 (one past the
kernel's staging chunk of 256)."""

SEED = 20261
CALLS = 3
A = (2, 3, 8, 12)
B = (1, 1, 5, 7)
C = (1, 2, 8, 12)
D = (1, 2, 5, 7)
CHUNK_EDGE = 257

DISTANCE = (
    ("d_euclidean", A, dict(n_points=(33,), distance_mode=("euclidean",))),
    ("d_manhatten", A, dict(n_points=(5,), distance_mode=("manhatten",), result_mode=("f2",))),
    ("d_chebyshev", A, dict(n_points=(33,), distance_mode=("chebyshev",), result_mode=("f3",))),
    ("d_minkowski", A, dict(n_points=(33,), distance_mode=("minkowski:p=2.5",), result_mode=("f4",))),
    ("d_quadratic", A, dict(n_points=(5,), distance_mode=("quadratic",), result_mode=("f:idx=1",))),
    ("d_angle", A, dict(n_points=(5,), distance_mode=("angle",))),
    ("d_angle_tanh", A, dict(n_points=(33,), distance_mode=("angle_tanh:idx=0",), result_mode=("diff",))),
    ("d_angle_sigmoid", A, dict(n_points=(5,), distance_mode=("angle_sigmoid:idx=1",), result_mode=("diff2",))),
    ("d_weight", A, dict(n_points=(33,), distance_mode=("weight:h=0.5:w=2.0:z=1.0",))),
    ("d_fractal_sin", A, dict(n_points=(33,), distance_mode=("fractal_norm:name=chebyshev:scale=0.2:multiplier=7",))),
    ("d_fractal_cos", A, dict(n_points=(5,), distance_mode=("fractal_norm:mode=cos",))),
    ("d_sum_dscale", A, dict(n_points=(33,), distance_mode=("euclidean+chebyshev:dscale=0.5+quadratic",), result_mode=("diff2",))),
    ("d_fuzz", B, dict(n_points=(5,), distance_mode=("fuzz",), result_mode=("f2",))),
    ("d_fuzz_sum", D, dict(n_points=(5,), octaves=2, distance_mode=("chebyshev+fuzz:name=weight:h=0.5:fuzz=0.1:dscale=0.5",), result_mode=("diff2",))),
    ("d_nested", A, dict(n_points=(33,), distance_mode=("weight:name=fractal_norm:__name=chebyshev:_mode=sin:h=0.7",))),
)
RESULT = (
    ("r_f_all", A, dict(n_points=(33,), result_mode=("f1+f2+f3+f4",))),
    ("r_inv_f_all", A, dict(n_points=(33,), result_mode=("inv_f1+inv_f3+inv_f4+inv_f2",))),
    ("r_inv_f", A, dict(n_points=(5,), result_mode=("inv_f:idx=2",))),
    ("r_diff", A, dict(n_points=(33,), result_mode=("diff:idx1=1:idx2=3",))),
    ("r_diff2", A, dict(n_points=(33,), result_mode=("diff2",))),
    ("r_ridge", A, dict(n_points=(33,), result_mode=("ridge",))),
    ("r_ridge_nested", A, dict(n_points=(5,), result_mode=("ridge:name=ridge:__name=f2:exp=-3:__exp=2",))),
    ("r_fractal", A, dict(n_points=(33,), result_mode=("fractal_norm:name=f2",))),
    ("r_fractal_cos_ridge", A, dict(n_points=(33,), result_mode=("fractal_norm:mode=cos:name=ridge:__name=diff2",))),
    ("r_softmin", A, dict(n_points=(33,), result_mode=("softmin:temperature=20",))),
    ("r_cellid", A, dict(n_points=(33,), result_mode=("cellid",))),
    ("r_gradient", A, dict(n_points=(33,), result_mode=("gradient_magnitude",))),
    ("r_gradient_two", A, dict(n_points=(33,), result_mode=("diff2+gradient_magnitude:name1=f2:name2=ridge:rscale=0.5+softmin",))),
    ("r_gradient_small", B, dict(n_points=(5,), result_mode=("gradient_magnitude:name1=f2:name2=f2",))),
    ("r_fuzz", A, dict(n_points=(33,), result_mode=("fuzz",))),
    ("r_fuzz_sum", C, dict(n_points=(5,), octaves=2, result_mode=("softmin+fuzz:name=diff2:fuzz=0.1:rscale=2",))),
    ("r_sum_rscale", A, dict(n_points=(33,), result_mode=("f1+ridge:rscale=0.25+softmin",))),
)
OCTAVE_MODES = ("same_invert_odd", "same_invert_even", "same_roll_chan_up", "same_roll_chan_down", "same_roll_dir_up", "same_roll_dir_down")
OCTAVES = (
    ("oct3_lac2_new", A, dict(n_points=(5, 33), octaves=3, lacunarity=2.0, octave_mode="new_features", distance_mode=("euclidean", "chebyshev"),
                              result_mode=("diff2", "f1"))),
    ("oct3_lac17_same", A, dict(n_points=(33,), octaves=3, lacunarity=1.7, gain=0.75, result_mode=("diff2",))),
    *((f"oct3_{om}", C, dict(n_points=(5,), octaves=3, lacunarity=1.7, octave_mode=om, result_mode=("f2",))) for om in OCTAVE_MODES),
)
Z_MODES = (
    ("z_reset", C, dict(n_points=(5,), z_max=1.0, z_max_mode="reset")),
    ("z_bounce", C, dict(n_points=(5,), z_max=1.0, z_max_mode="bounce")),
    ("z_other", C, dict(n_points=(5,), z_max=1.0, z_max_mode="none")),
    ("z_max0_range", C, dict(n_points=(5,), z_max=0, z_initial=2.5, z_increment=0.75, z_range=5.0)),
    ("z_range", C, dict(n_points=(5,), z_increment=1.25, z_range=3.5)),
)
POINTS = (
    ("n1_clamps", B, dict(n_points=(1,), result_mode=("f2",))),
    ("n5_small", B, dict(n_points=(5,), result_mode=("diff2",))),
    ("n257_small", B, dict(n_points=(CHUNK_EDGE,), result_mode=("f4",))),
    ("n257", C, dict(n_points=(CHUNK_EDGE,), result_mode=("diff2",))),
)
# the two NoiseType presets' generators at n_points 33 (VORONOI_FUZZ draws [B, C, H, W, N] uniforms on every call: the small latent)
PRESETS = (
    ("preset_fuzz", D, dict(n_points=(33,), octaves=1, distance_mode=("fuzz:name=angle_tanh:fuzz=0.1",), result_mode=("diff2",), z_max=0.0)),
    ("preset_mix", A, dict(n_points=(33,), octaves=3, distance_mode=("euclidean",), result_mode=("diff2",), octave_mode="new_features",
                           lacunarity=2.0, gain=0.75, z_max=0.0)),
)
# the cases whose ambiguous share may reach 1e-2 (the angle distances, cellid); 1e-3 for every other
WIDE = frozenset(("d_angle", "d_angle_tanh", "d_angle_sigmoid", "r_cellid", "preset_fuzz"))

ITEM = dict(latent=A, factor=0.5, global_seed=77, seed=5, sigma_min=0.03, sigma_max=14.6, sigmas=((14.6, 9.0), (9.0, 4.0), (4.0, 0.03)),
            params=dict(n_points=(33,), distance_mode=("euclidean",), result_mode=("diff2",), octaves=2, octave_mode="new_features", z_max=0.0))


def cases():
    return [*DISTANCE, *RESULT, *OCTAVES, *Z_MODES, *POINTS, *PRESETS]
