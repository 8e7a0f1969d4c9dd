"""The cases of tests/golden/collatz.npz: shared by the generator (make_collatz_golden.py, which runs the reference) and by
tests/test_collatz_cpu.py and tests/test_gpu_collatz.py (which read only the file).  Plain data, no imports."""

LATENT = (2, 3, 6, 10)
SEED = 1234                       # torch.manual_seed before every reference call
CHAIN_LENGTHS = (1, 2, 3, 4, 7, 16)  # a chain longer than the last two dimensions, ragged last chunks, a single chunk
ALL_DIMS = (-1, -2, 1, 0)
OUTPUT_MODES = ("values", "ratios", "mults", "adds", "seed_x_ratios", "seed_x_mults", "seed_x_adds", "noise_x_ratios", "noise_x_mults",
                "noise_x_adds")
RAW_MODES = ("ratios", "mults", "adds")  # the modes whose per-iteration output is the kept values alone

# what every case starts from: 12 iterations walk (dim, chain length) through half of the 24 pairs, the rotated lengths through the other half
BASE = dict(iterations=12, dims=ALL_DIMS, chain_length=CHAIN_LENGTHS, chain_offset=5, quantile=0, output_mode="ratios", rmin=-8000.0,
            rmax=8000.0)
ROTATED = CHAIN_LENGTHS[1:] + CHAIN_LENGTHS[:1]
SHORT = dict(iterations=4, chain_length=(3, 4, 7, 16))


def cases():
    """(name, parameters over the generator's defaults).  Exact cases have quantile 0 or 1 and no adjust_scale."""
    out = []

    def add(name, **kw):
        out.append((name, BASE | kw))

    for flatten in (False, True):
        f = "flat" if flatten else "dims"
        add(f"layout_{f}_off5", flatten=flatten)
        add(f"layout_{f}_off0_rot", flatten=flatten, chain_offset=0, chain_length=ROTATED)
        add(f"layout_{f}_values_rot", flatten=flatten, chain_length=ROTATED, output_mode="values")
    for mode in OUTPUT_MODES:
        add(f"mode_{mode}", output_mode=mode, **SHORT)
        add(f"mode_{mode}_flat_off0", output_mode=mode, flatten=True, chain_offset=0, **SHORT)
    for key in ("integer_math", "break_loops", "add_preserves_sign"):
        add(f"no_{key}", **{key: False}, **SHORT)
        add(f"no_{key}_adds", output_mode="adds", **{key: False}, **SHORT)
    for seed_mode in ("default", "force_odd", "force_even"):
        add(f"seed_{seed_mode}", seed_mode=seed_mode, output_mode="values", **SHORT)
    add("unit_multipliers", even_multiplier=1, odd_multiplier=1, even_addition=2, **SHORT)
    add("unit_multipliers_adds", even_multiplier=1.0, odd_multiplier=1.0, even_addition=2.0, output_mode="adds", **SHORT)
    add("no_additions", even_addition=0.0, odd_addition=0.0, output_mode="mults", **SHORT)
    add("one_sided", even_multiplier=1.0, odd_multiplier=2.5, even_addition=0.0, odd_addition=-1.5, output_mode="values", **SHORT)
    add("no_sign_flipping", iteration_sign_flipping=False, output_mode="values", **SHORT)
    add("wide_range", rmin=-9500.0, rmax=9500.0, **SHORT)
    add("positive_range", rmin=1.0, rmax=100.0, output_mode="adds", **SHORT)
    add("defaults", iterations=10, dims=(-1, -1, -2, -2), chain_length=(1, 1, 2, 2, 3, 3), quantile=1, output_mode="values")
    # the quantile stage (and adjust_scale) is the one inexact stage: these are held to quantile_normalize's tolerance
    add("quantile_half_clamp", quantile=0.5, quantile_strategy="clamp", output_mode="values", **SHORT)
    add("quantile_half_clamp_flat", quantile=0.5, quantile_strategy="clamp", flatten=True, **SHORT)
    add("quantile_tanh", quantile=0.75, quantile_strategy="tanh", output_mode="noise_x_adds", **SHORT)
    add("quantile_default_call", iterations=10, dims=(-1, -1, -2, -2), chain_length=(1, 1, 2, 2, 3, 3), quantile=0.5, output_mode="values")
    add("adjust_scale", adjust_scale=True, output_mode="values", **SHORT)
    return out


def is_exact(params):
    return params["quantile"] in (0, 1) and not params.get("adjust_scale", False)


ITEM = dict(latent=LATENT, factor=0.8, global_seed=7, seed=42, sigma_min=0.1, sigma_max=10.0, sigmas=((10.0, 5.0), (5.0, 2.0)),
            params=dict(iterations=4, dims=ALL_DIMS, chain_length=(3, 4, 7, 16), chain_offset=5, quantile=0.5, quantile_strategy="clamp",
                        output_mode="noise_x_ratios", rmin=-8000.0, rmax=8000.0, adjust_scale=False, iteration_sign_flipping=True,
                        flatten=False, noise_dtype="float32", integer_math=True, add_preserves_sign=True, even_multiplier=0.5,
                        even_addition=0.0, odd_multiplier=3.0, odd_addition=1.0, seed_mode="default", break_loops=True))
