"""Case table of NormalizeToScaleNoise's golden file (shared by tests/golden/make_normalize_dims_golden.py, which runs the reference's item
on the CPU, tests/test_normalize_dims_cpu.py and tests/test_gpu_group_stats.py, which runs the product's on the device): plain data and a
tensor builder, no item code.

A case is (latent, mode, dims, mean_dims, std_dims, the two multipliers, normalize, factor) over the stored noise of its latent: a
recording inner item hands back ``planted(latent)``, the same values on both sides.  The item takes ``mean_dims`` and ``std_dims``
separately (the node gives both the values of ``dims``), so the table does too.  ``error`` names the exception type torch raises for the
case's dims (nothing is stored for those).  The advanced mode's own sockets keep the node's defaults; the simple mode rescales into
[min_negative_value, max_positive_value]."""

LATENTS = {"l4": (3, 4, 6, 10), "l5": (2, 3, 5, 6, 7), "l3": (4, 5, 9), "l1": (1, 3, 4, 5)}
SIGMA = (9.0, 6.0)
TRAILING = (-3, -2, -1)
RANGE = dict(min_negative_value=-3.5, max_negative_value=-0.25, min_positive_value=0.125, max_positive_value=4.0)


def _case(latent, mean_dims, std_dims=None, *, mode="advanced", dims=TRAILING, mean_multiplier=1.0, std_multiplier=1.0, normalize=False,
          factor=1.0, error=None, all_nan=False):
    return dict(latent=latent, mode=mode, dims=tuple(dims), mean_dims=tuple(mean_dims), std_dims=tuple(mean_dims if std_dims is None else std_dims),
                mean_multiplier=mean_multiplier, std_multiplier=std_multiplier, normalize=normalize, factor=factor, error=error, all_nan=all_nan)


def _tag(dims):
    return "all" if not dims else "_".join(str(d).replace("-", "m") for d in dims)


CASES = {}
# (a) one choice of dims for both reductions, advanced mode: every 4-D choice, the trailing one included
for _d in ((0,), (1,), (0, 2, 3), (-2,), (0, -1), (1, 3), (), TRAILING):
    CASES[f"a_l4_{_tag(_d)}"] = _case("l4", _d)
for _d in ((0, 2), (1, 3, 4)):
    CASES[f"a_l5_{_tag(_d)}"] = _case("l5", _d)
for _d in ((0,), (0, 2)):
    CASES[f"a_l3_{_tag(_d)}"] = _case("l3", _d)
# (b) different mean_dims and std_dims in one case (one of them trailing: both routes in one call)
CASES["b_mean_0_std_1_3"] = _case("l4", (0,), (1, 3))
CASES["b_mean_trailing_std_0"] = _case("l4", TRAILING, (0,))
CASES["b_mean_m2_std_trailing"] = _case("l4", (-2,), TRAILING)
CASES["b_l5_mean_0_2_std_1_3_4"] = _case("l5", (0, 2), (1, 3, 4))
# (c) simple mode with non-trailing dims (the node's form: one tuple for all three), and with its own tuple for the rescale
CASES["c_simple_0_2_3"] = _case("l4", (0, 2, 3), mode="simple", dims=(0, 2, 3))
CASES["c_simple_1"] = _case("l4", (1,), mode="simple", dims=(1,))
CASES["c_simple_m2_stats_1_3"] = _case("l4", (1, 3), mode="simple", dims=(-2,))
CASES["c_simple_l5_0_2"] = _case("l5", (0, 2), mode="simple", dims=(0, 2))
CASES["c_simple_l3_0"] = _case("l3", (0,), mode="simple", dims=(0,))
# (d) multipliers; 0 skips the step
CASES["d_half"] = _case("l4", (0, 2, 3), mean_multiplier=0.5, std_multiplier=0.5)
CASES["d_negative"] = _case("l4", (1,), mean_multiplier=-0.25, std_multiplier=-0.25)
CASES["d_no_mean"] = _case("l4", (0,), mean_multiplier=0.0, std_multiplier=0.5)
CASES["d_no_std"] = _case("l4", (1, 3), mean_multiplier=-0.25, std_multiplier=0.0)
CASES["d_l5_half"] = _case("l5", (1, 3, 4), mean_multiplier=0.5, std_multiplier=-0.25)
# (e) normalize forced and disabled, with a factor
CASES["e_forced"] = _case("l4", (0, 2, 3), normalize=True, factor=0.7)
CASES["e_forced_1"] = _case("l4", (1,), normalize=True, factor=-0.3)
CASES["e_disabled"] = _case("l4", (0, 2, 3), normalize=False, factor=0.7)
# (f) a group of one member: std is NaN, and so is everything after the division
CASES["f_nan_batch_1"] = _case("l1", (0,), all_nan=True)
# (g) what torch refuses
CASES["g_repeated"] = _case("l4", (1, 1), error="RuntimeError")
CASES["g_repeated_negative"] = _case("l4", (1, -3), error="RuntimeError")
CASES["g_std_repeated"] = _case("l4", (0,), (2, 2), error="RuntimeError")
CASES["g_out_of_range"] = _case("l4", (4,), error="IndexError")
CASES["g_out_of_range_negative"] = _case("l4", (0,), (-5,), error="IndexError")


def planted(torch, latent):
    """The stored noise of a latent: unit normals, stretched and shifted so that no group's mean or std is near zero."""
    import zlib

    g = torch.Generator().manual_seed(zlib.crc32(latent.encode()))
    return torch.randn(LATENTS[latent], generator=g) * 1.5 + 0.4


def item_kwargs(case):
    """The keywords of NormalizeToScaleNoise (the factor goes first, the inner chain as ``noise``)."""
    return dict(RANGE, mode=case["mode"], dims=case["dims"], mean_dims=case["mean_dims"], std_dims=case["std_dims"],
                mean_multiplier=case["mean_multiplier"], std_multiplier=case["std_multiplier"], normalize=case["normalize"], normalize_noise=False)
