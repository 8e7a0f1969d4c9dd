"""Case table of SonarCustomNoiseParameters' golden file (shared by tests/golden/make_noise_params_golden.py, which runs the reference's
item on the CPU, and tests/test_gpu_noise_params.py, which runs the product's on the device): plain data and tensor builders, no item code.

A case is (shape, latent dtype, base, factor, item keywords, seed).  ``base`` "gaussian" is a one-item gaussian chain drawn in replay mode
(cpu=True: the host generator, the same values on both sides).  ``base`` "planted:<name>" is a recording inner item that hands back the
stored planes ``PLANTED[<name>]`` builds, converted to the dtype of the latent it is given: the half-precision cases use it because a
half-precision host draw is not the float32 draw rounded, and the fix_invalid cases because no generator emits NaN on demand.

The bfloat16-latent cases of group f run with normalisation off and factor 1: the reference's scale_noise on a bfloat16 tensor rounds
after every operation, the product computes in float32 and rounds once (its rule for half-precision latents), so with arithmetic the two
differ by a bfloat16 ulp (4e-3), a hundred times the comparison's tolerance; without it the result is the conversion alone, bit for bit.
Normalisation into a bfloat16 latent is pinned by f_norm_bf16_latent and f_norm_bf16_latent_square instead (``compare`` =
"float64_rounded"): their expectation is the reference's scale_noise run in float64 on the bfloat16 tensor the reference's item hands it,
rounded to bfloat16, and the comparison is one bfloat16 ulp -- the bound of the kernel-level half-precision tests (double rounding).  The
golden file's meta also records how far the reference's own bfloat16 arithmetic is from that expectation (``reference_ulps``).
The all-NaN case runs with normalisation off as well: its fixed tensor is all zeros, which scale_noise would divide by a zero std."""

SIGMAS = [(9.0, 6.0), (6.0, 3.5)]
DEFAULTS = dict(rng_state_offset=0, rng_offset_mode="disabled", rng_mode="default", frames_to_channels=False, ensure_square_aspect_ratio=False,
                fix_invalid=False, override_dtype=None, override_device=None, normalize=None)


def _case(shape, base="gaussian", factor=1.0, dtype="float32", seed=0, compare="reference", **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(shape=tuple(shape), base=base, factor=factor, dtype=dtype, seed=seed, compare=compare, kw=DEFAULTS | kw)


CASES = {
    # (a) default sockets
    "a_default": _case((2, 4, 10, 14), seed=301),
    # (b) ensure_square_aspect_ratio: 140 -> 12 x 12, a 3-D latent 77 -> 9 x 9, 144 = 12 x 12 stays 6 x 24
    "b_square_140": _case((2, 4, 10, 14), seed=302, ensure_square_aspect_ratio=True),
    "b_square_3d_77": _case((2, 4, 77), seed=303, ensure_square_aspect_ratio=True),
    "b_square_exact_144": _case((1, 4, 6, 24), seed=304, ensure_square_aspect_ratio=True),
    # (c) frames_to_channels, alone and with the square option (60 -> 8 x 8)
    "c_frames": _case((1, 4, 3, 6, 10), seed=305, frames_to_channels=True),
    "c_frames_square": _case((1, 4, 3, 6, 10), seed=306, factor=0.8, frames_to_channels=True, ensure_square_aspect_ratio=True),
    # (d) fix_invalid over planted planes
    "d_nan": _case((2, 4, 10, 14), base="planted:nan", seed=307, fix_invalid=True),
    "d_inf_positive_part": _case((2, 4, 10, 14), base="planted:inf_positive_part", factor=0.6, seed=308, fix_invalid=True),
    "d_inf_negative_part": _case((2, 4, 10, 14), base="planted:inf_negative_part", seed=309, fix_invalid=True),
    "d_padding_only": _case((2, 4, 10, 14), base="planted:padding_only", seed=310, fix_invalid=True, ensure_square_aspect_ratio=True),
    "d_padding_extremes": _case((2, 4, 10, 14), base="planted:padding_extremes", seed=311, fix_invalid=True, ensure_square_aspect_ratio=True),
    "d_all_nan": _case((2, 4, 10, 14), base="planted:all_nan", factor=0.6, seed=312, fix_invalid=True, normalize=False),
    # (f) override_dtype over planted float32 planes
    "f_f16_on_f32": _case((2, 4, 10, 14), base="planted:plain", factor=0.6, seed=330, override_dtype="float16"),
    "f_bf16_on_f32": _case((2, 4, 10, 14), base="planted:plain", factor=0.6, seed=331, override_dtype="bfloat16", ensure_square_aspect_ratio=True),
    "f_f16_on_bf16": _case((2, 4, 10, 14), base="planted:plain", dtype="bfloat16", seed=332, override_dtype="float16", normalize=False),
    "f_bf16_on_bf16": _case((2, 4, 10, 14), base="planted:plain", dtype="bfloat16", seed=333, override_dtype="bfloat16", normalize=False,
                            ensure_square_aspect_ratio=True),
    "f_norm_bf16_latent": _case((2, 4, 10, 14), base="planted:plain", factor=0.6, dtype="bfloat16", seed=334, compare="float64_rounded"),
    "f_norm_bf16_latent_square": _case((2, 4, 10, 14), base="planted:plain", factor=0.6, dtype="bfloat16", seed=335, compare="float64_rounded",
                                       override_dtype="bfloat16", ensure_square_aspect_ratio=True),
}
# (e) the normalize tristate x factor
_E_SEEDS = iter(range(401, 410))  # (400 puts a mean within 20 % of its threshold)
for _n, _norm in (("default", None), ("forced", True), ("disabled", False)):
    for _f in (1.0, 0.6, -0.3):
        CASES[f"e_{_n}_{_f}"] = _case((2, 4, 10, 14), factor=_f, seed=next(_E_SEEDS), normalize=_norm)
# (g) rng_offset_mode x rng_mode over a gaussian base: two consecutive calls, and the caller's next four host draws after each
_G_SEEDS = iter(range(420, 424))
for _om in ("override", "add"):
    for _rm in ("separate", "fork"):
        CASES[f"g_{_om}_{_rm}"] = _case((2, 4, 10, 14), seed=next(_G_SEEDS), rng_offset_mode=_om, rng_mode=_rm, rng_state_offset=77)


def planted(torch, name, shape):
    """The stored planes (two calls' worth, stacked) of a planted base on the shape the INNER sampler sees.  Offsets and scales are
    chosen so that the mean and std of what reaches scale_noise are far from its thresholds (the golden script asserts 20 %)."""
    import zlib

    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    z = torch.randn((2, *shape), generator=g)
    if name == "plain":
        return z * 1.5 + 0.4
    if name == "nan":
        z = z * 0.7 + 0.3
        z.view(2, -1)[:, ::37] = float("nan")
        return z
    if name in ("inf_positive_part", "inf_negative_part"):
        z = z.abs() + 0.5  # every finite value positive: -inf must become 0, not the finite minimum
        flat = z.view(2, -1)
        flat[:, 5::101] = float("inf")
        flat[:, 7::113] = float("-inf")
        flat[:, 11::127] = float("nan")
        return z if name == "inf_positive_part" else -z
    if name in ("padding_only", "padding_extremes"):
        # shape is (..., side, side); the kept part of a plane is its first 140 values, 140 .. 143 are padding
        z = z * 1.4 - 0.5
        planes = z.view(2, -1, shape[-1] * shape[-2])
        planes[:, ::2, 140] = float("nan")
        planes[:, 1::3, 141] = float("inf")
        planes[:, ::5, 143] = float("-inf")
        if name == "padding_extremes":  # the finite extremes live in the padding, non-finite values in the kept part take them
            planes[:, 3, 142] = 50.0
            planes[:, 5, 142] = -40.0
            planes[:, :, 17] = float("inf")
            planes[:, ::2, 90] = float("-inf")
        return z
    if name == "all_nan":
        return torch.full_like(z, float("nan"))
    raise KeyError(name)


def inner_shape(case):
    """The shape the inner sampler is asked for (frames folded, plane squared)."""
    import math

    shape = list(case["shape"])
    kw = case["kw"]
    if len(shape) == 5 and kw["frames_to_channels"]:
        shape = [shape[0], shape[1] * shape[2], *shape[3:]]
    if kw["ensure_square_aspect_ratio"]:
        spat = 1 if len(shape) == 3 else 2
        n = math.prod(shape[-spat:])
        hw = n ** 0.5
        if not hw.is_integer():
            side = math.ceil(hw)
            shape = [*shape[:-spat], side, side]
    return tuple(shape)
