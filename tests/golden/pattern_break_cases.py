"""The cases of tests/golden/pattern_break*.npz: shared by the generator (make_pattern_break_golden.py, which runs the reference) and by the
tests (which read only the files).  Plain data, no imports.

A function case is (name, input, percentage, detail_level, restore_scale, blend mode).  The full cross of 3 percentages x 3 detail
levels x 2 x 3 modes is taken on the smallest input with the percentage cycling (every pair of values of two parameters occurs); the other
inputs take a few combinations each, so that every parameter value meets every input kind at least once where it matters."""

SEED = 20260

# input name -> (shape, kind); "gauss": torch.randn under Generator(SEED + index in this table)
INPUTS = {
    "g256": ((1, 4, 8, 8), "gauss"),             # below one 16-byte group per lane of a workgroup
    "g4488": ((2, 4, 33, 17), "gauss"),          # odd tails, rows that start off a 16-byte boundary
    "g64k": ((1, 16, 64, 64), "gauss"),          # the launch-bound latent: sixteen 16-byte groups per lane of the one-launch route
    "g83k": ((3, 4, 96, 72), "gauss"),           # many blocks
    "g5d": ((1, 4, 3, 16, 16), "gauss"),         # 5-D
    "scaled": ((2, 4, 33, 17), "scaled"),        # g4488 * 37.5 + 3: another magnitude
    "extremes": ((2, 4, 8, 8), "extremes"),      # the minimum and the maximum three times each, +0.0 and -0.0
    "const": ((1, 4, 8, 8), "const"),            # every value 1.25: the denominator is eps
    "single": ((1, 1, 1, 1), "single"),          # one value
}
# the inputs stored in files of their own (a file stays below 1 MiB): input name -> file stem
LARGE = {"g64k": "pattern_break_64k", "g83k": "pattern_break_83k"}

PERCENTAGES = (0.25, 0.5, 1.0)
DETAIL_LEVELS = (0.0, 3.5, -4.0)
MODES = ("lerp", "inject", "subtract_b")


def _name(inp, p, d, r, m):
    return f"{inp}_p{p}_d{d}_{'restore' if r else 'raw'}_{m}"


def function_cases():
    out = []
    k = 0
    for d in DETAIL_LEVELS:
        for r in (True, False):
            for m in MODES:
                out.append(("g256", PERCENTAGES[(k + k // 3) % 3], d, r, m))
                k += 1
    out += [
        ("g4488", 0.5, 0.0, True, "lerp"), ("g4488", 0.25, 3.5, False, "lerp"), ("g4488", 1.0, -4.0, True, "inject"),
        ("g4488", 0.5, 3.5, True, "subtract_b"), ("g4488", 0.25, 0.0, False, "inject"), ("g4488", 1.0, 0.0, False, "subtract_b"),
        ("g64k", 0.5, 0.0, True, "lerp"), ("g64k", 0.25, 3.5, False, "inject"),
        ("g83k", 0.5, 0.0, True, "lerp"), ("g83k", 1.0, -4.0, False, "subtract_b"),
        ("g5d", 0.5, 0.0, True, "lerp"), ("g5d", 1.0, 3.5, False, "lerp"), ("g5d", 0.25, -4.0, True, "subtract_b"),
        ("scaled", 0.5, 0.0, True, "lerp"), ("scaled", 0.25, 3.5, False, "inject"), ("scaled", 1.0, -4.0, True, "subtract_b"),
        ("extremes", 0.5, 0.0, True, "lerp"), ("extremes", 1.0, 3.5, False, "lerp"), ("extremes", 0.25, -4.0, True, "inject"),
        ("const", 0.5, 0.0, True, "lerp"), ("const", 0.5, 0.0, False, "lerp"), ("const", 0.25, 3.5, False, "inject"),
        ("single", 0.5, 0.0, True, "lerp"), ("single", 1.0, 3.5, False, "subtract_b"),
    ]
    return [(_name(*c), *c) for c in out]


# the item over a chain of one gaussian item in replay mode (cpu=True: the inner values equal the reference's bit for bit)
ITEM_LATENT = (2, 4, 10, 14)
ITEM_SIGMAS = ((10.0, 5.0), (5.0, 2.0), (2.0, 1.0))
ITEM_SEED, ITEM_GLOBAL_SEED, SIGMA_MIN, SIGMA_MAX = 42, 7, 0.1, 10.0
# name -> (factor, normalized, item parameters)
ITEMS = {
    "norm_f1": (1.0, True, dict(detail_level=0.0, percentage=0.5, restore_scale=True, blend_mode="lerp")),
    "norm_f07": (0.7, True, dict(detail_level=3.5, percentage=0.25, restore_scale=False, blend_mode="inject")),
    "raw_f1": (1.0, False, dict(detail_level=-4.0, percentage=1.0, restore_scale=True, blend_mode="subtract_b")),
    "raw_f07": (0.7, False, dict(detail_level=0.0, percentage=0.5, restore_scale=True, blend_mode="lerp")),
    "pass_through": (0.7, True, dict(detail_level=0.0, percentage=0.0, restore_scale=True, blend_mode="lerp")),
}
