"""The cases of tests/golden/shuffle.npz: shared by the generator (make_shuffle_golden.py, which runs the reference) and by
tests/test_gpu_shuffle.py (which reads only the file).  Plain data, no imports."""

# (shape, dim as the caller writes it)
LAYOUTS = (
    ((2, 3, 5, 7), 0), ((2, 3, 5, 7), 1), ((2, 3, 5, 7), 2), ((2, 3, 5, 7), 3),
    ((1, 4, 8, 8), -1),
    ((2, 3, 4, 6, 5), 2),       # 5-D
    ((3, 1, 1, 64), -1),        # a row is one wave
    ((3, 1, 1, 65), -1),        # ... and one lane more
    ((1, 2, 1, 4), 2),          # n == 1: the default path is the identity
)
PROBS = (1.0, 0.5, 0.0)
SEED = 1234          # torch.manual_seed / Generator.manual_seed before every reference call
HALF_CASE = ((2, 3, 5, 7), 3, 1.0, False)  # (shape, dim, prob, no_identity) of the fp16 case

ITEM = dict(latent=(2, 4, 10, 14), dims=(-1, -2), percentages=(1.0, 0.5), no_identity=False, fork_rng=False, factor=0.8,
            global_seed=7, seed=42, sigma_min=0.1, sigma_max=10.0, sigmas=((10.0, 5.0), (5.0, 2.0)))


def case_name(shape, dim, prob, no_identity, rng):
    return f"{'x'.join(map(str, shape))}_d{dim}_p{prob}_{'rot' if no_identity else 'perm'}_{rng}"


def replay_cases():
    """(name, shape, dim, prob, no_identity, rng) -- rng "gen": a torch.Generator seeded with SEED, "global": torch.manual_seed(SEED)."""
    for shape, dim in LAYOUTS:
        n = shape[dim]
        for prob in PROBS:
            for no_identity in (False, True):
                if no_identity and n < 2:
                    continue
                for rng in ("gen", "global"):
                    yield case_name(shape, dim, prob, no_identity, rng), shape, dim, prob, no_identity, rng
