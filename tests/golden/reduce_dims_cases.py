"""The case tables of tests/golden/reduce_dims.npz (make_reduce_dims_golden.py writes it from the reference on the CPU;
tests/test_reduce_dims_cpu.py and tests/test_gpu_reduce_dims.py read it): plain data and two helpers, no reference code.

Shapes and dims (every way a strided reduction can go wrong, at sizes that keep the file small):
  s4   (3, 5, 6, 7)       (0, 2) (1, 3) (0, 3) (0, 2, 3), [0, 2] as a list, (-4, -2): three and four segments, either kind innermost
  s5   (2, 3, 4, 5, 6)    (1, 3) and (0, 2, 4): five segments, the latter starting and ending reduced
  s6   (2, 3, 2, 3, 2, 3) (0, 2, 4): six segments, the most the kernels take
  one  (1, 4, 1, 9)       (0, 2): the reduced extents are 1, every element is its own group
  big  (2, 2, 65, 130)    (0, 2) and (1, 3): kept and reduced extents either side of a wave (64) and a workgroup (256); (0, 2) has the
                          contiguous W kept (a lane per group), (1, 3) has it reduced (a wave per group)"""

SEED = 77
SIGMA = (14.6, 10.0)
SHAPES = {"s4": (3, 5, 6, 7), "s5": (2, 3, 4, 5, 6), "s6": (2, 3, 2, 3, 2, 3), "one": (1, 4, 1, 9), "big": (2, 2, 65, 130)}
DIMS = {
    "s4": {"02": (0, 2), "13": (1, 3), "03": (0, 3), "023": (0, 2, 3), "list02": [0, 2], "neg": (-4, -2)},
    "s5": {"13": (1, 3), "024": (0, 2, 4)},
    "s6": {"024": (0, 2, 4)},
    "one": {"02": (0, 2)},
    "big": {"02": (0, 2), "13": (1, 3)},
}
# what the host hands the kernels for each of them: (segment sizes, first_reduced, groups)
SEGMENTS = {
    ("s4", "02"): ([3, 5, 6, 7], 1, 35), ("s4", "13"): ([3, 5, 6, 7], 0, 18), ("s4", "03"): ([3, 30, 7], 1, 30),
    ("s4", "023"): ([3, 5, 42], 1, 5), ("s4", "list02"): ([3, 5, 6, 7], 1, 35), ("s4", "neg"): ([3, 5, 6, 7], 1, 35),
    ("s5", "13"): ([2, 3, 4, 5, 6], 0, 48), ("s5", "024"): ([2, 3, 4, 5, 6], 1, 15),
    ("s6", "024"): ([2, 3, 2, 3, 2, 3], 1, 27),
    ("one", "02"): ([36], 0, 36),
    ("big", "02"): ([2, 2, 65, 130], 1, 260), ("big", "13"): ([2, 2, 65, 130], 0, 130),
}
VARIANTS = {  # (alpha, use_sign, use_div_max_abs)
    "a2": (2.0, False, True), "a2_sign": (2.0, True, True), "a2_noabs": (2.0, False, False), "a2_sign_noabs": (2.0, True, False),
    "a05": (0.5, False, True), "a05_sign": (0.5, True, True), "a05_noabs": (0.5, False, False), "a05_sign_noabs": (0.5, True, False),
}


def _powerlaw_cases():
    out = {}
    for latent, table in DIMS.items():
        for key in table:
            if (latent, key) == ("s4", "02"):
                names = list(VARIANTS)  # every combination once
            elif latent == "big":
                names = ["a05_sign_noabs"] if key == "02" else ["a05_sign"]  # (this shape is most of the file: one pre-division tensor)
            else:
                names = ["a2_noabs", "a05_sign"]
            for v in names:
                alpha, use_sign, use_abs = VARIANTS[v]
                out[f"{latent}_{key}_{v}"] = dict(latent=latent, dims=key, alpha=alpha, use_sign=use_sign, use_div_max_abs=use_abs)
    return out


def _scale_cases():
    out = {}
    for latent, table in DIMS.items():
        for key in table:
            if latent == "big":
                combos = [(1.0, True)] if key == "02" else [(0.35, True)]
            else:
                combos = [(1.0, False), (0.35, True)]
            for factor, offset in combos:
                out[f"{latent}_{key}_f{int(factor * 100)}_{'offset' if offset else 'plain'}"] = dict(latent=latent, dims=key, factor=factor,
                                                                                                 offset=offset)
    return out


def pre_key(case):
    """The fixture's name for the reference's tensor before the division: it depends on the latent, alpha and use_sign alone."""
    return f"pre_{case['latent']}_a{int(case['alpha'] * 10):02d}_{'sign' if case['use_sign'] else 'plain'}"


POWERLAW = _powerlaw_cases()
SCALE = _scale_cases()


def draw(torch, latent):
    """The base draw of a latent: what a replay-mode sampler built after torch.manual_seed(SEED) draws first."""
    return torch.randn(SHAPES[latent], generator=torch.Generator().manual_seed(SEED))


def offsets(torch, latent, key):
    """One offset per group of (latent, dims), as a keepdim tensor: half of the groups (every other one in the flattened keepdim order) get
    a mean far above scale_noise's skip threshold 2.5 / sqrt(numel), the others none."""
    shape = SHAPES[latent]
    dims = {d % len(shape) for d in DIMS[latent][key]}
    kept = [1 if d in dims else n for d, n in enumerate(shape)]
    groups = 1
    for n in kept:
        groups *= n
    return ((torch.arange(groups) % 2).to(torch.float32) * 1.5).reshape(kept)
