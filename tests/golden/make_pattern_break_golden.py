"""Generates tests/golden/pattern_break.npz (and one file per input of pattern_break_cases.LARGE, to keep every file below 1 MiB) by
running the REAL reference's utils.pattern_break and noise.PatternBreakNoise (imported through oracle/ref_import.py) on the CPU in the
build container: inputs and outputs.

    python tests/golden/make_pattern_break_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import pattern_break_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

ref = load_reference()


def make_input(name):
    shape, kind = cases.INPUTS[name]
    idx = list(cases.INPUTS).index(name)
    if kind == "scaled":
        return make_input("g4488") * 37.5 + 3
    if kind == "const":
        return torch.full(shape, 1.25)
    if kind == "single":
        return torch.full(shape, 0.7)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(cases.SEED + idx))
    if kind == "extremes":
        f = x.flatten()
        lo, hi = f.min().item(), f.max().item()
        f[[3, 200, 511]] = lo
        f[[0, 64, 300]] = hi
        f[17], f[18] = 0.0, -0.0
    return x


def save(stem, arrays):
    path = os.path.join(HERE, stem + ".npz")
    with open(path, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    size = os.path.getsize(path)
    assert size < 1 << 20, (stem, size)
    print(f"{stem}.npz  {len(arrays)} arrays  {size / 1024:.1f} KiB")


def main():
    files = {"pattern_break": {}}
    for stem in cases.LARGE.values():
        files[stem] = {}
    inputs = {name: make_input(name) for name in cases.INPUTS}
    for name, x in inputs.items():
        files[cases.LARGE.get(name, "pattern_break")][f"in_{name}"] = x.numpy()
    for name, inp, p, d, r, m in cases.function_cases():
        x = inputs[inp]
        before = x.clone()
        out = ref.utils.pattern_break(x, percentage=p, detail_level=d, restore_scale=r, blend_function=ref.utils.BLENDING_MODES[m])
        assert out.shape == x.shape and out.dtype == torch.float32 and torch.equal(x, before)
        files[cases.LARGE.get(inp, "pattern_break")][f"out_{name}"] = out.numpy()
    for name, (factor, normalized, kw) in cases.ITEMS.items():
        chain = ref.noise.CustomNoiseChain()
        chain.add(ref.noise.CustomNoiseItem(1.0, noise_type="gaussian"))
        item = ref.noise.PatternBreakNoise(factor, noise=chain, **kw).clone()
        torch.manual_seed(cases.ITEM_GLOBAL_SEED)
        ns = item.make_noise_sampler(torch.zeros(cases.ITEM_LATENT), cases.SIGMA_MIN, cases.SIGMA_MAX, seed=cases.ITEM_SEED, cpu=True,
                                     normalized=normalized)
        files["pattern_break"][f"item_{name}"] = torch.stack([ns(torch.tensor(s), torch.tensor(sn)) for s, sn in cases.ITEM_SIGMAS]).numpy()
    for stem, arrays in files.items():
        save(stem, arrays)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
