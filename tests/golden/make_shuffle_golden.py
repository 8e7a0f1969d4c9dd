"""Generates tests/golden/shuffle.npz by running the REAL reference's utils.elementwise_shuffle_by_dim and noise.ShuffledNoise (imported
through oracle/ref_import.py) on the CPU in the build container: inputs, outputs, and four uniforms drawn from the same generator right
after each call (the generator's position: a port that skips or adds a draw gets other values).

    python tests/golden/make_shuffle_golden.py

The reference function takes ``dim >= 0`` only (its ``orig_shape[dim + 1:]`` is the whole shape at -1), as its one caller, the item,
normalises the dimension first; the cases written with a negative dim are run at the normalised one.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import shuffle_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "shuffle.npz")
ref = load_reference()
shuffle = ref.utils.elementwise_shuffle_by_dim


def planted(shape, dtype=torch.float32):
    """Distinct values: a wrong index cannot hide behind equal ones."""
    return torch.arange(int(np.prod(shape)), dtype=dtype).reshape(shape)


def run(t, dim, prob, no_identity, rng):
    if rng == "gen":
        gen = torch.Generator().manual_seed(cases.SEED)
    else:
        gen = None
        torch.manual_seed(cases.SEED)
    out = shuffle(t, dim=dim % t.ndim, prob=prob, no_identity=no_identity, generator=gen)
    return out, torch.rand(4, generator=gen)


def main():
    arrays, meta = {}, {}
    for shape in sorted({s for s, _d in cases.LAYOUTS}):
        arrays[f"in_{'x'.join(map(str, shape))}"] = planted(shape).numpy()
    for name, shape, dim, prob, no_identity, rng in cases.replay_cases():
        out, after = run(planted(shape), dim, prob, no_identity, rng)
        assert out.shape == tuple(shape) and torch.equal(out.flatten().sort().values, planted(shape).flatten())
        arrays[f"out_{name}"], arrays[f"next_{name}"] = out.numpy(), after.numpy()
        meta[name] = dict(shape=shape, dim=dim, prob=prob, no_identity=no_identity, rng=rng)
    shape, dim, prob, no_identity = cases.HALF_CASE
    out, after = run(planted(shape, torch.float16), dim, prob, no_identity, "global")
    assert out.dtype == torch.float16
    arrays["out_half"], arrays["next_half"] = out.numpy(), after.numpy()

    it = cases.ITEM
    chain = ref.noise.CustomNoiseChain()
    chain.add(ref.noise.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = ref.noise.ShuffledNoise(it["factor"], noise=chain, dims=it["dims"], percentages=it["percentages"], no_identity=it["no_identity"],
                                   fork_rng=it["fork_rng"]).clone()
    torch.manual_seed(it["global_seed"])
    ns = item.make_noise_sampler(torch.zeros(it["latent"]), it["sigma_min"], it["sigma_max"], seed=it["seed"], cpu=True, normalized=True)
    arrays["item_out"] = torch.stack([ns(torch.tensor(s), torch.tensor(sn)) for s, sn in it["sigmas"]]).numpy()
    arrays["item_next"] = torch.rand(4).numpy()
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
