"""Generates tests/golden/collatz.npz by running the REAL reference's CollatzNoiseGenerator and noise.AdvancedCollatzNoise (imported through
oracle/ref_import.py) on the CPU in the build container.  Per case of collatz_cases.py: every draw the generator took (``draws_``: the
uniforms of the seeds and, in the noise_x_* modes, the normals of the mix noise, flat, in call order), the final output (``out_``), four
uniforms drawn from the same generator right after the call (``next_``: the generator's position) and, for the quantile-off ratios /
mults / adds cases, every iteration's output before its weight (``raw_``).  One item case with a Gaussian seed chain and a mix chain.

    python tests/golden/make_collatz_golden.py
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

import collatz_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "collatz.npz")
ref = load_reference()


def run(params):
    gen = ref.noise_generation.CollatzNoiseGenerator(torch.zeros(cases.LATENT), cpu=True, normalized=False, **params)
    draws, raw = [], []
    rand_like, iteration = gen.rand_like, gen._generate_iteration

    def recording_rand_like(*a, **k):
        t = rand_like(*a, **k)
        draws.append(t.detach().clone().flatten())
        return t

    def recording_iteration(*a, **k):
        t = iteration(*a, **k)
        raw.append(t.detach().clone())
        return t

    gen.rand_like, gen._generate_iteration = recording_rand_like, recording_iteration
    torch.manual_seed(cases.SEED)
    out = gen.generate(torch.tensor(10.0), torch.tensor(5.0))
    return out, torch.rand(4), torch.cat(draws), torch.stack(raw)


def main():
    arrays, meta = {}, {}
    for name, params in cases.cases():
        out, after, draws, raw = run(params)
        assert out.shape == tuple(cases.LATENT) and out.dtype == torch.float32 and bool(torch.isfinite(out).all()), name
        arrays[f"out_{name}"], arrays[f"next_{name}"], arrays[f"draws_{name}"] = out.numpy(), after.numpy(), draws.numpy()
        if cases.is_exact(params) and params["output_mode"] in cases.RAW_MODES:
            arrays[f"raw_{name}"] = raw.numpy()
        meta[name] = {k: list(v) if isinstance(v, tuple) else v for k, v in params.items()}

    it = cases.ITEM
    chains = []
    for _ in range(2):
        chain = ref.noise.CustomNoiseChain()
        chain.add(ref.noise.CustomNoiseItem(1.0, noise_type="gaussian"))
        chains.append(chain)
    params = it["params"] | dict(noise_dtype=torch.float32)
    item = ref.noise.AdvancedCollatzNoise(it["factor"], seed_custom_noise=chains[0], mix_custom_noise=chains[1], **params).clone()
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
