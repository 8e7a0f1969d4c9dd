"""Generates tests/golden/voronoi_rank.npz by running the REAL reference's VoronoiNoiseGenerator (imported through oracle/ref_import.py) on
the CPU in the build container, by the scheme of make_voronoi_golden.py.  Per case of voronoi_rank_cases.py, over three consecutive calls
of one generator: every tensor of uniforms it drew (``draws_``, flat, in call order), the outputs (``out_`` [3, B, C, H, W]), four
uniforms drawn from the same generator right after the last call (``next_``: the generator's position) and z_curr / z_increment after
the last call (``z_``).

    python tests/golden/make_voronoi_rank_golden.py
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

import voronoi_rank_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "voronoi_rank.npz")
ref = load_reference()


def run(latent, params):
    draws, outs, rand = [], [], torch.rand

    def recording_rand(*a, **k):
        t = rand(*a, **k)
        draws.append(t.detach().clone().flatten())
        return t

    torch.manual_seed(cases.SEED)
    gen = ref.noise_generation.VoronoiNoiseGenerator(torch.zeros(latent), cpu=True, normalized=False, **params)
    torch.rand = recording_rand  # the feature points and the fuzz modes' uniforms, in call order
    try:
        for _ in range(cases.CALLS):
            outs.append(gen.generate(torch.tensor(10.0), torch.tensor(5.0)).clone())
    finally:
        torch.rand = rand
    return torch.stack(outs), torch.rand(4), torch.cat(draws), np.array([gen.z_curr, gen.z_increment], np.float64)


def main():
    arrays, meta = {}, {}
    for name, latent, params in cases.cases():
        out, after, draws, z = run(latent, params)
        assert out.shape == (cases.CALLS, *latent) and out.dtype == torch.float32 and bool(torch.isfinite(out).all()), name
        arrays[f"out_{name}"], arrays[f"next_{name}"], arrays[f"draws_{name}"], arrays[f"z_{name}"] = out.numpy(), after.numpy(), draws.numpy(), z
        meta[name] = {"latent": list(latent), "params": {k: list(v) if isinstance(v, tuple) else v for k, v in params.items()}}
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
