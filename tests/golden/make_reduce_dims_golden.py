"""Generates tests/golden/reduce_dims.npz by running the REAL reference (imported through oracle/ref_import.py) in the build container, on
the CPU in replay mode, over the tables of tests/golden/reduce_dims_cases.py:

  draw_<latent>      the base draw of the latent
  pre_<latent>_...   the reference's power-law noise on it without div_max_dims: its own float32 pow (reduce_dims_cases.pre_key)
  pl_<case>          the reference's power-law noise (get_noise_sampler("grey", ..., alpha, div_max_dims, use_sign, use_div_max_abs)) on it
  sn_<case>          the reference's scale_noise(x, factor, normalized=True, normalize_dims=dims) of x = draw (+ the per-group offsets)
  flags_<case>       per group of an offset case, in the flattened keepdim order: 1 where |mean of x| is above 2.5 / sqrt(members)

    python tests/golden/make_reduce_dims_golden.py

What the script asserts while it writes:
  * the stored draw is what a sampler draws after torch.manual_seed(SEED);
  * the power-law output is the reference's own pre-division tensor divided by its amax over the tuple, bit for bit (amax and a true
    division are exact, so the only inexact step of a case is the pow the pre-division tensor records; torch's CPU pow is not the same on
    every machine, which is why it is stored and not recomputed by the tests);
  * the reference's float32 scale_noise lies within the node sweep's bound of its own float64 run (atol = 2e-6 * max|want| + 2e-6, rtol 0:
    tests/test_gpu_group_stats.py), the bound the device route is then held to against the float32 output;
  * every offset case has groups on both sides of the mean threshold, and the reference centres both kinds alike: with normalize_dims
    it skips nothing (py/utils.py:96-99 has no threshold), so the output's group means are all zero to rounding."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import reduce_dims_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "reduce_dims.npz")
ref = load_reference()


def powerlaw(case, divide=True):
    shape = cases.SHAPES[case["latent"]]
    torch.manual_seed(cases.SEED)
    ns = ref.noise.get_noise_sampler("grey", torch.zeros(shape), 0.03, 14.6, seed=cases.SEED, cpu=True, factor=1.0, normalized=False,
                                     alpha=case["alpha"], div_max_dims=cases.DIMS[case["latent"]][case["dims"]] if divide else None,
                                     use_sign=case["use_sign"], use_div_max_abs=case["use_div_max_abs"])
    return ns(torch.tensor(cases.SIGMA[0]), torch.tensor(cases.SIGMA[1])).clone()


def scale_input(case, dtype=torch.float32):
    x = cases.draw(torch, case["latent"])
    if case["offset"]:
        x = x + cases.offsets(torch, case["latent"], case["dims"])
    return x.to(dtype)


def main():
    arrays, meta = {}, {}
    for latent, shape in cases.SHAPES.items():
        d = cases.draw(torch, latent)
        torch.manual_seed(cases.SEED)
        assert torch.equal(d, torch.randn(shape)), latent
        arrays[f"draw_{latent}"] = d.numpy()
    for name, case in cases.POWERLAW.items():
        out = powerlaw(case)
        dims = tuple(cases.DIMS[case["latent"]][case["dims"]])
        pre = powerlaw(case, divide=False)
        if cases.pre_key(case) in arrays:
            assert torch.equal(pre, torch.from_numpy(arrays[cases.pre_key(case)])), name
        arrays[cases.pre_key(case)] = pre.numpy()
        want = pre / torch.amax(pre.abs() if case["use_div_max_abs"] else pre, dim=dims, keepdim=True)
        assert out.dtype == torch.float32 and torch.equal(out, want) and bool(out.isfinite().all()), name
        arrays[f"pl_{name}"] = out.numpy()
        meta[f"pl_{name}"] = dict(case, dims=list(dims))
    worst = 0.0
    for name, case in cases.SCALE.items():
        dims = cases.DIMS[case["latent"]][case["dims"]]
        x = scale_input(case)
        out = ref.utils.scale_noise(x.clone(), case["factor"], normalized=True, normalize_dims=dims)
        exact = ref.utils.scale_noise(scale_input(case, torch.float64), case["factor"], normalized=True, normalize_dims=dims)
        members = x.numel() // cases.SEGMENTS[(case["latent"], case["dims"])][2]
        entry = dict(case, dims=list(dims), members=members, all_nan=members == 1)
        if members == 1:  # the std of one member
            assert bool(out.isnan().all()) and bool(exact.isnan().all()), name
        else:
            bound = 2e-6 * float(exact.abs().max()) + 2e-6
            err = float((out.double() - exact).abs().max())
            assert err <= bound, (name, err, bound)
            worst = max(worst, err / bound)
            entry.update(reference_fp32_error=err, bound=bound)
            if case["offset"]:
                flags = x.double().mean(dim=tuple(dims), keepdim=True).abs() > 2.5 / math.sqrt(members)
                assert bool(flags.any()) and not bool(flags.all()), f"{name}: every group on one side of the threshold"
                centred = exact.mean(dim=tuple(dims), keepdim=True).abs()
                assert float(centred[flags].max()) < 1e-12 and float(centred[~flags].max()) < 1e-12, f"{name}: the reference skipped a group"
                arrays[f"flags_{name}"] = flags.flatten().numpy().astype(np.uint8)
        arrays[f"sn_{name}"] = out.numpy()
        meta[f"sn_{name}"] = entry
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    print(f"{os.path.basename(OUT)}  {len(cases.POWERLAW)} + {len(cases.SCALE)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB  "
          f"reference fp32 scale_noise error at most {worst:.2f} of the bound")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
