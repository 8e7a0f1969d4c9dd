"""Generates tests/golden/normalize_dims.npz by running the REAL reference's NormalizeToScaleNoise (imported through
oracle/ref_import.py) in the build container, on the CPU, over the stored noise of tests/golden/normalize_dims_cases.py: per latent the
planted tensor, per case the item's output, or the type of the exception torch raises for its dims.

    python tests/golden/make_normalize_dims_golden.py

Every case is also run with the planted tensor (and the latent) cast to float64.  The script asserts that the reference's own float32
output lies within the node sweep's bound of that (atol = 2e-6 * max|want| + 2e-6, rtol = 0, tests/test_gpu_round2.py) -- the bound the
device path is then held to against the float32 output -- that no adjusted std (the divisor of the std step) comes within 1e-3 of zero,
and, for the cases that normalise, that the mean and std scale_noise decides on are at least 20 % away from its threshold."""
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

import normalize_dims_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "normalize_dims.npz")
ref = load_reference()


class PlantedNoise(ref.noise.CustomNoiseItemBase):
    """Hands back the stored tensor in the dtype and on the device of the latent it was built for."""

    def make_noise_sampler(self, x, *args, **kwargs):
        stored = self.planes

        def noise_sampler(_s, _sn):
            assert stored.shape == x.shape, (stored.shape, x.shape)
            return stored.to(device=x.device, dtype=x.dtype, copy=True)

        return noise_sampler


def run(case, planes, dtype, **override):
    chain = ref.noise.CustomNoiseChain()
    chain.add(PlantedNoise(1.0, planes=planes))
    kw = cases.item_kwargs(case) | override
    item = ref.noise.NormalizeToScaleNoise(kw.pop("factor", case["factor"]), noise=chain, **kw).clone()
    x = torch.zeros(cases.LATENTS[case["latent"]], dtype=dtype)
    ns = item.make_noise_sampler(x, 0.03, 14.6, seed=0, cpu=True, normalized=True)
    return ns(torch.tensor(cases.SIGMA[0]), torch.tensor(cases.SIGMA[1])).clone()


def smallest_divisor(case, planes):
    """min |adjusted std| of the case, recomputed in float64 from the tensor the std step sees (the case without that step, unscaled)."""
    if case["std_multiplier"] == 0:
        return math.inf
    pre = run(case, planes, torch.float64, std_multiplier=0.0, normalize=False, factor=1.0)
    adj = (pre.std(dim=case["std_dims"], keepdim=True) - 1.0) * case["std_multiplier"] + 1.0
    return float(adj.abs().min())


def main():
    arrays, meta, bad = {}, {}, []
    for latent in cases.LATENTS:
        arrays[f"planes_{latent}"] = cases.planted(torch, latent).numpy()
    for name, case in cases.CASES.items():
        planes = torch.from_numpy(arrays[f"planes_{case['latent']}"])
        entry = dict(case, shape=list(cases.LATENTS[case["latent"]]), reference_error=None)
        try:
            out = run(case, planes, torch.float32)
        except (RuntimeError, IndexError) as exc:
            entry["reference_error"] = {"type": type(exc).__name__, "message": str(exc)[:200]}
            assert type(exc).__name__ == case["error"], (name, type(exc).__name__, str(exc))
            meta[name] = entry
            continue
        assert case["error"] is None, f"{name}: the reference accepted the dims"
        exact = run(case, planes, torch.float64)
        assert out.dtype == torch.float32 and tuple(out.shape) == cases.LATENTS[case["latent"]], name
        if case["all_nan"]:
            assert bool(out.isnan().all()) and bool(exact.isnan().all()), name
        else:
            assert not bool(out.isnan().any()), name
            bound = 2e-6 * float(exact.abs().max()) + 2e-6
            err = float((out.double() - exact).abs().max())
            entry["reference_fp32_error"], entry["bound"] = err, bound
            if err > bound:
                bad.append((name, "the reference's float32 output misses the bound against float64", err, bound))
            div = smallest_divisor(case, planes)
            if div < 1e-3:
                bad.append((name, "an adjusted std within 1e-3 of zero", div))
            if case["normalize"]:
                pre = run(case, planes, torch.float64, normalize=False, factor=1.0)
                thr = 2.5 / math.sqrt(pre.numel())
                mean, std = abs(float(pre.mean())), abs(1.0 - float(pre.std()))
                if not (abs(mean - thr) >= 0.2 * thr and abs(std - thr) >= 0.2 * thr):
                    bad.append((name, "scale_noise's decision on a knife edge", mean, std, thr))
        arrays[f"out_{name}"] = out.numpy()
        meta[name] = entry
    assert not bad, f"cases to drop or reshape: {bad}"
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    worst = max((m.get("reference_fp32_error", 0.0) / m["bound"] for m in meta.values() if m.get("bound")), default=0.0)
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB  reference fp32 error at most {worst:.2f} of the bound")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
