"""Generates tests/golden/noise_params.npz by running the REAL reference's CustomNoiseParametersNoise (imported through
oracle/ref_import.py) in the build container, on the CPU in replay mode (cpu=True): per case of tests/golden/noise_params_cases.py the
stored planes of a planted base, the two outputs, and for group g the caller's next four host draws after each call.

    python tests/golden/make_noise_params_golden.py

Every case is also run with normalisation off and factor 1 -- that is the tensor scale_noise sees -- and the script asserts that its
|mean| and |1 - std| are at least 20 % away from the threshold 2.5 / sqrt(numel): no decision of the file sits on a knife edge, and both
sides of both thresholds occur among the normalised cases.
"""
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

import noise_params_cases as cases  # noqa: E402
from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(HERE, "noise_params.npz")
ref = load_reference()


class PlantedNoise(ref.noise.CustomNoiseItemBase):
    """Hands back the stored planes, one per call, in the dtype and on the device of the latent it was built for."""

    def make_noise_sampler(self, x, *args, **kwargs):
        planes, state = self.planes, {"i": 0}

        def noise_sampler(_s, _sn):
            out = planes[state["i"] % planes.shape[0]].to(device=x.device, dtype=x.dtype, copy=True)
            state["i"] += 1
            assert out.shape == x.shape, (out.shape, x.shape)
            return out

        return noise_sampler


def ordered_bits(t):
    """16-bit floats as integers in value order: neighbours differ by one."""
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, 0x8000 - b, b)


def build(case, planes, **override):
    chain = ref.noise.CustomNoiseChain()
    if case["base"] == "gaussian":
        chain.add(ref.noise.CustomNoiseItem(1.0, noise_type="gaussian"))
    else:
        chain.add(PlantedNoise(1.0, planes=planes))
    kw = dict(case["kw"]) | override
    factor = kw.pop("factor", case["factor"])
    if kw["override_dtype"] is not None:
        kw["override_dtype"] = getattr(torch, kw["override_dtype"])
    return ref.noise.CustomNoiseParametersNoise(factor, noise=chain, **kw).clone()


def run(case, planes, **override):
    item = build(case, planes, **override)
    x = torch.zeros(case["shape"], dtype=getattr(torch, case["dtype"]))
    torch.manual_seed(case["seed"])
    ns = item.make_noise_sampler(x, 0.03, 14.6, seed=case["seed"], cpu=True, normalized=True)
    outs, after = [], []
    for s, sn in cases.SIGMAS:
        outs.append(ns(torch.tensor(s), torch.tensor(sn)).clone())
        after.append(torch.randn(4))
    return torch.stack(outs), torch.stack(after)


def run_composed(case, **override):
    """A gaussian-base case the reference's item refuses (a 3-D latent with the square option: its crop flattens one dimension of the
    two-dimensional squared plane and the reshape back fails), put together from the reference's own parts in the item's order: the
    chain's draws on the squared latent, each plane flattened and cut to its first h * w values, scale_noise."""
    kw = dict(case["kw"]) | override
    factor = kw.pop("factor", case["factor"])
    assert case["base"] == "gaussian" and kw["rng_mode"] == "default" and not kw["fix_invalid"] and kw["override_dtype"] is None
    chain = ref.noise.CustomNoiseChain()
    chain.add(ref.noise.CustomNoiseItem(1.0, noise_type="gaussian"))
    inner = cases.inner_shape(case)
    keep = math.prod(case["shape"]) // math.prod(inner[:-2])
    torch.manual_seed(case["seed"])
    ns = chain.make_noise_sampler(torch.zeros(inner), 0.03, 14.6, seed=case["seed"], cpu=True, normalized=False)
    outs = []
    for s, sn in cases.SIGMAS:
        noise = ns(torch.tensor(s), torch.tensor(sn)).flatten(start_dim=-2)[..., :keep].reshape(case["shape"]).clone()
        normalize = True if kw["normalize"] is None else kw["normalize"]
        outs.append(ref.utils.scale_noise(noise, factor, normalized=normalize).clone())
        torch.randn(4)  # the caller's draws between calls, as in run()
    return torch.stack(outs)


def main():
    arrays, meta, bad = {}, {}, []
    sides = {"mean_above": 0, "mean_below": 0, "std_above": 0, "std_below": 0}
    for name, case in cases.CASES.items():
        planes = None
        if case["base"].startswith("planted:"):
            planes = cases.planted(torch, case["base"][8:], cases.inner_shape(case))
            arrays[f"planes_{name}"] = planes.numpy()
        error = None
        try:
            outs, after = run(case, planes)
            pre, _ = run(case, planes, normalize=False, factor=1.0)
        except RuntimeError as exc:
            error = {"type": type(exc).__name__, "message": str(exc)[:200]}
            outs, pre, after = run_composed(case), run_composed(case, normalize=False, factor=1.0), None
        ulps = None
        if case["compare"] == "float64_rounded":
            # the reference's own scale_noise in float64 on the tensor its item hands it (``pre``), rounded to the latent's dtype
            normalize = True if case["kw"]["normalize"] is None else case["kw"]["normalize"]
            exact = torch.stack([ref.utils.scale_noise(t.double().clone(), case["factor"], normalized=normalize) for t in pre]).to(outs.dtype)
            ulps = int((ordered_bits(outs) - ordered_bits(exact)).abs().max())  # how far the reference's half-precision arithmetic is from it
            outs = exact
        assert outs.dtype == getattr(torch, case["dtype"]) and tuple(outs.shape[1:]) == case["shape"], name
        normalised = case["kw"]["normalize"] is not False
        for t in pre.double():
            thr = 2.5 / math.sqrt(t.numel())
            mean, std = abs(float(t.mean())), abs(1.0 - float(t.std()))
            if not (abs(mean - thr) >= 0.2 * thr and abs(std - thr) >= 0.2 * thr):
                bad.append((name, case["seed"], round(mean, 4), round(std, 4), round(thr, 4)))
            if normalised:
                sides["mean_above" if mean > thr else "mean_below"] += 1
                sides["std_above" if std > thr else "std_below"] += 1
        arrays[f"out_{name}"] = outs.float().numpy()  # (bfloat16 has no numpy dtype: its values are exact in float32)
        if name.startswith("g_"):
            arrays[f"after_{name}"] = after.numpy()
        meta[name] = {"shape": list(case["shape"]), "dtype": case["dtype"], "base": case["base"], "factor": case["factor"], "seed": case["seed"],
                      "kw": case["kw"], "reference_error": error, "compare": case["compare"], "reference_ulps": ulps}
    assert not bad, f"cases on a knife edge (choose other seeds / offsets): {bad}"
    assert all(sides.values()), sides
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB  sides {sides}")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
