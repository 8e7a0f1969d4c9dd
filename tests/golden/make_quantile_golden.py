"""Generates tests/golden/quantile_filter.npz by running the REAL reference's utils.quantile_normalize (imported through
oracle/ref_import.py) in the build container: inputs, outputs, and the exception type of every refusal.

    python tests/golden/make_quantile_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "quantile_filter.npz")
ref = load_reference()
qn = ref.utils.quantile_normalize
STRATEGIES = tuple(ref.utils.quantile_handlers.keys())
FOCUS = ("clamp", "scale_down", "mean", "median", "mode_1dec", "replace_3pt_flip_keepsign", "sigmoid_outliers")


def inputs():
    g = torch.Generator().manual_seed(1234)
    out = {"base": torch.randn(2, 4, 10, 14, generator=g), "video": torch.randn(1, 4, 3, 8, 6, generator=g)}
    # ties and exact zeros: half-integer steps, a quarter of the values zero
    t = torch.round(torch.randn(2, 4, 10, 14, generator=g) * 2) / 2
    t[torch.rand(t.shape, generator=g) < 0.25] = 0
    out["ties"] = t
    # one value far below the rest: at q = 0 it is the only in-range value (replace with one candidate)
    s = torch.randn(2, 3, 6, 5, generator=g).sign() * (torch.rand(2, 3, 6, 5, generator=g) + 1.0)
    s[1, 2, 3, 4] = 0.01
    out["single"] = s
    return out


SEQ_SIGMAS = ((10.0, 5.0), (5.0, 2.0), (2.0, 1.0))
SEQ_CASES = {"clamp_dim1": dict(quantile=0.85, norm_dim=1, norm_flatten=True, norm_pow=0.5, norm_fac=1.0, strategy="clamp"),
             "median_centered": dict(quantile=-0.7, norm_dim=2, norm_flatten=False, norm_pow=0.75, norm_fac=1.3, strategy="median"),
             "replace_global": dict(quantile=0.6, norm_dim=None, norm_flatten=False, norm_pow=1.0, norm_fac=1.0, strategy="replace_2pt_flip")}


def sequences(arrays, meta):
    """QuantileFilteredNoise over a gaussian + perlin chain: three seeded cpu=True calls of a clone.  The chain's own draws for the same
    seed are stored too (the device path draws its own streams; the test feeds these draws to the item instead)."""
    chain = ref.noise.CustomNoiseChain()
    chain.add(ref.noise.CustomNoiseItem(1.0, noise_type="gaussian"))
    chain.add(ref.noise.CustomNoiseItem(0.5, noise_type="perlin"))
    x = torch.zeros(2, 4, 16, 12)
    for name, kw in SEQ_CASES.items():
        item = ref.noise.QuantileFilteredNoise(0.8, noise=chain, normalize=True, normalize_noise=False, **kw).clone()
        torch.manual_seed(7)  # the chain also draws from the global generator
        ns = item.make_noise_sampler(x, 0.1, 10.0, seed=42, cpu=True, normalized=True)
        outs = [ns(torch.tensor(s), torch.tensor(sn)) for s, sn in SEQ_SIGMAS]
        torch.manual_seed(7)
        raw_ns = chain.make_noise_sampler(x, sigma_min=0.1, sigma_max=10.0, seed=42, cpu=True, normalized=False)
        raws = [raw_ns(torch.tensor(s), torch.tensor(sn)) for s, sn in SEQ_SIGMAS]
        for raw, out in zip(raws, outs):  # the item is the filter and the scaling of exactly these draws
            filt = qn(raw.clone(), quantile=kw["quantile"], dim=kw["norm_dim"], flatten=kw["norm_flatten"], nq_fac=kw["norm_fac"],
                      pow_fac=kw["norm_pow"], strategy=kw["strategy"])
            assert torch.equal(ref.utils.scale_noise(filt, 0.8, normalized=True), out), name
        arrays[f"seq_{name}_raw"] = torch.stack(raws).numpy()
        arrays[f"seq_{name}_out"] = torch.stack(outs).numpy()
        meta[f"seq_{name}"] = {"sequence": kw, "factor": 0.8, "sigmas": SEQ_SIGMAS, "error": None}


def latent_op(ins, arrays, meta):
    """The quantile latent operation (built as the reference's node builds it) inside SonarLatentOperationAdvanced."""
    lo = ref.latent_ops
    kw = dict(quantile=-0.6, dim=1, flatten=False, nq_fac=1.2, pow_fac=0.75, strategy="sigmoid_outliers")
    qop = lo.SonarLatentOperation(op=lambda latent: qn(latent, **kw))
    adv = lo.SonarLatentOperationAdvanced(ops=(qop,), start_sigma=10.0, end_sigma=1.0, blend_mode="lerp", blend_strength=0.7,
                                          input_multiplier=1.2, output_multiplier=1.0, difference_multiplier=0.9)
    arrays["advop_out"] = adv(ins["base"].clone(), sigma=torch.tensor([5.0])).numpy()
    meta["advop"] = {"latent_op": kw, "error": None}


def main():
    ins = inputs()
    arrays = {f"in_{k}": v.numpy() for k, v in ins.items()}
    meta = {}

    def case(name, inp, **kw):
        assert name not in meta, name
        entry = {"input": inp, "kwargs": kw, "error": None}
        try:
            arrays[f"out_{name}"] = qn(ins[inp].clone(), **kw).numpy()
        except Exception as exc:  # noqa: BLE001  (the refusal is the expected result)
            entry["error"] = type(exc).__name__
            entry["message"] = str(exc)[:200]
        meta[name] = entry

    for s in STRATEGIES:
        for q in (0.85, -0.7):
            case(f"all_{s}_q{q}", "base", quantile=q, dim=1, flatten=True, strategy=s)
    for s in FOCUS:
        for dim in (None, 0, 1, 2, 3, 4):
            for flatten in (True, False):
                case(f"dims_{s}_{dim}_{flatten}", "base", quantile=0.8, dim=dim, flatten=flatten, strategy=s)
        for dim in (1, 2):
            for flatten in (True, False):
                case(f"video_{s}_{dim}_{flatten}", "video", quantile=-0.6, dim=dim, flatten=flatten, strategy=s)
        for inp in ("ties", "single"):
            case(f"{inp}_{s}", inp, quantile=0.7, dim=1, flatten=True, strategy=s)
            case(f"{inp}_{s}_q0", inp, quantile=0.0, dim=0, flatten=True, strategy=s)
    for pf in (0.0, 1.0, 0.5, -0.25, 2.0):
        for s in ("clamp", "tanh", "replace_2pt"):
            case(f"pow_{s}_{pf}", "base", quantile=0.75, pow_fac=pf, strategy=s)
    for s in ("clamp", "median", "cos_wrong_keepsign", "replace_3pt_avoidsign"):
        case(f"nqfac_{s}", "base", quantile=0.6, nq_fac=1.7, strategy=s)
        case(f"list_{s}", "base", quantile=[0.9, 0.6], strategy=s)
        case(f"zeroq_{s}", "base", quantile=0.0, strategy=s)
    # no value in range: q = 0 with nq_fac < 1 (the reference divides by zero)
    case("empty_replace", "single", quantile=0.0, nq_fac=0.5, dim=0, strategy="replace")
    case("unknown_strategy", "base", strategy="no_such_strategy")
    sequences(arrays, meta)
    latent_op(ins, arrays, meta)
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
