"""Generates tests/golden/image_noise.npz by running the REAL reference's SonarNoiseImage node (imported through oracle/ref_import.py) in the
build container, in replay mode (cpu_noise=True) on float32 images: outputs, the exception type of every refusal, whether the global torch
RNG state and the ``random`` state after each call equal the states before it, and the channel-target table of every channel_mode for 1, 3
and 4 channels (read off the reference's own outputs: the channels a pure-noise call leaves non-zero).

    python tests/golden/make_image_noise_golden.py
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import load_reference  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "image_noise.npz")
ABI = json.load(open(os.path.join(HERE, "node_abi.json")))["SonarNoiseImage"]
ref = load_reference()
NODE = ref.nodes.NODE_CLASS_MAPPINGS["SonarNoiseImage"]
MODES = tuple(ABI["inputs"]["channel_mode"]["type"])
assert len(MODES) == 15

# input images, [0, 1) uniform: name -> NHWC shape (HWC: the unbatched form)
IMAGES = {"b1c4": (1, 9, 14, 4), "b2c3": (2, 9, 14, 3), "b1c1": (1, 16, 16, 1), "hwc3": (9, 14, 3), "b2c3s": (2, 8, 12, 3),
          "b2c4s": (2, 8, 12, 4), "tile3": (1, 33, 70, 3), "tile4": (1, 33, 70, 4), "flat2": (9, 14), "vid5": (1, 2, 9, 14, 3)}
DEFAULTS = dict(noise_type="gaussian", noise_multiplier=0.5, noise_min=0.0, noise_max=1.0, channel_mode="RGB", blend_mode="simple_add",
                blend_strength=0.5, overflow_mode="clamp", greyscale_mode=False, dtype="default", pure_noise_mode=False, cpu_noise=True,
                normalize=True)


def cases():
    out = {}

    def add(name, image, **over):
        assert name not in out, name
        out[name] = dict(image=image, kwargs=over)

    for mode in MODES:
        add(f"c4_{mode}", "b1c4", channel_mode=mode)
    for mode in ("RGB", "G", "BA", "A"):
        add(f"c3_{mode}", "b2c3", channel_mode=mode, blend_mode="lerp", blend_strength=0.3)
    for mode in ("RGB", "R"):
        add(f"c1_{mode}", "b1c1", channel_mode=mode)
    add("c3_A_rescale", "b2c3", channel_mode="A", overflow_mode="rescale")
    add("unbatched", "hwc3")
    for blend, t in (("simple_add", 0.9), ("lerp", 0.3), ("lerp", 0.8), ("inject", 0.7), ("subtract_b", 0.25)):
        for overflow in ("clamp", "rescale"):
            add(f"blend_{blend}_{t}_{overflow}", "b2c3s", blend_mode=blend, blend_strength=t, overflow_mode=overflow, noise_multiplier=0.8)
    for img in ("b2c3s", "b2c4s", "b1c1"):
        for overflow in ("clamp", "rescale"):
            add(f"grey_{img}_{overflow}", img, greyscale_mode=True, overflow_mode=overflow, channel_mode="RGBA", noise_multiplier=1.2)
    add("grey_pure_inject", "b2c4s", greyscale_mode=True, pure_noise_mode=True, blend_mode="inject", blend_strength=0.6, channel_mode="GA")
    for overflow in ("clamp", "rescale"):
        add(f"pure_{overflow}", "b2c3s", pure_noise_mode=True, overflow_mode=overflow, noise_multiplier=1.0)
    add("normalize_off", "b2c3s", normalize=False)
    add("range_equal", "b2c3s", noise_min=0.5, noise_max=0.5, noise_multiplier=0.25)
    add("range_max_zero", "b2c3s", noise_min=-1.0, noise_max=0.0, noise_multiplier=0.25)
    add("range_inverted", "b2c3s", noise_min=1.0, noise_max=0.25)
    add("range_inverted_to_zero", "b2c3s", noise_min=0.0, noise_max=-0.5)
    add("range_inexact", "b2c3s", noise_min=0.1, noise_max=0.3, noise_multiplier=1.0)
    add("range_signed_rescale", "b2c4s", noise_min=-0.5, noise_max=0.5, overflow_mode="rescale")
    add("multiplier_zero", "b2c3s", noise_multiplier=0.0)
    add("multiplier_negative", "b2c3s", noise_multiplier=-0.75)
    add("multiplier_negative_rescale", "b2c3s", noise_multiplier=-0.75, overflow_mode="rescale")
    for typ in ("gaussian", "perlin", "pyramid", "uniform"):
        for overflow in ("clamp", "rescale"):
            add(f"type_{typ}_{overflow}", "b2c4s", noise_type=typ, overflow_mode=overflow, channel_mode="RGBA")
    for img, overflow in (("tile3", "rescale"), ("tile4", "clamp")):
        add(f"{img}_{overflow}", img, overflow_mode=overflow, blend_mode="inject", blend_strength=0.4, channel_mode="RBA")
    add("tile3_grey_rescale", "tile3", overflow_mode="rescale", greyscale_mode=True)
    for overflow in ("clamp", "rescale"):
        add(f"chain_{overflow}", "b2c4s", chain=[[0.6, "gaussian"], [0.4, "perlin"]], overflow_mode=overflow, channel_mode="RGBA")
    add("refuse_2d", "flat2")
    add("refuse_5d", "vid5")
    return out


def run(image, seed, chain=None, **over):
    kw = dict(DEFAULTS, seed=seed, image=image, **over)
    if chain is not None:
        c = ref.noise.CustomNoiseChain()
        for factor, typ in chain:
            c.add(ref.noise.CustomNoiseItem(factor, noise_type=ref.noise.NoiseType[typ.upper()]))
        kw["custom_noise_opt"] = c
    return NODE.go(**kw)[0]


def main():
    arrays, meta = {}, {}
    g = torch.Generator().manual_seed(20250)
    images = {name: torch.rand(shape, generator=g) for name, shape in IMAGES.items()}
    for name, img in images.items():
        arrays[f"image_{name}"] = img.numpy()
    for idx, (name, case) in enumerate(cases().items()):
        seed = 1000 + idx
        entry = dict(case, seed=seed, error=None)
        img = images[case["image"]]
        before_img = img.clone()
        torch.manual_seed(77 + idx)
        random.seed(77 + idx)
        st_torch, st_py = torch.random.get_rng_state(), random.getstate()
        try:
            out = run(img, seed, **case["kwargs"])
            assert out.dtype == torch.float32
            arrays[f"out_{name}"] = out.contiguous().numpy()
        except Exception as exc:  # noqa: BLE001  (the refusal is the expected result)
            entry["error"] = type(exc).__name__
            entry["message"] = str(exc)[:200]
        entry["rng_restored"] = bool(torch.equal(torch.random.get_rng_state(), st_torch) and random.getstate() == st_py)
        assert torch.equal(img, before_img), name
        meta[name] = entry
    # the channel-target table, from the reference's behaviour: a pure-noise call with the noise left as it is (no range rescale) writes
    # noise into the target channels and leaves zeros in the others
    table = {}
    for channels in (1, 3, 4):
        for mode in MODES:
            out = run(torch.zeros(1, 8, 8, channels), 5, pure_noise_mode=True, channel_mode=mode, noise_min=0.0, noise_max=0.0,
                      noise_multiplier=1.0)
            table[f"{mode}/{channels}"] = [c for c in range(channels) if bool((out[..., c] != 0).any())]
    arrays["meta_json"] = np.array(json.dumps({"cases": meta, "targets": table}, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    errors = {k: v["error"] for k, v in meta.items() if v["error"]}
    bad_rng = [k for k, v in meta.items() if not v["rng_restored"]]
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB  refusals: {errors}  rng not restored: {bad_rng}")
    print("targets:", table)


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
