"""Generates tests/golden/preview.npz by running the REAL reference's filter previews (imported through oracle/ref_import.py) in the build
container: ``PowerFilter.preview(raw=True)`` (the two fp32 panels), ``PowerNoiseItem.preview()`` (the three-panel ``L`` image as uint8),
the host spectrum draw the noise panel is made of, and ``rfft2_to_fft2`` of a random real tensor for the small planes.

The uint8 image truncates: a pixel whose fp32 value lies within rounding of a whole number may land on either side of it.  Every stored
case is therefore checked here against an fp64 evaluation of the same formulas (same fp32 filter, same spectrum): fewer than 1 % of the
pixels may differ and none by more than one grey level, or the case does not go into the file (pick another filter or seed).  The shares
are printed and recorded in the archive's ``meta_json``.

    python tests/golden/make_preview_golden.py
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

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "preview.npz")
ABI = json.load(open(os.path.join(HERE, "node_abi.json")))
ref = load_reference()
PN = ref.powernoise

SMALL = ((8, 8), (8, 6), (6, 10), (7, 9), (9, 7))  # rfft2_to_fft2 is stored for these
SIZES = (*SMALL, (16, 12))
FILTERS = {
    "band": dict(),  # PowerFilter's defaults: the band-pass with alpha = 0
    "band_mid": dict(min_freq=0.1, max_freq=0.35),  # stands in for "band" where that case fails the fp64 check (REPLACED)
    "shaped": dict(alpha=1.0, rotate=30.0, stretch=2.0, min_freq=0.05, max_freq=0.45),
    "composed": dict(alpha=1.0, compose_with=dict(min_freq=0.2, max_freq=0.3), compose_mode="max"),
}
# The default band-pass lets every bin through: its kernel is one spike and exact zeros around it, grey level 128.0 on the nose.  On the
# 6 x 10 plane the host FFT leaves +-1e-8 instead of zeros there and 45 % of the kernel panel's pixels truncate to 127 in fp32 but not in
# fp64: the case fails the check below and another band-pass takes its place.
REPLACED = {((6, 10), "band"): "band_mid"}
MIXES = ((1.0, 1.0), (0.5, 1.0), (1.0, 0.5), (0.5, 0.5))  # (mix, filter_norm_factor)


def node_defaults(key):
    return {k: v["default"] for k, v in ABI[key]["inputs"].items() if "default" in v}


def make_filter(spec):
    spec = dict(spec)
    inner = spec.pop("compose_with", None)
    return PN.PowerFilter(compose_with=None if inner is None else PN.PowerFilter(**inner), **spec)


def cases():
    out = {}
    for h, w in SIZES:
        for fname in ("band", "shaped", "composed"):
            fname = REPLACED.get(((h, w), fname), fname)
            # every (mix, norm) pair on two planes (Wh even and odd), the plain pair everywhere
            for mix, nf in (MIXES if (h, w) in ((8, 6), (16, 12)) else MIXES[:1]):
                out[f"{h}x{w}_{fname}_m{mix}_n{nf}"] = dict(size=[h, w], filter=fname, mix=mix, norm=nf)
    # the node's default sockets (SonarPowerNoise), mix as the socket has it and at 0.5
    for mix in (1.0, 0.5):
        out[f"128x128_node_m{mix}_n1.0"] = dict(size=[128, 128], filter="node", mix=mix, norm=1.0)
    return out


def item_for(case):
    if case["filter"] == "node":
        kw = node_defaults("SonarPowerNoise")
        kw.pop("preview")
        kw["mix"] = case["mix"]
        return PN.PowerNoiseItem(**kw)
    return PN.PowerNoiseItem(1.0, power_filter=make_filter(FILTERS[case["filter"]]), time_brownian=False, mix=case["mix"], common_mode=0.0,
                             channel_correlation="1, 1, 1, 1, 1, 1", filter_norm_factor=case["norm"])


def image_fp64(item, size, spectrum):
    """The three panels of PowerNoiseItem.preview in fp64 on the same fp32 filters and spectrum, before the clamp and the cast."""
    nf = getattr(item, "filter_norm_factor", 1.0)
    f_noise = item.make_filter(size, oversample=1).double()
    noise = torch.fft.irfft2(f_noise * spectrum.to(torch.complex128), s=size, norm="ortho")
    f_prev = PN.PowerFilter.normalize(item.power_filter.build(size), (1, 4, *size), mix=1.0, normalization_factor=nf).double()
    kernel = torch.fft.irfft2(f_prev, s=size, norm="ortho").roll((size[0] // 2, size[1] // 2), (-2, -1))
    return torch.cat(((PN.rfft2_to_fft2(f_prev) * (1 / 3)).tanh() * 256.0, ((kernel * (1 / 3)).tanh() + 1.0) * 128.0,
                      ((noise * (1 / 3)).tanh() + 1.0) * 128.0), dim=-1)[0, 0]


def main():
    arrays, meta = {}, {}
    for name, case in cases().items():
        size = tuple(case["size"])
        item = item_for(case)
        nf = getattr(item, "filter_norm_factor", 1.0)
        raw_f, raw_k = item.power_filter.preview(size=size, mix=case["mix"], normalization_factor=nf, raw=True)
        img = np.asarray(item.preview(size=size))
        assert img.dtype == np.uint8 and img.ndim == 2
        # the reference's own draw (PowerNoiseItem.preview, noise=None)
        spectrum = torch.randn((1, 1, size[0], size[1] // 2 + 1), dtype=torch.complex64, generator=torch.Generator().manual_seed(0))
        exact = image_fp64(item, size, spectrum)
        assert tuple(exact.shape) == img.shape, (name, exact.shape, img.shape)
        # a pixel differs when the truncated fp64 value is another grey level
        want = exact.clamp(0, 255).to(torch.uint8).numpy()
        diff = np.abs(img.astype(np.int16) - want.astype(np.int16))
        share = float((diff != 0).mean())
        assert diff.max() <= 1 and share < 0.01, f"{name}: fp32 image vs fp64: {share:.4f} of the pixels differ, worst {diff.max()}: replace the case"
        arrays[f"{name}/filter_panel"] = raw_f.numpy()
        arrays[f"{name}/kernel_panel"] = raw_k.numpy()
        arrays[f"{name}/image"] = img
        arrays[f"{name}/spectrum"] = spectrum.numpy()
        meta[name] = dict(case, fp64_share=share, fp64_worst=int(diff.max()))
    g = torch.Generator().manual_seed(4711)
    for h, w in SMALL:
        x = torch.randn((1, 2, h, w // 2 + 1), generator=g)
        arrays[f"fft2/{h}x{w}/in"] = x.numpy()
        arrays[f"fft2/{h}x{w}/out"] = PN.rfft2_to_fft2(x).contiguous().numpy()
    filters = {k: v for k, v in FILTERS.items()}
    arrays["meta_json"] = np.array(json.dumps({"cases": meta, "filters": filters, "small": [list(s) for s in SMALL]}, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    shares = sorted(((m["fp64_share"], n) for n, m in meta.items()), reverse=True)
    print(f"{os.path.basename(OUT)}  {len(meta)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB")
    print("largest shares of pixels that differ from the fp64 evaluation:", [(n, round(s, 4)) for s, n in shares[:5]])


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
