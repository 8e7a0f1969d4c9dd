"""SonarCustomNoiseParameters' tail (fix_invalid -> crop -> scale_noise, csrc/noise_params.hip: a scan launch and an apply launch, the
source read twice and the output written once) on a 512x4x128x128 float32 result, without a crop and with one (128x128 kept out of a
130x130 source), against (1) a ``fill_`` of the output and (2) the same arithmetic composed from torch's own operations as the reference
writes it (py/noise.py:2172-2185, py/utils.py:100-106: nan_to_num x 2 with max / min read back, flatten + slice + reshape, mean / std
read back, sub, div, mul).  The torch composition works on a copy-free view where the reference does and leaves its input alone (the
first nan_to_num is out of place in the reference too), so every window runs on the same data.  HIP events; the variants take turns,
window by window (300 calls after 20 warm-up calls each), five rounds, median / min / max per variant.
Usage: python scratch/noise_params_time.py [output file; default profiles/noise_params_time.txt]"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
lines = ["# scratch/noise_params_time.py on one MI355X (fp32, fix_invalid + normalisation + factor 0.6, HIP events, 5 alternating windows of 300 calls per variant)"]
FACTOR = 0.6


def report(variants, iters=300, warm=20, rounds=5):
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(bench.event_us(fn, iters, warm))
    meds = []
    for name, _ in variants:
        t = sorted(times[name])
        meds.append(t[len(t) // 2])
        lines.append(f"{name:78s} median {meds[-1]:8.2f} us  min {t[0]:8.2f}  max {t[-1]:8.2f}")
        print(lines[-1], flush=True)
    return meds


def torch_tail(noise, lead, plane_out, shape):
    tmp = noise.nan_to_num(0, posinf=0, neginf=0)
    noise = noise.nan_to_num(0, posinf=float(tmp.max()), neginf=float(tmp.min()))
    noise = noise.reshape(lead, -1)[..., :plane_out].reshape(shape)
    mean, std = noise.mean().item(), noise.std().item()
    thr = 2.5 / math.sqrt(noise.numel())
    if abs(mean) > thr:
        noise -= mean
    if abs(1.0 - std) > thr:
        noise /= std
    return noise.mul_(FACTOR)


shape = (512, 4, 128, 128)
planes, plane_out = shape[0] * shape[1], shape[2] * shape[3]
for side in (128, 130):
    plane_in = side * side
    g = torch.Generator(device="cuda").manual_seed(side)
    src = torch.randn(planes, plane_in, device="cuda", generator=g) * 1.7 + 0.8
    flat = src.view(-1)
    flat[::100003] = float("nan"); flat[7::200003] = float("inf"); flat[11::300007] = float("-inf")
    keep = src.clone()
    out = hl.noise_params_tail(src, shape, torch.float32, planes, plane_in, plane_out, fix_invalid=True, normalized=True, factor=FACTOR)
    ref = torch_tail(src, planes, plane_out, shape)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-6)
    tag = f"{planes} planes, {plane_in} -> {plane_out}"
    moved = (2 * planes * plane_in + planes * plane_out) * 4
    lines.append(f"## {tag}: source {planes * plane_in * 4 / 1e6:.1f} MB, output {out.numel() * 4 / 1e6:.1f} MB; the tail moves {moved / 1e6:.1f} MB; kernels and torch composition agree (rtol 1e-5, atol 1e-6)")
    tail, fill, comp = report([(f"{tag}: HIP tail (2 launches)", lambda: hl.noise_params_tail(src, shape, torch.float32, planes, plane_in, plane_out, fix_invalid=True, normalized=True, factor=FACTOR)),
                               (f"{tag}: fill_ of the output", lambda: out.fill_(1.0)),
                               (f"{tag}: torch composition (host reads max / min / mean / std back)", lambda: torch_tail(src, planes, plane_out, shape))])
    assert torch.equal(torch.isnan(src), torch.isnan(keep)) and torch.equal(src.nan_to_num(0, 0, 0), keep.nan_to_num(0, 0, 0)), "a timed call wrote its input"
    lines.append(f"{tag}: tail {tail:.2f} us = {moved / tail / 1e6:.2f} TB/s over its own traffic, {tail / fill:.2f} x the fill_; torch composition {comp:.2f} us ({comp / tail:.2f} x the tail)")
    print(lines[-1], flush=True)
    del src, keep, out, ref

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "noise_params_time.txt")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
