"""Voronoi noise on 4 x 4 x 128 x 128 fp32, generate mode, 256 feature points: us per call of VoronoiNoiseGenerator.generate
(csrc/voronoi.hip) against the reference's op sequence written with torch ops on the same device (the [B, C, H, W, N, 3] differences, the
distance, a sort of the last axis and the result).  Both presets' parameter sets: NoiseType.VORONOI_MIX's generator (3 octaves, euclidean,
diff2, new_features: one launch per octave) and NoiseType.VORONOI_FUZZ's (1 octave, fuzz:name=angle_tanh:fuzz=0.1, diff2: three launches,
the uniforms computed in the kernel; the torch sequence draws the [B, C, H, W, N] tensor and reads the extremes on the host, as the
reference does).  Both have z_max 0 and re-draw their features on every call.  GPU time from HIP events around each call, median and
minimum of the repetitions after warm-up calls.
Usage: python scratch/voronoi_time.py"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

entry.build()
from comfyui_sonar_amd.py import noise_generation as ng  # noqa: E402

DEV = "cuda"
SHAPE = (4, 4, 128, 128)
x = torch.zeros(SHAPE, device=DEV)
SIG = (torch.tensor(10.0), torch.tensor(5.0))
SETS = {
    "voronoi_mix": dict(n_points=(256,), octaves=3, distance_mode=("euclidean",), result_mode=("diff2",), octave_mode="new_features",
                        lacunarity=2.0, gain=0.75, z_max=0.0),
    "voronoi_fuzz": dict(n_points=(256,), octaves=1, distance_mode=("fuzz:name=angle_tanh:fuzz=0.1",), result_mode=("diff2",), z_max=0.0),
}


def report(label, fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    print(f"{label:<72s} median {statistics.median(times):10.1f} us  min {min(times):10.1f}", flush=True)
    return statistics.median(times)


def torch_sequence(p):
    B, C, H, W = SHAPE
    y, xs = torch.linspace(0, H - 1, H, device=DEV), torch.linspace(0, W - 1, W, device=DEV)
    grid = torch.stack(torch.meshgrid(y, xs, indexing="ij"), dim=-1) / torch.tensor((H, W), device=DEV)

    def call():
        feats = [torch.rand(B, C, p["n_points"][0], 3, device=DEV) for _ in range(p["octaves"] if p.get("octave_mode") == "new_features" else 1)]
        z_grid = grid.new_full((H, W, 1), 0.0)
        result = grid.new_zeros(SHAPE)
        amplitude, scale, total = 1.0, 1.0, 0.0
        for octave in range(p["octaves"]):
            g3 = torch.cat((grid, z_grid), dim=-1)[None, None].expand(B, C, -1, -1, -1).unsqueeze(-2)
            g3 = (g3 * scale) % 1.0
            fp = (feats[octave % len(feats)][:, :, None, None] * scale) % 1.0
            d = (g3 - fp + 0.5) % 1.0 - 0.5
            if p["distance_mode"][0] == "euclidean":
                dist = d.pow(2).sum(dim=-1).sqrt_()
            else:
                dist = torch.nn.functional.normalize(d, dim=-1)[..., 2].tanh_().acos_()
                rmin, rmax = dist.aminmax()
                spread = max(abs(rmin.item()), abs(rmax.item())) * 0.1
                dist += torch.rand(dist.shape, device=DEV).mul_(spread * 2).sub_(spread)
                lo, hi = dist.amin(dim=(-2, -1), keepdim=True), dist.amax(dim=(-2, -1), keepdim=True)
                dist = (dist - lo).div_((hi - lo).add_(1e-07)).mul_(rmax.item() - rmin.item()).add_(rmin.item()).clamp_(rmin.item(), rmax.item())
            s = dist.sort(dim=-1).values
            v1, v2 = s[..., 0], s[..., 1]
            result += ((v2 - v1) / (v2 + v1 + 1e-06)).mul_(amplitude)
            total += abs(amplitude)
            amplitude *= p.get("gain", 0.5)
            scale *= p.get("lacunarity", 2.0)
        return result.div_(total)

    return call


for label, p in SETS.items():
    gen = ng.VoronoiNoiseGenerator(x, cpu=False, normalized=False, **p)
    t_kernel = report(f"{label}: VoronoiNoiseGenerator.generate (fused octave kernel)", lambda: gen.generate(*SIG))
    t_torch = report(f"{label}: the same op sequence in torch ops on the device", torch_sequence(p), iters=5, warm=1)
    print(f"{label}: the kernel route is {t_torch / t_kernel:.1f} times faster", flush=True)
