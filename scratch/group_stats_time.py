"""Statistics + affine update over non-trailing dimensions of a 512x4x128x128 float32 tensor (csrc/group_stats.hip: one sweep for the
per-group mean and std, one for (x - mean[g]) / std[g]; 3 N words moved) for dims (0,), (1,), (0, 2, 3) and (-2,), against (1) the
composition the package had for such a reduction before -- ``dims_last`` (a transposed copy), ``rowstats``, ``row_affine``,
``dims_restore`` (the copy back): 7 N words -- and (2) a ``fill_`` of the tensor (N words written).  Both pairs give the same
normalisation; the script checks them against each other first (the sums are added in another order: 2e-6).  HIP events; the variants
take turns, window by window (100 calls after 10 warm-up calls each), five rounds, median / min / max per variant.
Usage: python scratch/group_stats_time.py [output file; default profiles/group_stats_time.txt]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
import importlib
utils = importlib.import_module("comfyui_sonar_amd.py.utils")
lines = ["# scratch/group_stats_time.py on one MI355X (fp32 512x4x128x128 = 134.2 MB, HIP events, 5 alternating windows of 100 calls per variant)"]


def report(variants, iters=100, warm=10, rounds=5):
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


shape = (512, 4, 128, 128)
x = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 1.5 + 0.4
n_bytes = x.numel() * 4
out = torch.empty_like(x)


def strided(dims):
    mean, std = hl.group_stats(x, dims)
    return hl.group_affine(0, x, dims, mean, std)


def composed(dims):
    xt, inverse = utils.dims_last(x, dims)
    groups = hl.group_segments(shape, dims)[2]
    inner = x.numel() // groups
    mean, std = hl.rowstats(xt, groups, inner)
    return utils.dims_restore(hl.row_affine(0, xt, groups, inner, mean, std), inverse)


for dims in ((0,), (1,), (0, 2, 3), (-2,)):
    a, b = strided(dims), composed(dims)
    torch.testing.assert_close(a, b, rtol=0, atol=2e-6 * float(b.abs().max()) + 2e-6)
    del a, b
    sizes, first, groups = hl.group_segments(shape, dims)
    tag = f"dims {dims}: segments {sizes}, {'reduced' if first else 'kept'} first, {groups} groups of {x.numel() // groups}"
    new, old, fill = report([(f"dims {dims}: group_stats + group_affine", lambda: strided(dims)),
                             (f"dims {dims}: dims_last + rowstats + row_affine + dims_restore", lambda: composed(dims)),
                             (f"dims {dims}: fill_ of the tensor", lambda: out.fill_(1.0))])
    lines.append(f"{tag}: strided pair {new:.1f} us = {3 * n_bytes / new / 1e6:.2f} TB/s over its 3 N words, {new / fill:.2f} x the fill_; "
                 f"composition {old:.1f} us ({old / new:.2f} x the pair)")
    print(lines[-1], flush=True)

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "group_stats_time.txt")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
