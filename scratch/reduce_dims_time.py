"""scale_noise(normalize_dims=...) and the power-law peak division over non-adjacent dimensions of a 512x4x128x128 float32 tensor, in place:

  scale_noise (0, 2) and (1, 3)   the strided route (group_stats, the divided mean, the apply kernel: 3 reads + 1 write of the tensor)
                                  against the route of the commit before -- ``dims_last`` (a transposed copy), the row kernel,
                                  ``dims_restore`` (the copy back);
  power law (0, 2)                ``group_peak`` + ``group_div_`` against the adjacent-dims pair ``amax_mid`` + ``div_mid_`` over (2, 3) of
                                  the same tensor (the commit before refuses (0, 2)).  The pow before them is the same call in both and is
                                  left out.

The routes are checked against each other first (bit for bit).  HIP events; the variants take turns, window by window (100 calls after 10
warm-up calls each), five rounds, median / min / max per variant; and the box's device-to-device copy rate as bench.py measures it.
Usage: python scratch/reduce_dims_time.py [output file; default profiles/reduce_dims_time.txt]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
import importlib
utils = importlib.import_module("comfyui_sonar_amd.py.utils")
lines = ["# scratch/reduce_dims_time.py on one MI355X (fp32 512x4x128x128 = 134.2 MB, HIP events, 5 alternating windows of 100 calls per variant)"]


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
base = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 1.5 + 0.4
n_bytes = base.numel() * 4
x = base.clone()


def transposed(dims, factor=0.35):
    rows_last, inverse = utils.dims_last(x, dims)
    inner = x.numel() // hl.group_segments(shape, dims)[2]
    return utils.dims_restore(hl.scale_noise_rows_(rows_last, x.numel() // inner, inner, factor), inverse)


big_a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
big_b = torch.empty_like(big_a)
copy = 2 * big_a.numel() * 4 / (bench.event_us(lambda: big_b.copy_(big_a), 10, 3) * 1e-6) / 1e9
del big_a, big_b
lines.append(f"device-to-device copy of 1 GiB: {copy:.0f} GB/s read + write")
print(lines[-1], flush=True)

for dims in ((0, 2), (1, 3)):
    x.copy_(base)
    want = transposed(dims)
    assert torch.equal(hl.group_scale_noise_(x, dims, 0.35), want)
    del want
    sizes, first, groups = hl.group_segments(shape, dims)
    new, old = report([(f"scale_noise normalize_dims {dims}: strided route, in place", lambda: hl.group_scale_noise_(x, dims, 0.35)),
                       (f"scale_noise normalize_dims {dims}: dims_last + scale_noise_rows_ + dims_restore", lambda: transposed(dims))])
    lines.append(f"dims {dims}: segments {sizes}, {'reduced' if first else 'kept'} first, {groups} groups of {x.numel() // groups}: strided route "
                 f"{new:.1f} us = {4 * n_bytes / new / 1e6:.2f} TB/s over its 4 N words; transposed route {old:.1f} us ({old / new:.2f} x)")
    print(lines[-1], flush=True)

x.copy_(base)
peak = hl.group_peak(x, (0, 2), True)
assert torch.equal(peak, x.abs().amax(dim=(0, 2)).flatten())
assert torch.equal(hl.group_div_(x.clone(), (0, 2), peak), x / x.abs().amax(dim=(0, 2), keepdim=True))
new, old = report([("power law div_max_dims (0, 2): group_peak + group_div_", lambda: hl.group_div_(x, (0, 2), hl.group_peak(x, (0, 2), True))),
                   ("power law div_max_dims (2, 3): amax_mid + div_mid_", lambda: hl.div_mid_(x, 2048, 16384, 1, hl.amax_mid(x, 2048, 16384, 1, True)))])
lines.append(f"power law: (0, 2) {new:.1f} us = {3 * n_bytes / new / 1e6:.2f} TB/s over its 3 N words; adjacent (2, 3) {old:.1f} us ({old / new:.2f} x)")
print(lines[-1], flush=True)

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "reduce_dims_time.txt")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write("\n".join(lines) + "\n")
