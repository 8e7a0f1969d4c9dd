"""Quantile filter on 512 x 4 x 128 x 128 fp32 (the bench shape): us per call of utils.quantile_normalize (dim 1 flattened: 512 rows of
65536, register-resident) for clamp / median / replace_2pt, A/B against the StudentT composition abs_quantile_rows + clamp_signpow_rows
on a copy, dim 0 (one row of 33.5 M values), "global", few rows and long rows (the multi-workgroup route), and a same-size device copy.  Usage: python scratch/quantile_time.py"""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
utils = importlib.import_module("comfyui_sonar_amd.py.utils")
torch.manual_seed(0)
x = torch.randn(512, 4, 128, 128, device="cuda")
b, inner = 512, 4 * 128 * 128
y = torch.empty_like(x)


def composition():
    y.copy_(x)  # the composition works in place; the filter must not touch its input
    nq = hl.abs_quantile_rows(y, b, inner, 0.85)
    hl.clamp_signpow_rows_(y, b, inner, nq, 1.0, 0.5)


def report(name, fn, iters=20, warm=3):
    fn()
    times = sorted(bench.event_us(fn, iters, warm) for _ in range(5))
    print(f"{name:44s} median {times[2]:9.1f} us  min {times[0]:9.1f}", flush=True)
    return times[2]


copy_us = report("copy (y.copy_(x), 134 MB read + write)", lambda: y.copy_(x))
comp_us = report("composition clamp (copy + quantile + clamp)", composition)
new_us = report("quantile_normalize clamp dim 1", lambda: utils.quantile_normalize(x, quantile=0.85, strategy="clamp"))
ref = x.clone(); composition()
got = utils.quantile_normalize(x, quantile=0.85, strategy="clamp")
print(f"clamp: max |new - composition| = {float((got - y).abs().max()):.3e}")
print(f"clamp: new / composition = {new_us / comp_us:.3f}; new / copy = {new_us / copy_us:.2f}; (composition - copy) / new = {(comp_us - copy_us) / new_us:.2f}")
report("quantile_normalize median dim 1", lambda: utils.quantile_normalize(x, quantile=0.85, strategy="median"))
report("quantile_normalize replace_2pt dim 1", lambda: utils.quantile_normalize(x, quantile=0.85, strategy="replace_2pt"), iters=5, warm=1)
report("quantile_normalize clamp dim 0 (one row)", lambda: utils.quantile_normalize(x, quantile=0.85, dim=0, strategy="clamp"))
report("quantile_normalize median dim 0 (one row)", lambda: utils.quantile_normalize(x, quantile=0.85, dim=0, strategy="median"))
report("quantile_normalize clamp global, flatten=False", lambda: utils.quantile_normalize(x, quantile=0.85, dim=None, flatten=False, strategy="clamp"))
few = x[:8].contiguous()
report("8 rows of 65536: clamp dim 1 (row kernel)", lambda: utils.quantile_normalize(few, quantile=0.85, strategy="clamp"))
report("8 rows of 65536: composition (one workgroup per row)", lambda: (lambda yy: hl.clamp_signpow_rows_(yy, 8, inner, hl.abs_quantile_rows(yy, 8, inner, 0.85), 1.0, 0.5))(few.clone()))
long = torch.randn(2, 16, 128, 128, device="cuda")
report("2 rows of 262144: clamp dim 1 (split)", lambda: utils.quantile_normalize(long, quantile=0.85, strategy="clamp"))
