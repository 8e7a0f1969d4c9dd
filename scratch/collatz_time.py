"""Collatz noise on 4 x 4 x 128 x 128 fp32, generate mode, default parameters (10 iterations, quantile 0.5): us per call of
CollatzNoiseGenerator (csrc/collatz.hip: one chain launch and one mix launch per iteration) against the op sequence of
tests/collatz_refs.py written with torch ops on the same device (about twenty small launches per link of the chains), both with the
same draws, the same utils.quantile_normalize and the same result.  Also the two kernels alone for one iteration.
Usage: python scratch/collatz_time.py"""
import importlib, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
utils = importlib.import_module("comfyui_sonar_amd.py.utils")
shape = (4, 4, 128, 128)
x = torch.zeros(shape, device="cuda")
gen = ng.CollatzNoiseGenerator(x, cpu=False, normalized=False)
P = gen.ng_params()


def report(name, fn, iters=10, warm=2):
    fn()
    times = sorted(bench.event_us(fn, iters, warm) for _ in range(5))
    print(f"{name:64s} median {times[2]:10.1f} us  min {times[0]:10.1f}", flush=True)
    return times[2]


def rem2(t):
    return torch.remainder(t, 2.0)


def torch_chain(seeds, cl, offset):
    """tests/collatz_refs.py chain(), default parameters, output ratios: [outer][n_chunks][inner] -> [outer][n_chunks * cl][inner]."""
    noise = seeds * (P["rmax"] - P["rmin"] + 1) + P["rmin"]
    noise = torch.where(noise == 0, noise.max() / noise.numel(), noise)
    result, muls, adds = noise, torch.ones_like(noise), torch.zeros_like(noise)
    kept = []
    for t in range(cl + offset):
        if t > 0:
            prev = result
            xi = prev.trunc()
            pt = xi + ((prev - xi) * 100.0).trunc() * (1.0 / 100)
            reset = ((pt >= 1.0) & (pt < 1.001)) | (pt.abs() < 0.001)
            even = rem2(prev) < 1.0
            m = torch.where(reset, 1.0, torch.where(even, muls * P["even_multiplier"], muls * P["odd_multiplier"]))
            a = adds * m
            a = torch.where(reset, 0.0, torch.where(even, a, a + P["odd_addition"] * prev.sign()))
            result, muls, adds = torch.where(reset, noise, (noise * m + a).trunc()), m, a
        if t >= offset:
            kept.append(result / noise)
    return torch.stack(kept, dim=2).reshape(seeds.shape[0], seeds.shape[1] * cl, seeds.shape[2])


def torch_call():
    dims = tuple(d % 4 for d in P["dims"])
    acc = torch.zeros(shape, device="cuda")
    for it in range(P["iterations"]):
        dim, chain_length = dims[it % len(dims)], P["chain_length"][it % len(P["chain_length"])]
        outer, length, inner = math.prod(shape[:dim]), shape[dim], math.prod(shape[dim + 1:])
        cl, n_chunks, _ = hl.collatz_view(outer, length, inner, chain_length)
        seeds = gen.rand_like(fun=torch.rand, shape=(outer, n_chunks, inner))
        out1 = utils.quantile_normalize(torch_chain(seeds, cl, P["chain_offset"]), quantile=P["quantile"], dim=0, strategy=P["quantile_strategy"])
        v = seeds.repeat_interleave(cl, 1)[:, :length] * out1[:, :length]
        acc += (v * ((1.0 / P["iterations"]) * (-1 if it & 1 else 1))).reshape(shape)
    return acc


torch.manual_seed(0)
a = gen.generate()
torch.manual_seed(0)
b = torch_call()
print(f"same draws: equal {bool(torch.equal(a, b))}, max |difference| {float((a - b).abs().max()):.3g}", flush=True)
t_kernel = report("CollatzNoiseGenerator.generate (chain + mix kernels)", lambda: gen.generate(), iters=5, warm=1)
t_torch = report("the same op sequence in torch ops", torch_call, iters=3, warm=1)
print(f"ratio torch / kernels {t_torch / t_kernel:.1f}", flush=True)
gen0 = ng.CollatzNoiseGenerator(x, cpu=False, normalized=False, quantile=0)
report("the same call with the quantile stage off", lambda: gen0.generate(), iters=5, warm=1)
for dim, chain_length in ((3, 3), (2, 3), (3, 128), (2, 128)):
    outer, length, inner = math.prod(shape[:dim]), shape[dim], math.prod(shape[dim + 1:])
    cl, n_chunks, len_p = hl.collatz_view(outer, length, inner, chain_length)
    seeds = torch.rand(outer * n_chunks * inner, device="cuda")
    ext, out1, acc = seeds.max().reshape(1), torch.empty(outer * len_p * inner, device="cuda"), torch.zeros(shape, device="cuda")
    kw = dict(span=16001.0, rmin=-8000.0, even_multiplier=0.5, even_addition=0.0, odd_multiplier=3.0, odd_addition=1.0, integer_math=True,
              break_loops=True, add_preserves_sign=True, seed_mode="default", output="ratios", out=out1)
    report(f"chain kernel, dim {dim}, chain length {chain_length} ({'LDS-staged' if inner == 1 else 'direct'} stores)",
           lambda: hl.collatz_chain(seeds, ext, outer, length, inner, chain_length, 5, **kw), iters=20)
    report(f"mix kernel, dim {dim}, chain length {chain_length}",
           lambda: hl.collatz_mix_(acc, out1, seeds, "seeds", outer, length, inner, chain_length, 0.1), iters=20)
