"""Distro noise on 512 x 4 x 128 x 128 fp32 (the bench shape), generate mode: us per raw fill (sonar_distro_fill_f32 through the
generator, normalisation off) for every family with default parameters, the default node call (uniform, "batch" mode: quantile over
dim 0 + the output normalisation), NoiseType "distro" (normal, quantile at dim 1), and the plain Gaussian fill for scale.
Usage: python scratch/distro_time.py"""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sonar_pkg, bench
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
reg = importlib.import_module("comfyui_sonar_amd.py.nodes.registry")
noise = importlib.import_module("comfyui_sonar_amd.py.noise")
shape = (512, 4, 128, 128)
x = torch.zeros(shape, device="cuda")
torch.manual_seed(0)


def report(name, fn, iters=10, warm=2):
    fn()
    times = sorted(bench.event_us(fn, iters, warm) for _ in range(5))
    print(f"{name:48s} median {times[2]:9.1f} us  min {times[0]:9.1f}", flush=True)
    return times[2]


gauss = ng.GaussianNoiseGenerator(x, cpu=False, normalized=False)
report("gaussian fill (GaussianNoiseGenerator, raw)", lambda: gauss())
for fam in ng.DistroNoiseGenerator.FAMILIES:
    gen = ng.DistroNoiseGenerator(x, distro=fam, result_index=(-1,), cpu=False, quantile_norm=1.0, normalized=False)
    report(f"raw fill {fam}", lambda: gen())
node = reg.NODE_CLASS_MAPPINGS["SonarAdvancedDistroNoise"]()
sockets = {k: v["default"] for k, v in reg.NODE_ABI["SonarAdvancedDistroNoise"]["inputs"].items() if "default" in v}
ns = node.go(**sockets)[0].make_noise_sampler(x, 0.03, 14.6, seed=0, cpu=False, normalized=True)
report("node, default sockets (uniform, batch mode, normalised)", lambda: ns(torch.tensor(10.0), torch.tensor(5.0)), iters=5, warm=1)
item = noise.CustomNoiseItem(1.0, noise_type="distro", ns_kwargs={})
ins = item.make_noise_sampler(x, 0.03, 14.6, seed=0, cpu=False, normalized=True)
report("NoiseType distro (normal, dim 1, normalised)", lambda: ins(torch.tensor(10.0), torch.tensor(5.0)))
