"""The two Brownian increments of a DPM++ SDE step on cfg5's shard (128 x 16 x 128 x 128, tree depth 24): GPU time of
``BrownianTreeNoiseSampler.pair`` (one launch for (t, s) and (t, t')) against the two single calls, with and without the statistics a
normalised draw reduces in the same pass.  Both ways are timed in the same process, alternating, five rounds of 24 steps each; the spread
of the two-call figure over the rounds is the bar ``pair`` has to stay within."""
import importlib, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sonar_pkg
pkg = sonar_pkg.load(); hl = pkg.hip_lib; hl.load()
NG = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
x = torch.zeros(128, 16, 128, 128, device="cuda")
sig = [14.6 * 0.93**k for k in range(33)]


def steps(ns, paired, stats, k0, k1):
    for k in range(k0, k1):
        s, sm, sn = sig[k], math.sqrt(sig[k] * sig[k + 1]), sig[k + 1]
        parts = tuple(hl.new_partials("cuda") for _ in range(2)) if stats else None
        if paired:
            ns.pair(s, sm, sn, partials=parts)
        else:
            ns(s, sm, partials=parts[0] if stats else None)
            ns(s, sn, partials=parts[1] if stats else None)


def timed(paired, stats):
    ns = NG.BrownianTreeNoiseSampler(x, 0.03, 14.6, seed=5, tree_depth=24)
    steps(ns, paired, stats, 0, 8)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    steps(ns, paired, stats, 8, 32)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 24 * 1e3  # us per step (both increments)


for stats in (True, False):
    rows = {False: [], True: []}
    for _ in range(5):
        for paired in (False, True):
            rows[paired].append(timed(paired, stats))
    for paired in (False, True):
        r = sorted(rows[paired])
        print(f"statistics {'on ' if stats else 'off'}  {'pair     ' if paired else 'two calls'}: median {r[2]:7.1f} us per step, "
              f"min {r[0]:7.1f}, max {r[-1]:7.1f}", flush=True)
