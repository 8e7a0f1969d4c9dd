"""hip_lib.scat_layer (csrc/scatternet.hip): us per call on a [64, 4, 256, 256] fp32 input -- the scatter step of ScatternetFilteredNoise at
batch 64, C = 4, a 128 x 128 latent, default mode (order 1, the inner plane enlarged by 2) -- of
  the fused layer with the item's window (channels 0 .. C - 1 of the 7 C),
  the fused layer writing all 7 C channels,
  the unfused composition on the device path as it was: DTCWT(level=1).forward (six axis_taps launches and a q2c), torch magnitude,
  avg_pool2d and cat, and that composition followed by the slice the item keeps.
GPU time from HIP events around batches of calls, alternating the candidates inside every round, after warm-up calls; median, minimum and
maximum of the rounds.  Bytes are the least each call has to move (input once, output once), computed from the shapes; the share of peak
is those bytes over the time against 8.0 TB/s (spec) -- for the window call, which reads L2-resident halos again, a share of what HBM
must do, not a count of what the kernel requests.  Before timing, fused and unfused are compared.
Usage: python scratch/scatternet_time.py [output file, default profiles/scatternet_time.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.build()
from comfyui_sonar_amd import hip_lib  # noqa: E402
from comfyui_sonar_amd.py.dtcwt import DTCWT  # noqa: E402

DEV = "cuda"
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scatternet_time.txt")
PEAK = 8.0e12
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


B, C, H, W = 64, 4, 256, 256
x = torch.randn(B, C, H, W, device=DEV)
dt = DTCWT(level=1)
bias = 1e-2


def unfused():
    yl, yh = dt.forward(x)
    mag = torch.sqrt(yh[0][..., 0] ** 2 + yh[0][..., 1] ** 2 + bias * bias) - bias
    return torch.cat((torch.nn.functional.avg_pool2d(yl, 2)[:, None], mag.movedim(2, 1)), dim=1).reshape(B, 7 * C, H // 2, W // 2)


def unfused_window():
    return unfused()[:, :C].contiguous()


def fused_all():
    return hip_lib.scat_layer(x, magbias=bias)


def fused_window():
    return hip_lib.scat_layer(x, magbias=bias, channels=(0, C))


cands = {"fused, window of C channels": fused_window, "fused, all 7 C channels": fused_all, "unfused composition, all 7 C": unfused,
         "unfused composition + the item's slice": unfused_window}
ref = unfused()
err = float((fused_all() - ref).abs().max())
say(f"input [{B}, {C}, {H}, {W}] fp32; max |fused - unfused| = {err:.3e}; window == full slice: {torch.equal(fused_window(), fused_all()[:, :C])}")
for fn in cands.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
CALLS, ROUNDS = 50, 7
times = {k: [] for k in cands}
for _ in range(ROUNDS):
    for name, fn in cands.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        times[name].append(a.elapsed_time(b) * 1e3 / CALLS)
in_bytes = B * C * H * W * 4
out_all, out_win = 7 * in_bytes // 4, in_bytes // 4
least = {"fused, window of C channels": in_bytes + out_win, "fused, all 7 C channels": in_bytes + out_all,
         "unfused composition, all 7 C": in_bytes + out_all, "unfused composition + the item's slice": in_bytes + out_win}
for name, t in times.items():
    med = statistics.median(t)
    say(f"{name:<42s} median {med:9.2f} us  min {min(t):9.2f}  max {max(t):9.2f}   least bytes {least[name] / 1e6:7.2f} MB"
        f" -> {least[name] / (med * 1e-6) / 1e12:5.2f} TB/s = {100 * least[name] / (med * 1e-6) / PEAK:5.1f} % of 8.0 TB/s")
m = {k: statistics.median(v) for k, v in times.items()}
names = list(cands)
say(f"window: the unfused path takes {m[names[3]] / m[names[0]]:.1f} x the fused call's time; all 7 C: {m[names[2]] / m[names[1]]:.1f} x")
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
