"""utils.pattern_break (csrc/pattern_break.hip): us per call on [16, 16, 128, 128] and [1, 4, 128, 128] fp32 of
  the new function (default route, restore_scale and lerp: all three phases),
  the reference's op sequence (py/utils.py:575-596) written with torch ops on the same device tensor, its two .item() reads included,
  the library's own out-of-place pass of the same bytes (sonar_scalar_op_f32, x * 1),
and the two routes on n = 4 Ki .. 1 Mi values (powers of two), alternating, to place SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX where they cross.
GPU time from HIP events around batches of calls, several rounds after warm-up calls of every shape; median, minimum and maximum of the
rounds.  Before timing, the outputs of the two routes are compared at every size (torch.equal).
Usage: python scratch/pattern_break_time.py [output file, default profiles/pattern_break_time.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.build()
from comfyui_sonar_amd import hip_lib  # noqa: E402
from comfyui_sonar_amd.py import utils  # noqa: E402

DEV = "cuda"
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pattern_break_time.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def rounds_of(fn, calls, rounds=5, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / calls)
    return times


def row(label, times, extra=""):
    say(f"{label:<58s} median {statistics.median(times):9.2f} us  min {min(times):9.2f}  max {max(times):9.2f}{extra}")
    return statistics.median(times)


def torch_sequence(noise, percentage=0.5, detail_level=0.0):
    orig_min, orig_max = noise.min().item(), noise.max().item()

    def to_scale(t, tmin, tmax):
        lo, hi = t.amin(), t.amax()
        n = t - lo
        n /= (hi - lo).add_(1e-7)
        return n.mul_(tmax - tmin).add_(tmin).clamp_(tmin, tmax)

    normed = to_scale(noise, -1.0, 1.0)
    result = torch.remainder(torch.abs(normed) * 1000000, 11) / 11
    result = ((1 + detail_level / 10) * torch.erfinv(2 * result - 1) * (2**0.5)).mul_(0.2).clamp_(-1, 1)
    result = to_scale(result, orig_min, orig_max)
    return torch.lerp(noise, result, percentage)


LIMIT = max(n for n in (1 << k for k in range(8, 26)) if hip_lib.load().sonar_pattern_break_route(n) == 1)
say(f"device: {torch.cuda.get_device_name(0)}; the default route is one launch up to {LIMIT} values")
g = torch.Generator().manual_seed(1)
for shape, calls in (((16, 16, 128, 128), 100), ((1, 4, 128, 128), 400)):
    x = torch.randn(shape, generator=g).to(DEV)
    out = torch.empty_like(x)
    n = x.numel()
    say(f"--- {list(shape)}: {n} values, {8 * n / 1e6:.2f} MB read + written by a copy")
    t_new = row("pattern_break (default route)", rounds_of(lambda: utils.pattern_break(x), calls))
    for route in ("one", "three"):
        if route == "one" and n > (1 << 20):
            continue
        row(f"pattern_break (route {route!r})", rounds_of(lambda: utils.pattern_break(x, route=route), calls))
    row("pattern_break (restore_scale=False: two launches)", rounds_of(lambda: utils.pattern_break(x, restore_scale=False, route="three"), calls))
    t_torch = row("the reference's op sequence in torch ops on the device", rounds_of(lambda: torch_sequence(x), max(calls // 10, 10)))
    t_copy = row("the library's copy of the same bytes (x * 1)", rounds_of(lambda: hip_lib.mul_scalar(x, 1.0, out), calls))
    say(f"    pattern_break: {t_torch / t_new:.1f} times faster than the torch sequence, {t_new / t_copy:.1f} times the copy")

say("--- route sweep, restore_scale and lerp, the entry point called on buffers allocated once (the Python wrapper's allocations left out);")
say("    us per call, medians of 5 rounds of 300 calls, the routes alternating per size")
lib = hip_lib.load()
ws = torch.empty(hip_lib.PATTERN_BREAK_WS, device=DEV)
stats = hip_lib.new_partials(DEV)
stream = hip_lib._stream()


def raw(x, out, route):
    args = (x.data_ptr(), out.data_ptr(), x.numel(), 1.0, 0.5, 0, 1, route, ws.data_ptr(), ws.numel(), stats.data_ptr(), stream)
    return lambda: lib.sonar_pattern_break_f32(*args)


for k in range(12, 21):
    n = 1 << k
    x = torch.randn(n, generator=g).to(DEV)
    out = torch.empty_like(x)
    assert torch.equal(utils.pattern_break(x, route="one"), utils.pattern_break(x, route="three"))
    one, three = [], []
    for _ in range(5):
        one += rounds_of(raw(x, out, 1), 300, rounds=1, warm=2)
        three += rounds_of(raw(x, out, 2), 300, rounds=1, warm=2)
    say(f"n = {n:8d}  one launch {statistics.median(one):9.2f} us (min {min(one):8.2f})   three launches {statistics.median(three):9.2f} us "
        f"(min {min(three):8.2f})   {'one' if statistics.median(one) < statistics.median(three) else 'three'}")

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
