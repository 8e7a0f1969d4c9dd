"""FreeUExtremeConfig.apply on float16 maps of SDXL's three stages at batch 2, slice 1.0 and 0.5, three ways in one process, alternating:
the fused route, the pre-filtered route (cast + sonar_spectral_filter_f32 + one finishing sweep) and the same values composed from
ffilter + torch ops as the reference's apply is written (what the parent commit offers).  Every timed call gets a fresh clone made outside
the timed region; each figure is the median of 4 x 30 event-timed calls.  Before timing, the three results are compared with each other.
Rewrites the section between the timing markers of profiles/freeu_extreme.md:

    python scratch/freeu_time.py            # the table
    python scratch/freeu_time.py --trace    # only a few fused calls per shape: the workload of a kernel-trace run of its own
"""
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sonar_pkg  # noqa: E402

pkg = sonar_pkg.load()
pkg.hip_lib.load()
fx = importlib.import_module("comfyui_sonar_amd.py.nodes.freeu_extreme")
PF = importlib.import_module("comfyui_sonar_amd.py.nodes.powernoise").PowerFilter
HBM_PEAK = 8.0e12  # bytes / s
SHAPES = ((2, 1280, 32, 32), (2, 640, 64, 64), (2, 320, 128, 128))
BEGIN, END = "<!-- timing:begin -->", "<!-- timing:end -->"


def composed(cfg, idx, x, cache):
    """The reference's apply, line by line, on the parent commit's pieces."""
    c0, cn = cfg.slice_bounds(x.shape[1])
    hmean = x.mean(1).unsqueeze(1)
    hmax, hmin = (op(hmean.view(hmean.shape[0], -1), dim=-1, keepdim=True)[0] for op in (torch.max, torch.min))
    hmean -= hmin.unsqueeze(2).unsqueeze(3)
    hmean /= (hmax - hmin).unsqueeze(2).unsqueeze(3)
    scale = 1.0 + (cfg.scale - 1.0) * hmean
    xs = fx.ffilter(x[:, c0:c0 + cn], cfg.sonar_power_filter, normalization_factor=cfg.filter_norm, cfg_idx=idx, filter_cache=cache) * scale
    x[:, c0:c0 + cn] = torch.lerp(x[:, c0:c0 + cn], xs, cfg.blend)
    return x


def routed(cfg, x, cache, prefiltered):
    keep = fx.PREFILTERED_PLANES
    fx.PREFILTERED_PLANES = frozenset({tuple(x.shape[-2:])}) if prefiltered else frozenset()
    try:
        return cfg.apply(0, x, cache)
    finally:
        fx.PREFILTERED_PLANES = keep


def timed(fn, x, reps=30):
    out = []
    for _ in range(reps):
        y = x.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(y)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def main():
    rows, checks = [], []
    for shape in SHAPES:
        for sl in (1.0, 0.5):
            cfg = fx.FreeUExtremeConfig(target="both", stage_1=True, slice=sl, scale=1.2, blend=0.7, blend_mode="lerp", hidden_mean=True,
                                        sonar_power_filter_opt=PF(alpha=1.0, max_freq=0.7071))
            x = (torch.randn(shape, device="cuda") + torch.tensor([0.7, -1.1], device="cuda").view(2, 1, 1, 1)).half()
            ca, cb = {}, {}
            fns = {"fused": lambda y: routed(cfg, y, ca, False), "prefiltered": lambda y: routed(cfg, y, ca, True),
                   "composed": lambda y: composed(cfg, 0, y, cb)}
            res = {k: f(x.clone()).float() for k, f in fns.items()}
            if "--trace" in sys.argv:
                for _ in range(5):
                    fns["fused"](x.clone())
                torch.cuda.synchronize()
                continue
            span = (res["composed"].max() - res["composed"].min()).item()
            d = {k: ((res[k] - res["composed"]).abs().max().item() / span) for k in ("fused", "prefiltered")}
            d["routes"] = (res["fused"] - res["prefiltered"]).abs().max().item() / span
            assert all(torch.isfinite(v).all() for v in res.values()) and max(d.values()) < 4 * 2.0 ** -11, (shape, sl, d)  # a few fp16 roundings of the composition
            checks.append(f"| {shape} | {sl} | {d['fused']:.2e} | {d['prefiltered']:.2e} | {d['routes']:.2e} |")
            for k, f in fns.items():
                timed(f, x, 5)
            t = {k: [] for k in fns}
            for _ in range(4):  # alternate
                for k, f in fns.items():
                    t[k] += timed(f, x)
            med = {k: statistics.median(v) for k, v in t.items()}
            n = x.numel() * 2
            floor = n + 2 * n * sl  # one read of x for the mean, one read and one write of the slice
            best = min(med["fused"], med["prefiltered"])
            rows.append(f"| {shape} | {sl} | {med['fused']:.1f} | {med['prefiltered']:.1f} | {med['composed']:.1f} | {med['composed'] / med['fused']:.2f} | "
                        f"{med['composed'] / med['prefiltered']:.2f} | {floor / 1e6:.1f} | {floor / (best * 1e-6) / HBM_PEAK:.1%} |")
    if "--trace" in sys.argv:
        return
    table = (f"{BEGIN}\n### Measured (us per call, medians of 120 event-timed calls; floor = one read of x + one read and one write of the slice)\n\n"
             "| shape | slice | fused | pre-filtered | composed | composed / fused | composed / pre-filtered | floor MB | floor at HBM peak / best time |\n"
             "|---|---|---|---|---|---|---|---|---|\n" + "\n".join(rows) +
             "\n\n### The same calls compared (largest difference as a fraction of the output's range, float16)\n\n"
             "| shape | slice | fused vs composed | pre-filtered vs composed | fused vs pre-filtered |\n|---|---|---|---|---|\n" + "\n".join(checks) + f"\n{END}\n")
    print(table)
    path = os.path.join(ROOT, "profiles", "freeu_extreme.md")
    text = open(path).read()
    if BEGIN in text and END in text:
        text = text[:text.index(BEGIN)] + table + text[text.index(END) + len(END) + 1:]
    else:
        text += "\n" + table
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
