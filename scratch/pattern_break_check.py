"""utils.pattern_break / PatternBreakNoise on the device against the golden cases (tests/golden/pattern_break*.npz): per function case the
kernel's largest distance from the fp64 statement (tests/pattern_break_refs.py) and from the reference's stored output, over the case's
output range, and whether the two routes gave the same bits; per item case and call the largest distance from the reference's output.
The figures tests/test_gpu_pattern_break.py asserts on, kept as a file.
Usage: python scratch/pattern_break_check.py [output file, default profiles/pattern_break_kernel.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry.build()
from comfyui_sonar_amd.py import noise as nz  # noqa: E402
from tests import pattern_break_refs as R  # noqa: E402

cases = R.cases
DEV = "cuda"
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pattern_break_kernel.txt")
st = R.statements()
E = st["E"]
lines = [f"E = {E:.4e}, bound {R.MARGIN * E:.3e} of a case's output range; distances below are over that range, every element included"]
worst_s, worst_r = 0.0, 0.0
for name, inp, p, d, r, m in cases.function_cases():
    want, _s32, s64, scale = st["table"][name]
    x = torch.from_numpy(st["g"][f"in_{inp}"]).to(DEV)
    kw = dict(percentage=p, detail_level=d, restore_scale=r, blend_function=nz.utils.BLENDING_MODES[m])
    one, three = (nz.utils.pattern_break(x, route=route, **kw) for route in ("one", "three"))
    got = three.cpu().numpy().astype(np.float64)
    ds, dr = float(np.abs(got - s64).max()) / scale, float(np.abs(got - want).max()) / scale
    worst_s, worst_r = max(worst_s, ds), max(worst_r, dr)
    lines.append(f"{name}: kernel - fp64 statement {ds:.3e}  kernel - reference {dr:.3e}  routes equal {torch.equal(one, three)}")
lines.append(f"largest: kernel - fp64 statement {worst_s:.3e}, kernel - reference {worst_r:.3e}")
for name, (factor, normalized, kw) in cases.ITEMS.items():
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.PatternBreakNoise(factor, noise=chain, **kw).clone()
    torch.manual_seed(cases.ITEM_GLOBAL_SEED)
    ns = item.make_noise_sampler(torch.zeros(cases.ITEM_LATENT, device=DEV), cases.SIGMA_MIN, cases.SIGMA_MAX, seed=cases.ITEM_SEED, cpu=True,
                                 normalized=normalized)
    for i, (s, sn) in enumerate(cases.ITEM_SIGMAS):
        w = st["g"][f"item_{name}"][i].astype(np.float64)
        got = ns(torch.tensor(s), torch.tensor(sn)).cpu().numpy().astype(np.float64)
        lines.append(f"item {name} call {i} (normalized {normalized}): kernel - reference {float(np.abs(got - w).max()) / R.out_range(w):.3e}")
print("\n".join(lines))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write("\n".join(lines) + "\n")
