"""Generates tests/golden/freeu_edges.npz by running the REAL reference's FreeUExtremeConfig.apply (imported through oracle/ref_import.py)
on the CPU, in the build container only:

    python tests/golden/make_freeu_edges_golden.py

For every plane size of tests/freeu_edge_refs.FREEU_SWEEP + FREEU_FIXED the reference runs in float32 on the input and the filter the GPU
test uses (fused_inputs; the filter is put into the reference's filter cache, where a hit wins over the config's own), with the hidden-mean
map and a lerp blend on channels 1 and 2 of three.  Recorded: ONLY E_size = the largest distance between the reference's fp32 output and
the fp64 statement, as a fraction of the statement's range, per size -- what the reference's own fp32 FFT costs at 18 x 1008 or 132 x 288,
which tests/golden/freeu_extreme.npz (8 x 8 ... 16 x 16) cannot say.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import load_reference  # noqa: E402
from tests import freeu_edge_refs as F  # noqa: E402
from tests import freeu_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = load_reference()
    fx = importlib.import_module("sonar_ref.nodes.freeu_extreme")
    sizes = F.FREEU_SWEEP + F.FREEU_FIXED
    errs = []
    for hw in sizes:
        x, filt = F.fused_inputs(hw)
        cfg = fx.FreeUExtremeConfig(target="both", stage_1=True, sonar_power_filter_opt=ref.powernoise.PowerFilter(), **F.FUSED_REF_KW)
        xin = torch.from_numpy(x.copy())
        held = torch.from_numpy(filt)
        cache = {(0, xin.shape[-2:]): held}
        got = cfg.apply(0, xin, cache)
        assert got is xin and cache[(0, xin.shape[-2:])] is held and got.dtype == torch.float32
        st = R.apply_ref(x, filt, **F.FUSED_REF_KW)
        assert np.array_equal(got[:, 0].numpy(), x[:, 0]) and not np.array_equal(got[:, 1:].numpy(), x[:, 1:])
        errs.append(R.distance(got.numpy(), st))
        print(f"{hw[0]:4d} x {hw[1]:4d}  E_size = {errs[-1]:.3e}")
    path = os.path.join(OUT, "freeu_edges.npz")
    np.savez_compressed(path, sizes=np.array(sizes, dtype=np.int32), e_size=np.array(errs, dtype=np.float64))
    print(f"freeu_edges.npz  {os.path.getsize(path)} bytes; E_size {min(errs):.3e} ... {max(errs):.3e}")


if __name__ == "__main__":
    main()
