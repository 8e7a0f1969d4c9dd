"""Generates tests/golden/signed_rescale.npz by running the REAL reference's ``utils.normalize_to_scale_adv`` (imported through
oracle/ref_import.py) in the build container, one row at a time with ``dim=()`` as NormalizeToScaleNoise calls it (py/noise.py:1263-1286):
rows of every sign pattern against target sets that exercise the fixed targets, both data-derived ones (``max_neg >= 0``, ``min_pos < 0``),
either skipped sign and targets whose difference is not a float32 number.

    python tests/golden/make_signed_rescale_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import load_reference  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "signed_rescale.npz")
WIDTH = 12

# name -> (min_neg, max_neg, min_pos, max_pos)
CASES = {
    "fixed": (-3.0, -0.5, 0.25, 2.0),
    "auto": (-4.3, 0.0, -1.0, 3.7),        # max_neg >= 0 and min_pos < 0: both inner targets come from the data
    "auto_neg_only": (-2.0, 0.5, 0.5, 1.5),
    "auto_pos_only": (-2.0, -0.25, -0.5, 1.5),
    "skip_neg": (0.5, 1.0, 0.1, 1.2),      # min_neg >= 0: the negatives are copied
    "skip_pos": (-2.0, -0.1, 0.5, 0.0),    # max_pos <= 0: the positives are copied
    "inexact": (-0.3, -0.1, 0.1, 0.3),     # 0.3 - 0.1 is not a float32 number: the span meets the tensor rounded once
}


def rows():
    g = torch.Generator().manual_seed(4711)
    z = torch.randn(8, WIDTH, generator=g) * 2.0
    out = {"mixed": z[0], "all_positive": z[1].abs() + 0.01, "all_negative": -z[2].abs() - 0.01, "mixed_wide": z[3] * 100.0}
    zeros = z[4].clone()
    zeros[[1, 4, 7, 10]] = torch.tensor([0.0, -0.0, 0.0, 0.0])
    out["with_zeros"] = zeros
    one = torch.zeros(WIDTH)
    one[3], one[8] = 1.75, -0.625  # one value per sign: each group's denominator is eps alone
    out["one_each"] = one
    out["all_zero"] = torch.zeros(WIDTH)
    dup = z[5].clone()
    dup[6:] = dup[:6]
    out["repeated"] = dup
    return out


def main():
    ref = load_reference()
    named = rows()
    arrays = {"rows": torch.stack(list(named.values())).numpy(), "row_names": np.array(list(named)), "case_names": np.array(list(CASES))}
    for name, (min_neg, max_neg, min_pos, max_pos) in CASES.items():
        outs = [ref.utils.normalize_to_scale_adv(row.clone(), min_pos=min_pos, max_pos=max_pos, min_neg=min_neg, max_neg=max_neg, dim=())
                for row in named.values()]
        arrays[f"{name}_targets"] = np.array([min_neg, max_neg, min_pos, max_pos], dtype=np.float64)
        arrays[f"{name}_out"] = torch.stack(outs).numpy()
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    print(f"{os.path.basename(OUT)}  {len(named)} rows x {len(CASES)} cases  {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
