#!/usr/bin/env python3
"""PyWavelets 1.1.1 results for the cases of tests/golden/dwt_edge_cases.py (the arithmetic the reference reaches through
pytorch_wavelets).  Run with the interpreter that has pywt:   /opt/conda/bin/python3.9 tests/golden/make_dwt_edge_golden.py
Writes tests/golden/dwt_edges.npz: per case ``<id>__lo`` / ``__hi`` (pywt.dwt, or pywt.dwt2 as cA and (cH, cV, cD)) and ``__rec``
(pywt.idwt / idwt2 of the case's own synthesis inputs), row / plane [0, 0] only, fp64; 2-D results through ``probe()``.
Single-level calls only, so nothing here depends on pywt's level bookkeeping."""
import os
import sys
import warnings

import numpy as np
import pywt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dwt_edge_cases as ec  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dwt_edges.npz")


def results(case):
    x, (lo, hi) = ec.inputs(case)
    wave, mode = case["wave"], case["mode"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if case["dim"] == 1:
            a, d = pywt.dwt(x[0, 0], wave, mode=mode)
            rec = pywt.idwt(lo[0, 0], hi[0, 0], wave, mode=mode)
            return a, d, rec
        ca, (ch, cv, cd) = pywt.dwt2(x[0, 0], wave, mode=mode)
        rec = pywt.idwt2((lo[0, 0], tuple(hi[0, 0])), wave, mode=mode)
    return ec.probe(ca), ec.probe(np.stack([ch, cv, cd])), ec.probe(rec)


def main():
    data = {}
    for case in ec.CASES:
        if not case["pywt"]:
            continue
        for key, val in zip(ec.fixture_keys(case), results(case)):
            data[key] = np.ascontiguousarray(val, dtype=np.float64)
    # one flat array and an index: 2000 separate members would cost more in zip headers than in values
    np.savez_compressed(OUT, keys=np.array(list(data), dtype="S"), sizes=np.array([v.size for v in data.values()], dtype=np.int32),
                        values=np.concatenate([v.ravel() for v in data.values()]))
    print(OUT, len(ec.CASES), "cases", os.path.getsize(OUT) // 1024, "KiB, pywt", pywt.__version__)


if __name__ == "__main__":
    main()
