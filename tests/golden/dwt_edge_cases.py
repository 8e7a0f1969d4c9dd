"""Case table for the per-pass 2-D DWT kernels and the 1-D DWT kernels at their edges.  Shared by
tests/golden/make_dwt_edge_golden.py (PyWavelets -> tests/golden/dwt_edges.npz), tests/test_dwt_edges_cpu.py (oracle against that
fixture) and tests/test_gpu_dwt_kernel_edges.py (kernels against both).  Data and small helpers only: numpy, no pywt, no torch.

A case is one single-level transform: ``{"id", "group", "dim", "wave", "mode", "shape"}``.  Its inputs come from a seed derived from
the id, so the fixture stores expected outputs only:

* the analysis input ``x`` [2, 3, *shape] and, independent of it, synthesis inputs of the analysis output's size (``lo``, ``hi``
  [2, 3, k] in 1-D; ``ll`` [2, 3, h, w], ``hi`` [2, 3, 3, h, w] in 2-D).  Every value is a float32 value widened to float64, so one
  PyWavelets result serves the fp64 and the fp32 kernels.
* the fixture holds PyWavelets' results for row / plane [0, 0] only.  1-D: the coefficient rows and the reconstruction in full.
  2-D: ``probe()`` of each band and of the reconstruction -- the plane contracted along W with fixed weights in [0.5, 2.5], one
  number per row: a wrong coefficient anywhere moves its row's number, and the file stays a fortieth of the full planes' size
  (the planes are mostly padding: a 64-tap filter turns 3 x 31 samples into four bands of 33 x 47).

Groups (the edge each stands at; the module docstring of the GPU test names the test of each):
  E1   extension wrap: all six modes, n in {1, 2, 3, F/2 - 1, F/2, F - 1, F, F + 1, 2F + 1}, rows of n and planes (n, m)
  E2   periodization: odd n, n = 1, synthesis with F > 2k coefficients
  E3   the 1-D kernel's interior / border switch: L = 4F + 3, 4F + 4
  E4   crop arguments: the synthesis inputs of these cases get a surplus row / column / sample in the test
  LONG the 13 wavelets of 66 .. 102 taps, symmetric, a (24, 20) plane and a row of 50
E5 (grid-stride loops) and E7 (multi-level through ``Wavelet``) are too large for a fixture and are compared with the oracle."""
from __future__ import annotations

import zlib

import numpy as np

MODES = ("zero", "symmetric", "reflect", "periodization", "periodic", "constant")
# wave -> filter length; db4 and shorter take the tile kernels in 2-D (the control), 22 taps is the first per-pass length
E1_WAVES = {"haar": 2, "db2": 4, "db4": 8, "db11": 22, "sym20": 40, "dmey": 62, "db32": 64}
E2_WAVES = {"db4": 8, "db11": 22, "coif10": 60, "db32": 64}
E3_WAVES = {"db4": 8, "db11": 22}
E4_WAVES = {"db4": 8, "db11": 22, "dmey": 62}
E4_MODES = ("symmetric", "periodization", "zero")
LONG_WAVES = {**{f"db{i}": 2 * i for i in range(33, 39)}, **{f"coif{i}": 6 * i for i in range(11, 18)}}
BATCH = (2, 3)
SENTINEL = 12345.0  # finite garbage for the surplus of an oversized approximation band


def out_len(n: int, flen: int, mode: str) -> int:
    return (n + 1) // 2 if mode == "periodization" else (n + flen - 1) // 2


def rec_len(k: int, flen: int, mode: str) -> int:
    return 2 * k if mode == "periodization" else 2 * k - flen + 2


def e1_lengths(flen: int):
    return sorted({n for n in (1, 2, 3, flen // 2 - 1, flen // 2, flen - 1, flen, flen + 1, 2 * flen + 1) if n >= 1})


def e2_lengths(flen: int):
    """odd lengths, 1, and lengths whose k = (n + 1) / 2 coefficients leave F > 2k (taps fold more than once in synthesis)"""
    return sorted({1, 2, 5, 7, flen // 2 - 3, flen + 3})


def _planes(lengths):
    """(n, m): m the entry half a list further on, so that rows and columns wrap differently and H != W"""
    k = len(lengths)
    step = max(1, k // 2)
    return [(n, lengths[(i + step) % k]) for i, n in enumerate(lengths) if lengths[(i + step) % k] != n]


def _case(group, dim, wave, flen, mode, shape):
    ident = f"{group}-{dim}d-{wave}-{mode}-" + "x".join(map(str, shape))
    # PyWavelets 1.1.1 never returns from a reflect extension of one sample (its period 2n - 2 is 0): those cases have no fixture entry;
    # the oracle and the kernels repeat the sample, which is what reflect gives at every n > 1 when the samples are equal
    return {"id": ident, "group": group, "dim": dim, "wave": wave, "flen": flen, "mode": mode, "shape": tuple(shape),
            "pywt": not (mode == "reflect" and 1 in shape)}


def _build():
    out = []
    for wave, flen in E1_WAVES.items():
        for mode in MODES:
            ns = e1_lengths(flen)
            out += [_case("E1", 1, wave, flen, mode, (n,)) for n in ns]
            out += [_case("E1", 2, wave, flen, mode, hw) for hw in _planes(ns)]
    for wave, flen in E2_WAVES.items():
        ns = e2_lengths(flen)
        out += [_case("E2", 1, wave, flen, "periodization", (n,)) for n in ns]
        out += [_case("E2", 2, wave, flen, "periodization", hw) for hw in _planes(ns)]
    for wave, flen in E3_WAVES.items():
        for mode in MODES:
            out += [_case("E3", 1, wave, flen, mode, (n,)) for n in (4 * flen + 3, 4 * flen + 4)]
    for wave, flen in E4_WAVES.items():
        for mode in E4_MODES:
            out += [_case("E4", 1, wave, flen, mode, (45,)), _case("E4", 2, wave, flen, mode, (23, 30))]
    for wave, flen in LONG_WAVES.items():
        out += [_case("LONG", 1, wave, flen, "symmetric", (50,)), _case("LONG", 2, wave, flen, "symmetric", (24, 20))]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES = _build()
GROUPS = ("E1", "E2", "E3", "E4", "LONG")


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def inputs(case):
    """(x, synthesis inputs): x [2, 3, *shape]; (lo, hi) [2, 3, k] or (ll [2, 3, h, w], hi [2, 3, 3, h, w]).  O(1) data off zero mean."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    x = _f32(rng.standard_normal(BATCH + case["shape"]) + 0.25)
    ks = tuple(out_len(n, case["flen"], case["mode"]) for n in case["shape"])
    lo = _f32(rng.standard_normal(BATCH + ks) + 0.25)
    hi = _f32(rng.standard_normal(BATCH + ((3,) if case["dim"] == 2 else ()) + ks))
    return x, (lo, hi)


def probe(plane):
    """[..., h, w] -> [..., h]: every row contracted with weights 1.5 + cos(0.7 j + 0.3)"""
    return plane @ (1.5 + np.cos(0.7 * np.arange(plane.shape[-1]) + 0.3))


def fixture_keys(case):
    return tuple(f"{case['id']}__{k}" for k in ("lo", "hi", "rec"))


def load_fixture(path):
    """dwt_edges.npz (``keys``, ``sizes``, flat ``values``) -> {key: fp64 vector}; a 2-D case's ``__hi`` is its three probes end to end"""
    z = np.load(path, allow_pickle=False)
    ends = np.cumsum(z["sizes"])
    return {k.decode(): z["values"][e - s:e] for k, s, e in zip(z["keys"], z["sizes"], ends)}


# ------------------------------------------------------------------------------------------------ beyond the fixture
# E5: the smallest counts at which a thread of each kernel takes a second trip round its grid-stride loop: grid_for caps the grid at
# kMaxGrid = 2048 blocks of kBlock = 256 threads, so more than 524288 work items.  (batch, wave, mode, shape); the 2-D plane is wider
# than the tile kernels' 64 KiB LDS tile in both precisions (W > 1020 forward, w > 512 inverse), which sends 4 taps down the per-pass route.
GRID_ITEMS = 2048 * 256
E5_1D = {"batch": (257, 8), "wave": "db2", "mode": "symmetric", "shape": (510,)}      # 2056 rows x 256 coefficients; x 510 samples back
E5_2D = {"batch": (240, 2), "wave": "db2", "mode": "symmetric", "shape": (4, 1100)}   # 480 planes: rows 480 x 4 x 551, columns 480 x 3 x 551

# E7: (wave, mode, level); 2-D on 33 x 47, 1-D on 1601 samples, batch (2, 3)
E7_2D = (("db11", "symmetric", 3), ("sym20", "reflect", 2), ("coif10", "periodization", 3))
E7_1D = E7_2D + (("dmey", "zero", 2),)
E7_PLANE, E7_ROW = (33, 47), (1601,)


def big_inputs(tag, batch, shape):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return _f32(rng.standard_normal(tuple(batch) + tuple(shape)) + 0.25)
