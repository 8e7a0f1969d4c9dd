"""One row of ``sonar_perlin_rows_f32`` restated on the host: the generate-mode Perlin streams of oracle/device_streams.py -- the lattice
drawn with (seed, stream + 1), the values with (seed, stream), element offset 0, ONE latent -- then the oracle's scale_noise in fp64.  No
kernel code is involved; tests/test_gpu_noise_rows_perlin.py compares against it."""
import math

import numpy as np
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc

NONE, FUSED = 0, 2  # SONAR_ROWS_NORM_* (include/sonar_hip.h): the two forms a Perlin row has
M64 = 2**64 - 1


def row_lattice(seed: int, stream: int, shape, iterations: int, blend_mode: str) -> np.ndarray:
    """The row's own summed lattice [C, H, W], fp64: the stream after the values' one."""
    c, h, w = shape
    return ds.perlin_lattice(seed & M64, (stream + 1) & M64, max(int(iterations), 0), c, h, w, blend_mode)


def row_raw(seed: int, stream: int, shape, iterations: int, div_fac: float, blend_mode: str) -> np.ndarray:
    """The row's values before any normalisation, fp64, flat: u / div_fac + lattice."""
    chw = math.prod(shape)
    lattice = row_lattice(seed, stream, shape, iterations, blend_mode).reshape(1, chw)
    values, _ = ds.perlin_values(seed & M64, stream & M64, lattice, chw, div_fac, chw, 0)
    return values


def row(seed: int, stream: int, shape, *, iterations: int, div_fac: float, blend_mode: str, factor: float, normalized: int,
        threshold_std_devs: float = 2.5, decisions=None) -> np.ndarray:
    """fp64 reference of one row, flat."""
    v = torch.from_numpy(row_raw(seed, stream, shape, iterations, div_fac, blend_mode).copy())
    return orc.scale_noise(v, factor, normalized=bool(normalized), threshold_std_devs=threshold_std_devs, decisions=decisions).numpy()
