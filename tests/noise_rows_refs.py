"""One row of ``sonar_philox_rows_f32`` restated on the host: the generate-mode stream of oracle/device_streams.py for (seed, stream id,
element offset 0), then the oracle's scale_noise in fp64.  No kernel code is involved; tests/test_gpu_noise_rows.py compares against it."""
import numpy as np
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc

NONE, SCALE_NOISE, FUSED = 0, 1, 2  # SONAR_ROWS_NORM_* (include/sonar_hip.h)


def row_draw(uniform: bool, seed: int, stream: int, inner: int, sub: float = 0.0, mul: float = 1.0, add: float = 0.0) -> np.ndarray:
    """The row's values before any normalisation, fp64 (the uniform words are exact; the affine map and Box-Muller run in fp64)."""
    seed, stream = seed & (2**64 - 1), stream & (2**64 - 1)
    if uniform:
        sub, mul, add = (float(np.float32(v)) for v in (sub, mul, add))  # the kernel's arguments are floats
        return (ds.uniform_fill(seed, stream, inner, 0).astype(np.float64) - sub) * mul + add
    return np.asarray(ds.normal_fill(seed, stream, inner, 0), dtype=np.float64)


def row_moments(values: np.ndarray):
    """(mean, unbiased std, threshold) as scale_noise sees them."""
    n = values.size
    sd = float(values.std(ddof=1)) if n > 1 else float("nan")
    return float(values.mean()), sd, 2.5 / np.sqrt(n)


def row(uniform: bool, seed: int, stream: int, inner: int, factor: float, normalized: int, *, sub=0.0, mul=1.0, add=0.0,
        threshold_std_devs: float = 2.5, decisions=None) -> np.ndarray:
    """fp64 reference of one row.  SCALE_NOISE and FUSED differ only in how the device rounds the quotient: one reference for both."""
    v = torch.from_numpy(row_draw(uniform, seed, stream, inner, sub, mul, add).copy())
    return orc.scale_noise(v, factor, normalized=bool(normalized), threshold_std_devs=threshold_std_devs, decisions=decisions).numpy()
