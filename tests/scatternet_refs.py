"""fp64 numpy statement of the scattering layer and of ScatternetFilteredNoiseGenerator's window (test side only; the product does not import
this).  pytorch_wavelets is absent here and in the reference tree: **parity unpinned**.  The layer is Cotter's ScatLayer as
pytorch_wavelets documents it, stated on the DTCWT oracle: the level-1 transform, the smoothed magnitude sqrt(re^2 + im^2 + b^2) - b of
the six oriented bands, the 2 x 2 mean of the low-pass, concatenated band-major ([B, 7, C, h, w] viewed as [B, 7 C, h, w])."""
import math

import numpy as np

from oracle import dtcwt_oracle as O

ANGLES = (15, 45, 75, 105, 135, 165)


def scat_layer(x, biort: str = "near_sym_a", magbias: float = 1e-2):
    """x [B, C, H, W] -> [B, 7 C, ceil(H / 2), ceil(W / 2)] in fp64; channel band * C + c, band 0 the pooled low-pass."""
    x = np.asarray(x, dtype=np.float64)
    yl, yh = O.forward(x, 1, biort)  # odd sides are extended by their last row / column in there
    ll = 0.25 * (yl[..., 0::2, 0::2] + yl[..., 0::2, 1::2] + yl[..., 1::2, 0::2] + yl[..., 1::2, 1::2])
    bands = yh[0]  # [B, C, 6, h, w, 2]
    mag = np.sqrt(bands[..., 0] ** 2 + bands[..., 1] ** 2 + magbias**2) - magbias
    z = np.concatenate((ll[:, None], np.moveaxis(mag, 2, 1)), axis=1)  # [B, 7, C, h, w]
    return z.reshape(z.shape[0], 7 * z.shape[2], *z.shape[3:])


def scat_stack(x, n: int, biort: str = "near_sym_a", magbias: float = 1e-2):
    """torch.nn.Sequential of n ScatLayers (py/noise_generation.py:2068-2073)."""
    for _ in range(n):
        x = scat_layer(x, biort, magbias)
    return np.asarray(x, dtype=np.float64)


def scatter(noise, order: int, per_channel: bool, biort: str = "near_sym_a", magbias: float = 1e-2):
    """py/noise_generation.py:2144-2155: the scattered tensor, [C, B, 7^n, h, w] per channel and [1, B, 7^n C, h, w] otherwise."""
    noise = np.asarray(noise, dtype=np.float64)
    n = abs(order)
    if per_channel:  # :2146-2152
        return np.stack([scat_stack(noise[:, c:c + 1], n, biort, magbias) for c in range(noise.shape[1])], axis=0)
    return scat_stack(noise, n, biort, magbias)[None]  # :2155


def window(z, *, shape, output_mode: str = "channels_adjusted", output_offset: float = 0.0, order: int = 1, per_channel: bool = False):
    """py/noise_generation.py:2156-2193 on the scattered tensor ``z`` of ``scatter``; ``shape`` is the latent's [B, C, H, W].  Returns what
    the generator returns; raises ValueError where the reference's final reshape does."""
    batch, channels, height, width = shape
    scaled = output_mode.endswith("_scaled")                       # :2106
    adjusted = scaled or output_mode.endswith("_adjusted")         # :2107
    n = abs(order)                                                 # :2108
    mode = output_mode.split("_", 1)[0] if adjusted else output_mode  # :2110-2112
    base_channels = 1 if per_channel else channels                 # :2156
    if mode == "flat":                                             # :2157-2161
        z = z.reshape(z.shape[0], batch, -1)
        initial_size = math.prod(shape[(2 if per_channel else 1):])
    elif adjusted:                                                 # :2162-2163
        initial_size = base_channels
    else:                                                          # :2164-2165
        initial_size = base_channels * ((2**n) ** 2)
    increment = 1 if mode == "flat" else base_channels            # :2166
    out_size = z.shape[2]                                          # :2167
    offset_size = (out_size - initial_size) / increment            # :2168
    if output_offset == 0 or abs(output_offset) >= 1:              # :2170-2173
        output_offset = int(output_offset)
        if output_offset < 0:
            output_offset = (offset_size + 1) + output_offset
    else:                                                          # :2174-2177
        if output_offset < 0:
            output_offset += 1.0
        output_offset = round(offset_size * output_offset)
    base_idx = int(output_offset * increment)                      # :2178
    z = z[:, :, base_idx:base_idx + initial_size]                  # :2182
    if per_channel:                                                # :2184-2186
        z = np.moveaxis(z.squeeze(2) if z.shape[2] == 1 else z, 0, 1)
    else:
        z = z[0]
    if mode == "channels":                                         # :2188-2189
        z = z[..., :height, :width]
    return np.ascontiguousarray(z.reshape(shape))                  # :2193


def tolerance(biort: str, max_abs: float) -> float:
    """The standard running-error bound of two passes of L-term fp32 dot products plus the magnitude's six operations, in units of the
    input's size: (L0 + L1 + 6) 2^-24 ||h||_1^2 max|x|, ||h||_1 the larger of the two filters' absolute sums (the gain of either pass)."""
    h0o, _g0o, h1o, _g1o = O.biort(biort)
    norm = max(float(np.abs(h0o).sum()), float(np.abs(h1o).sum()))
    return (len(h0o) + len(h1o) + 6) * 2.0**-24 * norm**2 * max_abs


def stack_tolerance(x, n: int, biort: str = "near_sym_a", magbias: float = 1e-2) -> float:
    """The bound for n layers in sequence: e_i = G e_(i-1) + tolerance(max|input of layer i|).  G = 2 ||h||_1^2 bounds what a layer does
    to an error of its input: the two filter passes by ||h||_1 each; a quad combination (p +- q) / sqrt 2 by sqrt 2; the magnitude is
    1-Lipschitz in (re, im), another sqrt 2 from the two components; the 2 x 2 mean by 1."""
    h0o, _g0o, h1o, _g1o = O.biort(biort)
    gain = 2.0 * max(float(np.abs(h0o).sum()), float(np.abs(h1o).sum())) ** 2
    z, err = np.asarray(x, dtype=np.float64), 0.0
    for _ in range(n):
        err = gain * err + tolerance(biort, float(np.abs(z).max()))
        z = scat_layer(z, biort, magbias)
    return err
