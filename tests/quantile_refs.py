"""A plain CPU restatement of the reference's utils.quantile_normalize (py/utils.py:123-449) for all 43 strategies, with the per-row
statistics the device kernels also report.  tests/test_quantile_refs_cpu.py pins it to the reference's recorded outputs
(tests/golden/quantile_filter.npz); the GPU tests then use it at shapes the reference cannot reach (torch.quantile stops at 2^24 values) or
is too slow at.

What is restated, and how:
  * the rows, the "centered" proxy, the fp32 threshold ``nq = quantile(|p|) * nq_fac + eps`` and the outlier test ``|p| > nq`` in fp32,
    exactly as the reference forms them; the order statistics come from a per-row sort and torch.quantile's fp32 rank split
    (``hip_lib.quantile_rank`` has its own CPU test), never from torch.quantile;
  * every strategy in float64 from the fp32 ``p`` and ``nq``, written as the reference's handlers write them (``math.pi`` arithmetic for the
    waves and atan, ``1 / count`` for replace*), then the centered back-mapping and the sign-preserving power in float64; only the waves'
    argument ``p * multiplier`` and replace*'s average of candidates keep the reference's fp32 roundings (see there);
  * the mode as the smallest of the most frequent rounded finite values (np.unique's sorted counts): torch.mode documents no tie order.
"""
import math
from typing import NamedTuple

import numpy as np
import torch


class RowStats(NamedTuple):
    """Per row: the fp32 threshold, max|x| (fp32), and the strategy's second statistic in float64 (0 where it has none): nq / max|p| for
    scale_down, the float64 mean, the lower median, the mode (NaN for a row without a finite value)."""
    nq: torch.Tensor
    maxabs: torch.Tensor
    second: torch.Tensor


def _rows(x, dim, flatten):
    """(rows [R, L] float32, function putting [R, L] back into x's shape)."""
    if dim is None:
        return x.reshape(1, -1), lambda r: r.reshape(x.shape)
    if flatten and x.ndim > 1:
        return x.reshape(int(np.prod(x.shape[:dim])), -1), lambda r: r.reshape(x.shape)
    xt = x.movedim(dim, -1)
    shape_t = xt.shape
    return xt.reshape(-1, x.shape[dim]), lambda r: r.reshape(shape_t).movedim(-1, dim)


def rank_split(q, n):
    """(lo, frac) of torch.quantile's linear interpolation over n values: rank = q * (n - 1) in fp32."""
    rank = torch.tensor(abs(q), dtype=torch.float32) * (n - 1)
    lo = int(torch.floor(rank))
    return lo, rank - lo


def row_mode(p, decimals):
    """[R, 1] float64: per row the smallest of the most frequent values of round(p, decimals) over the finite values (NaN: none)."""
    r = torch.round(p, decimals=decimals).numpy()
    out = np.full((r.shape[0], 1), np.nan)
    for i, row in enumerate(r):
        vals, counts = np.unique(row[np.isfinite(row)], return_counts=True)
        if vals.size:
            out[i, 0] = vals[np.argmax(counts)]  # (sorted values, the first maximum: the smallest of equals)
    return torch.from_numpy(out)


WAVES = {f"{fn}{'_wrong' if wrong else ''}{suffix}": (fn, wrong, pi_factor, keep)
         for fn in ("sin", "cos") for wrong in (False, True) for suffix, pi_factor, keep in (("", 0.5, False), ("_wholepi", 1.0, False),
                                                                                           ("_keepsign", 0.5, True))}


def _replace_args(strategy):
    """(count, count_flipping, keep_sign, avoid_sign) of a replace* name."""
    parts = strategy.split("_")
    assert parts[0] == "replace" and set(parts[1:]) <= {"2pt", "3pt", "flip", "keepsign", "avoidsign"}, strategy
    return 3 if "3pt" in parts else 2 if "2pt" in parts else 1, "flip" in parts, "keepsign" in parts, "avoidsign" in parts


def _once(x, q, dim, flatten, strategy, pow_fac, nq_fac, eps):
    rows, back = _rows(x, dim, flatten)
    centered = q < 0
    maxabs = rows.abs().amax(dim=1, keepdim=True)
    p = rows.sign() * (maxabs - rows.abs()) if centered else rows
    srt = p.abs().sort(dim=1).values
    n = rows.shape[1]
    lo, frac = rank_split(q, n)
    hi = min(lo + 1, n - 1)
    nq = torch.lerp(srt[:, lo:lo + 1], srt[:, hi:hi + 1], frac.reshape(1, 1).expand(rows.shape[0], 1))
    nq = nq * torch.tensor(nq_fac, dtype=torch.float32) + torch.tensor(eps, dtype=torch.float32)
    p64, nq64 = p.double(), nq.double()
    anq = nq64.abs()
    outl = p.abs() > nq
    second = torch.zeros(rows.shape[0], 1, dtype=torch.float64)
    if strategy == "clamp":
        o = torch.minimum(torch.maximum(p64, -nq64), nq64)
    elif strategy == "scale_down":
        mv = p.abs().amax(dim=1, keepdim=True).clamp(min=1e-6).double()
        second = nq64 / mv
        o = torch.where(outl, p64 * second, p64)
    elif strategy == "tanh":
        o = p64.tanh() * anq
    elif strategy == "tanh_outliers":
        o = torch.where(outl, p64.tanh() * anq, p64)
    elif strategy == "sigmoid_keepsign":
        o = (p64.sigmoid() * anq).copysign(p64)
    elif strategy == "sigmoid":
        o = p64.sigmoid() * (anq * 2) - anq
    elif strategy == "sigmoid_outliers":
        o = torch.where(outl, (p64.sigmoid() * anq).copysign(p64), p64)
    elif strategy in WAVES:
        fn, wrong, pi_factor, keep = WAVES[strategy]
        # the multiplier and the wave's argument are fp32 tensor arithmetic in the reference, and the argument's rounding is no detail:
        # it reaches several periods, and the square root that follows magnifies an error next to a zero of the wave
        mult = 1.0 / ((math.pi * pi_factor) / nq) if wrong else 1.0 / (nq / (math.pi * pi_factor))
        o = getattr(torch, fn)(p.mul(mult).double()) * nq64
        if keep:
            o = o.copysign(p64)
    elif strategy == "atan":
        o = p64.atan() * (anq / (math.pi / 2))
    elif strategy == "tenth":
        o = torch.where(outl, p64 * 0.1, p64)
    elif strategy == "half":
        o = torch.where(outl, p64 * 0.5, p64)
    elif strategy == "zero":
        o = torch.where(outl, torch.zeros_like(p64), p64)
    elif strategy == "reverse_zero":
        o = torch.where(p.abs() >= nq, p64, torch.zeros_like(p64))
    elif strategy in ("mean", "median", "mode_1dec", "mode_2dec"):
        if strategy == "mean":
            second = p64.mean(dim=1, keepdim=True)
        elif strategy == "median":
            second = p.sort(dim=1).values[:, (n - 1) // 2:(n - 1) // 2 + 1].double()  # torch.median: the lower of two middle values
        else:
            second = row_mode(p, 1 if strategy == "mode_1dec" else 2)
        o = torch.where(outl, second, p64)
    else:
        # _quantile_norm_replace: the mask, the candidates and the rolls run over the whole tensor in memory order
        count, flipping, keep_sign, avoid_sign = _replace_args(strategy)
        pf = back(p).reshape(-1)
        mask = back(~outl).reshape(-1)
        cand = pf[mask]
        if cand.numel() == 0:
            raise ZeroDivisionError("no candidate")
        idx = torch.arange(pf.numel()) % cand.numel()
        rep = cand[idx]
        if count >= 2:
            # the average of the rolled candidates keeps the reference's fp32 roundings: its terms cancel, and the square root that
            # follows magnifies their rounding error next to zero (4e-6 absolute at |average| = 1e-6) beyond any tolerance on the output
            rep = rep * (1.0 / count)
            for i in range(1, count):
                rep += cand[torch.roll(idx, i if not flipping or i % 2 == 0 else -i, dims=(-1,))] * (1.0 / count)
        rep = rep.double()
        if keep_sign or avoid_sign:
            rep = rep.copysign(-pf.double() if avoid_sign else pf.double())
        o = torch.where(mask, pf.double(), rep)
        o = _rows(o.reshape(x.shape), dim, flatten)[0]
    if centered:
        o = o.sign() * (maxabs.double() - o.abs())
    if pow_fac not in (0.0, 1.0):
        o = o.abs().pow(pow_fac).copysign(o)
    return back(o), RowStats(nq.reshape(-1), maxabs.reshape(-1), second.reshape(-1))


def restate(x, q, dim, flatten, strategy, pow_fac=0.5, nq_fac=1.0, eps=1e-8):
    """(float64 output in x's shape, RowStats) for an fp32 CPU tensor.  A list of quantiles filters repeatedly, through fp32 like the
    reference; the statistics are those of the last pass."""
    if isinstance(q, (tuple, list)):
        out, stats = x.double(), None
        for one in q:
            out, stats = restate(out.float(), one, dim, flatten, strategy, pow_fac, nq_fac, eps)
        return out, stats
    return _once(x, q, dim, flatten, strategy, pow_fac, nq_fac, eps)


def _restated(x, q, dim, flatten, strategy, pow_fac=0.5, nq_fac=1.0, eps=1e-8):
    return restate(x, q, dim, flatten, strategy, pow_fac, nq_fac, eps)[0]
