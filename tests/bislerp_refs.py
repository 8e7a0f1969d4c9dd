"""The statement of bislerp that the tests hold csrc/bislerp.hip, hip_lib's table builder and utils.bislerp to: torch on the CPU, fp64 by
default (``dtype=torch.float32`` runs the same formulae in fp32: the yardstick of the kernel's tolerance).

The reference reaches bislerp through ``comfy.utils.common_upscale(samples, width, height, "bislerp", None)`` (py/utils.py:58-67), i.e.
ComfyUI's ``bislerp(samples, width, height)``.  ComfyUI is neither vendored by the reference nor installed here, so there is nothing to
capture goldens from: **parity unpinned**.  What is written down here is the definition the project builds:

    axis tables, a function of (old, new) only
        c1f   = F.interpolate(arange(old, float32).reshape(1, 1, 1, old), size=(1, new), mode="bilinear")      # align_corners=False
        ratio = c1f - floor(c1f);  c1 = int64(c1f)
        c2    = int64(F.interpolate((arange(old) + 1, last element lowered by 1).float()..., size=(1, new), mode="bilinear"))
    slerp(b1, b2, r) on C-vectors (norms and dot over the channel axis)
        u = b / |b| (a vector of norm exactly 0 gives u = 0);  dot = sum(u1 u2);  om = acos(dot);  so = sin(om)
        res = ((sin((1 - r) om) / so) u1 + (sin(r om) / so) u2) * (|b1| (1 - r) + |b2| r)
        dot > 1 - 1e-5: res = b1;   dot < 1e-5 - 1: res = b1 (1 - r) + b2 r
    width pass   T[n, :, y, X] = slerp(S[n, :, y, c1w[X]], S[n, :, y, c2w[X]], ratio_w[X])
    height pass  O[n, :, Y, X] = slerp(T[n, :, c1h[Y], X], T[n, :, c2h[Y], X], ratio_h[Y])

The function jumps at the two ``dot`` thresholds (ComfyUI's behaviour, reproduced).  ``bislerp`` therefore also returns, per output pixel,
the three dots it took (the width-pass dots of rows c1h[Y] and c2h[Y], and the height-pass dot) so that a comparison can leave out pixels
that sit on a threshold (``near_threshold``)."""
import torch
import torch.nn.functional as F

HI, LO = 1.0 - 1e-5, 1e-5 - 1.0
BAND = 2e-6          # |dot - threshold| below this: the pixel is left out of a comparison
LEFT_OUT_CAP = 0.005  # at most this share of a case's pixels

# (h, w) -> (H, W) of the kernel cases; N = 2, every C of CHANNELS
SIZES = (((1, 1), (3, 5)), ((1, 5), (4, 9)), ((2, 3), (7, 5)), ((9, 7), (4, 3)), ((6, 6), (6, 6)), ((40, 24), (64, 72)))
CHANNELS = (1, 3, 4, 16, 20)
BATCH = 2
ACC_SCALE = 0.7


def axis_tables(old: int, new: int):
    """(c1 int64 [new], c2 int64 [new], ratio fp32 [new])"""
    c1f = F.interpolate(torch.arange(old, dtype=torch.float32).reshape(1, 1, 1, old), size=(1, new), mode="bilinear")
    ratio = c1f - c1f.floor()
    c2 = torch.arange(old).reshape(1, 1, 1, old) + 1
    c2[:, :, :, -1] -= 1
    c2f = F.interpolate(c2.float(), size=(1, new), mode="bilinear")
    return c1f.to(torch.int64).reshape(new), c2f.to(torch.int64).reshape(new), ratio.reshape(new)


def slerp(b1, b2, r, mutated=False):
    """b1, b2 [M, C], r [M, 1] -> (res [M, C], dot [M]).  ``mutated``: the lerp branch where slerp belongs (the negative control)."""
    dt = b1.dtype
    n1, n2 = b1.norm(dim=-1, keepdim=True), b2.norm(dim=-1, keepdim=True)
    u1, u2 = b1 / n1, b2 / n2
    u1[n1.expand_as(u1) == 0.0] = 0.0
    u2[n2.expand_as(u2) == 0.0] = 0.0
    dot = (u1 * u2).sum(1)
    om = torch.acos(dot)
    so = torch.sin(om)
    res = (torch.sin((1.0 - r.squeeze(1)) * om) / so).unsqueeze(1) * u1 + (torch.sin(r.squeeze(1) * om) / so).unsqueeze(1) * u2
    res = res * (n1 * (1.0 - r) + n2 * r)
    lerp = b1 * (1.0 - r) + b2 * r
    if mutated:
        res = lerp.clone()
    hi, lo = torch.tensor(HI, dtype=dt), torch.tensor(LO, dtype=dt)  # (an fp32 comparison sees the thresholds rounded to fp32)
    res[dot > hi] = b1[dot > hi]
    res[dot < lo] = lerp[dot < lo]
    return res, dot


def bislerp(samples, width: int, height: int, dtype=torch.float64, mutated=False):
    """(O [N, C, height, width] in ``dtype``, dots [N, 3, height, width] in ``dtype``)"""
    S = samples.detach().cpu().to(dtype)
    N, C, h, w = S.shape
    c1w, c2w, rw = axis_tables(w, width)
    c1h, c2h, rh = axis_tables(h, height)
    rw, rh = rw.to(dtype), rh.to(dtype)

    def rows(t):  # [N, C, a, b] -> [N * a * b, C]
        return t.movedim(1, -1).reshape(-1, C)

    r = rw.reshape(1, 1, width).expand(N, h, width).reshape(-1, 1)
    T, dw = slerp(rows(S[:, :, :, c1w]), rows(S[:, :, :, c2w]), r, mutated)
    T = T.reshape(N, h, width, C).movedim(-1, 1)
    dw = dw.reshape(N, h, width)
    r = rh.reshape(1, height, 1).expand(N, height, width).reshape(-1, 1)
    O, dh = slerp(rows(T[:, :, c1h]), rows(T[:, :, c2h]), r, mutated)
    O = O.reshape(N, height, width, C).movedim(-1, 1).contiguous()
    dots = torch.stack([dw[:, c1h], dw[:, c2h], dh.reshape(N, height, width)], dim=1)
    return O, dots


def near_threshold(dots):
    """[N, H, W] bool: any of the pixel's three dots within BAND of a threshold"""
    d = dots.double()
    return (((d - HI).abs() < BAND) | ((d - LO).abs() < BAND)).any(dim=1)


def source_scale(samples, width: int, height: int):
    """[N, H, W] fp64: the sum of the norms of the four source vectors an output pixel reads (what errors are relative to)"""
    S = samples.detach().cpu().double()
    _, _, h, w = S.shape
    c1w, c2w, _ = axis_tables(w, width)
    c1h, c2h, _ = axis_tables(h, height)
    n = S.norm(dim=1)  # [N, h, w]
    return n[:, c1h][:, :, c1w] + n[:, c1h][:, :, c2w] + n[:, c2h][:, :, c1w] + n[:, c2h][:, :, c2w]


def rel_error(got, want, scale, keep=None):
    """max over the kept pixels of max_c |got - want| / scale (a pixel whose four source vectors are all zero counts with its absolute error)"""
    err = (got.detach().cpu().double() - want.double()).abs().amax(dim=1)
    err = err / torch.where(scale > 0, scale, torch.ones_like(scale))
    if keep is not None:
        err = err[keep]
    return float(err.max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the kernel cases
def case_seed(index: int, C: int) -> int:
    return 7100 + 37 * index + C


def case_input(index: int, C: int):
    """(samples [N, C, h, w] fp32, base [N, C, H, W] fp32 -- what the accumulating form adds onto, (H, W))"""
    (h, w), (H, W) = SIZES[index]
    g = torch.Generator().manual_seed(case_seed(index, C))
    return torch.randn(BATCH, C, h, w, generator=g), torch.randn(BATCH, C, H, W, generator=g), (H, W)


_measured = {}


def fp32_statement_error():
    """The statement in fp32 against the statement in fp64 over every kernel case, plain and accumulated (base + ACC_SCALE * value, the add
    in fp32): the largest error relative to ``source_scale``.  The kernel's bound is four times this (``kernel_bound``); the margin covers
    the device's sin / acos / division and another summation order over the channels."""
    if "err" not in _measured:
        worst = 0.0
        for index, ((_h, _w), (H, W)) in enumerate(SIZES):
            for C in CHANNELS:
                src, base, _ = case_input(index, C)
                want, dots = bislerp(src, W, H)
                got, _ = bislerp(src, W, H, dtype=torch.float32)
                keep, scale = ~near_threshold(dots), source_scale(src, W, H)
                worst = max(worst, rel_error(got, want, scale, keep))
                worst = max(worst, rel_error(base + got * ACC_SCALE, base.double() + want * ACC_SCALE, scale, keep))
        _measured["err"] = worst
    return _measured["err"]


def kernel_bound():
    return 4.0 * fp32_statement_error()


# ------------------------------------------------------------------------------------------------ inputs with known values
def _pair(a, b):  # two C-vectors side by side: [1, C, 1, 2]
    return torch.stack([a, b], dim=-1).reshape(1, -1, 1, 2)


def known_inputs():
    """name -> (samples fp32, W, H): zero vectors, identical and negated neighbours, one channel -- robustly on one side of the thresholds"""
    g = torch.Generator().manual_seed(7001)
    v4, v16 = torch.randn(4, generator=g), torch.randn(16, generator=g)
    return {
        "zero_then_vector": (_pair(torch.zeros(4), v4), 5, 1),
        "zero_then_vector_c16": (_pair(torch.zeros(16), v16), 7, 3),
        "identical": (_pair(v4, v4.clone()), 5, 2),
        "negated": (_pair(v16, -v16), 5, 1),
        "one_channel": (torch.randn(2, 1, 5, 7, generator=g), 11, 9),
        "same_size": (torch.randn(2, 4, 6, 6, generator=g), 6, 6),
    }
