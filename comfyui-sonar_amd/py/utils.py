"""Tensor utilities of the Sonar hot path on MI355X (mirrors the reference's ``py/utils.py`` API).

Every arithmetic function launches hand-written HIP kernels (``hip_lib``) on ROCm tensors.  The
normaliser keeps the reference's whole-tensor, data-dependent semantics (py/utils.py:85-106) but
evaluates the thresholds on device, so there is no ``.item()`` host sync.
"""
from __future__ import annotations

import contextlib
import os
import threading
from typing import Callable, Optional, Sequence

import torch

from .. import hip_lib

Tensor = torch.Tensor

UPSCALE_METHODS = ("bilinear", "nearest-exact", "nearest", "area", "bicubic", "bislerp", "adaptive_avg_pool2d")

# scale_samples(mode="bislerp") -- and with it ResizedNoise's upscale_mode / downscale_mode -- runs utils.bislerp only with this switch on;
# off, it keeps refusing as before (the pyramid generators and utils.bislerp take the mode either way)
BISLERP_IN_SCALE_SAMPLES = os.environ.get("SONAR_BISLERP_SCALE", "0") != "0"

_STATS_ATTR = hip_lib.STATS_ATTR


_HOST_SETUP_THREADS = 4
_host_setup_lock = threading.Lock()
_host_setup_users = 0
_host_setup_before = None


@contextlib.contextmanager
def host_setup_threads():
    """The host-side, once-per-sampler tensor work of the path (the power filter's oversampled grid, py/nodes/powernoise.py:156-266) on a
    few CPU threads instead of torch's default of one per logical CPU.  Round 5 traced an intermittent 50-90 ms freeze of launch-bound
    steps (round 4's bench read 434 us for a 27 us call) to this: a 256-thread intra-op pool spins for a while after every parallel
    region, a container with a CPU quota (the GPU pool's: 16 CPUs per 100 ms) runs out of quota, and the kernel's bandwidth control
    throttles the WHOLE process -- the thread that launches kernels included -- until the period ends (cpu.stat nr_throttled 0 -> 100
    over three 4-second runs; none with 4 threads; scratch/stall_fresh.py).  The tensors are a few hundred kilobytes:
    four threads lose nothing, and elementwise results do not depend on the thread count.
    The count is process-global, so concurrent users share ONE lowering: the first to enter lowers it and remembers the old value, the
    last to leave puts it back (a lock and a count of users; interleaved enter / exit pairs used to be able to leave the pool at four
    threads, or restore a stale value)."""
    global _host_setup_users, _host_setup_before
    with _host_setup_lock:
        if _host_setup_users == 0:
            before = torch.get_num_threads()
            _host_setup_before = before if before > _HOST_SETUP_THREADS else None
            if _host_setup_before is not None:
                torch.set_num_threads(_HOST_SETUP_THREADS)
        _host_setup_users += 1
    try:
        yield
    finally:
        with _host_setup_lock:
            _host_setup_users -= 1
            if _host_setup_users == 0 and _host_setup_before is not None:
                torch.set_num_threads(_host_setup_before)
                _host_setup_before = None


def fallback(val, default=None):
    return val if val is not None else default


# --------------------------------------------------------------------------------------------------
# fused statistics hand-off: a producer kernel that already reduced (sum, sumsq) of the tensor it
# wrote tags the tensor; the next scale_noise() on that very tensor consumes the tag instead of
# re-reading the tensor.  Any in-package op that changes the values must drop the tag first.
def attach_stats(t: Tensor, partials: Optional[Tensor]) -> Tensor:
    if partials is not None:
        setattr(t, _STATS_ATTR, (partials, t._version))
        hip_lib.tag_register(t)
    return t


def pop_stats(t: Tensor) -> Optional[Tensor]:
    """The tag is honoured only if nothing wrote to the tensor since: torch's in-place ops bump ``_version`` (shared by all views of
    a storage); every kernel of this library that is handed ANY view of the tensor's storage drops the tag (hip_lib._dev)."""
    p = getattr(t, _STATS_ATTR, None)
    if p is None:
        return None
    delattr(t, _STATS_ATTR)
    hip_lib.tag_forget(t)
    partials, version = p
    return partials if version == t._version else None


def _require_device(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise hip_lib.SonarHipError(f"{what}: got a {t.device} tensor; this implementation only runs on a ROCm device")


def as_f32(t: Tensor) -> Tensor:
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


# --------------------------------------------------------------------------------------------------
def _tiles(t: Tensor, a: Tensor) -> bool:
    """True when ``t`` broadcast against ``a`` is a plain tiling of t's flat data (trailing dims match)."""
    ts = list(t.shape)
    while ts and ts[0] == 1:
        ts.pop(0)
    return ts == list(a.shape[a.ndim - len(ts):])


def _blend(mode: str) -> Callable:
    def fn(a: Tensor, b: Tensor, t, out: Optional[Tensor] = None) -> Tensor:
        _require_device(a, f"blend[{mode}]")
        a32, b32 = as_f32(a), as_f32(b.to(a.device))
        if b32.shape != a32.shape:
            b32 = b32.expand_as(a32).contiguous()
        if isinstance(t, Tensor):
            if t.numel() == 1:
                t = float(t)  # host scalar weight (syncs only if the weight lives on the device)
            else:
                t = as_f32(t.to(a.device))
                if not _tiles(t, a32):
                    t = t.expand_as(a32).contiguous()
        res = hip_lib.blend(mode, a32, b32, t, out)
        return res if a.dtype == torch.float32 else res.to(a.dtype)

    fn.__name__ = f"blend_{mode}"
    return fn


# py/utils.py:17-21
BLENDING_MODES = {"lerp": _blend("lerp"), "inject": _blend("inject"), "subtract_b": _blend("subtract_b")}


# --------------------------------------------------------------------------------------------------
def scale_noise(noise: Tensor, factor: float = 1.0, *, normalized: bool = True, threshold_std_devs: float = 2.5,
                normalize_dims: Optional[Sequence[int]] = None) -> Tensor:
    """py/utils.py:85-106, in place.  Two kernels (stats -> apply) unless a producer kernel already
    attached the statistics, in which case only the apply kernel runs."""
    n = noise.numel()
    if not normalized or n == 0:
        if factor == 1:
            return noise  # untouched: a statistics tag (written by the producing kernel, checked against storage + version) still describes it
        pop_stats(noise)  # the values change below: the tag would describe other contents
        _require_device(noise, "scale_noise")
        return hip_lib.scale_noise_(noise, factor, False, None)
    _require_device(noise, "scale_noise")
    if noise.dtype != torch.float32 or not noise.is_contiguous():
        raise hip_lib.SonarHipError("scale_noise: expects a contiguous float32 tensor")
    if normalize_dims is not None:
        pop_stats(noise)
        dims = sorted({d % noise.ndim for d in normalize_dims})
        trailing = dims == list(range(noise.ndim - len(dims), noise.ndim))
        if not trailing and not hip_lib.group_scale_noise_slow(noise.shape, dims):
            # not the trailing dimensions: the row kernel's three passes on the tensor as it lies (csrc/group_stats.hip), no transposed copy
            return hip_lib.group_scale_noise_(noise, dims, factor)
        # trailing dimensions, or the one layout measured faster through a transposed copy (few groups, the contiguous dimension kept)
        rows_last, inverse = dims_last(noise, dims)
        inner = 1
        for d in dims:
            inner *= noise.shape[d]
        return dims_restore(hip_lib.scale_noise_rows_(rows_last, n // inner, inner, factor), inverse)
    partials = pop_stats(noise)
    if partials is None:
        partials = hip_lib.stats(noise)
    noise, after = hip_lib.scale_noise_stats_(noise, factor, partials, threshold_std_devs=threshold_std_devs)
    return attach_stats(noise, after)  # a wrapper that normalises this result again skips its statistics sweep


def dims_last(t: Tensor, dims):
    """(tensor with the dimensions ``dims`` moved to the end and made contiguous, permutation that undoes the move or None).  The row
    kernels reduce over trailing dimensions; any other choice (the reference takes any ``dim`` tuple: py/utils.py:97-99,452-470,
    py/sonar.py:372-377) is the same reduction on a transposed copy -- a layout change, no arithmetic."""
    nd = t.ndim
    dims = sorted({d % nd for d in dims})
    if dims == list(range(nd - len(dims), nd)):
        return t.contiguous(), None
    perm = [d for d in range(nd) if d not in dims] + dims
    return t.permute(perm).contiguous(), [perm.index(d) for d in range(nd)]


def dims_restore(t: Tensor, inverse) -> Tensor:
    return t if inverse is None else t.permute(inverse).contiguous()


def bislerp(samples: Tensor, width: int, height: int) -> Tensor:
    """ComfyUI's ``comfy.utils.bislerp(samples, width, height)`` on the device (csrc/bislerp.hip): the C-vector of every pixel of
    ``samples`` [N, C, h, w] resampled by spherical interpolation, along the width and then along the height.  Any float dtype, contiguous or
    strided; computed in fp32, returned in the input's dtype.  ComfyUI is not vendored by the reference: **parity unpinned**, the
    definition is restated in DESIGN.md and pinned by tests/bislerp_refs.py."""
    _require_device(samples, "bislerp")
    if samples.ndim != 4:
        raise hip_lib.SonarHipError(f"bislerp: expects [N, C, h, w], got {tuple(samples.shape)}")
    src = as_f32(samples)
    out = torch.empty((*src.shape[:2], height, width), dtype=torch.float32, device=src.device)
    hip_lib.bislerp_acc_(out, src, 1.0, accumulate=False)
    return out if samples.dtype == torch.float32 else out.to(samples.dtype)


def scale_samples(samples: Tensor, width: int, height: int, *, mode: str = "bicubic") -> Tensor:
    """py/utils.py:58-67: ``F.interpolate(samples, size=(height, width), mode=mode)`` on the HIP resampler (bilinear / nearest /
    nearest-exact / bicubic / area / adaptive_avg_pool2d).  ``bislerp`` only with ``BISLERP_IN_SCALE_SAMPLES`` (off by default:
    SONAR_BISLERP_SCALE=1 in the environment); the pyramid generators and ``bislerp`` itself do not depend on the switch."""
    _require_device(samples, "scale_samples")
    if mode in hip_lib.UPSCALE_MODES:
        src = as_f32(samples)
        out = torch.empty((*src.shape[:-2], height, width), dtype=torch.float32, device=src.device)
        hip_lib.resample_acc_(out, src, 1.0, mode, accumulate=False)
        return out if samples.dtype == torch.float32 else out.to(samples.dtype)
    if mode == hip_lib.BISLERP and BISLERP_IN_SCALE_SAMPLES:
        return bislerp(samples, width, height)
    raise NotImplementedError(f"upscale mode {mode!r} needs ComfyUI's bislerp, which the reference does not vendor")


def normalize_to_scale(latent: Tensor, target_min: float, target_max: float, *, dim=(-3, -2, -1), eps: float = 1e-07) -> Tensor:
    """py/utils.py:452-470: per-group min / max (HIP reduction), then rescale + clamp in one kernel."""
    _require_device(latent, "normalize_to_scale")
    x = as_f32(latent)
    dims = sorted({d % x.ndim for d in dim}) if len(dim) else list(range(x.ndim))
    if dims != list(range(x.ndim - len(dims), x.ndim)):
        # not the trailing dimensions: min / max and the rescale on the tensor as it lies (csrc/group_stats.hip) -- the same values as the
        # row kernels give on a transposed copy (min and max do not depend on the order, the rescale is one device function), bit for bit
        lo, hi = hip_lib.group_stats(x, dims, mean_std=False, minmax=True)
        return hip_lib.group_minmax_rescale(x, dims, lo, hi, eps, target_min, target_max)
    x, inverse = dims_last(x, dims)
    inner = 1
    for d in range(x.ndim - len(dims), x.ndim):
        inner *= x.shape[d]
    rows = x.numel() // inner
    lo, hi = hip_lib.minmax_rows(x, rows, inner)
    return dims_restore(hip_lib.minmax_rescale(x, rows, inner, lo, hi, eps, target_min, target_max), inverse)


def normalize_to_scale_adv(t: Tensor, *, min_pos: float, max_pos: float, min_neg: float, max_neg: float, dim=(-3, -2, -1)) -> Tensor:
    """py/utils.py:473-510: negatives and positives rescaled separately between their own extremes.  The reference selects the values of a sign
    into a 1-D tensor first, so whatever ``dim`` says the extremes are those of the WHOLE tensor passed in: one row."""
    _require_device(t, "normalize_to_scale_adv")
    x = as_f32(t).contiguous()
    return hip_lib.signed_rescale(x, 1, x.numel(), min_neg, max_neg, min_pos, max_pos)


def elementwise_shuffle_by_dim(t: Tensor, *, dim: int = -1, prob: float = 1.0, no_identity: bool = False, generator=None,
                               device_key: Optional[tuple] = None) -> Tensor:
    """py/utils.py:599-657: every row of ``t`` along ``dim`` (one position of the other dimensions) shuffled on its own with probability
    ``prob`` -- rotated by a non-zero offset with ``no_identity``, permuted by the order of ``n`` uniform sort keys otherwise.  A gather on
    the tensor as it lies (csrc/shuffle.hip), a new tensor.

    ``device_key`` None is replay mode: the mask, then the offsets or the keys are drawn on the host with the reference's calls, shapes and
    order (``generator``, or torch's global host generator), sorted there and uploaded as int32, so after ``torch.manual_seed(s)`` the
    result is the reference's on the CPU copy of ``t``.  ``device_key`` = (seed, stream) is generate mode: the kernel draws them from streams
    ``stream`` .. ``stream + 2`` by global row, nothing but the tensor is read or written.  A negative ``dim`` counts
    from the end (the reference only takes ``dim >= 0``)."""
    from . import noise_generation

    _require_device(t, "elementwise_shuffle_by_dim")
    nd = t.ndim
    if not -nd <= dim < nd:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-max(nd, 1)}, {max(nd, 1) - 1}], but got {dim})")
    if t.numel() == 0:
        return t.clone()
    d = dim % nd
    x = as_f32(t)
    n = x.shape[d]
    rows = x.numel() // n
    if device_key is not None:
        seed, stream = device_key
        shard = noise_generation.current_batch_offset()
        if shard != 0 and d == 0:
            raise NotImplementedError("elementwise_shuffle_by_dim: dim 0 shuffles across the samples of the batch, which a sharded batch splits")
        out = hip_lib.shuffle_generate(x, d, prob, no_identity, seed, stream, shard * (rows // x.shape[0]))
    else:
        mask = torch.rand(rows, device="cpu", generator=generator) < prob if prob < 1.0 else torch.ones(rows, device="cpu", dtype=torch.bool)
        if no_identity:
            offsets = torch.randint(1, n, (rows,), device="cpu", generator=generator)
            idx = torch.where(mask, offsets, -1)
        else:
            idx = torch.arange(n, device="cpu").expand(rows, -1).clone()
            idx[mask] = torch.rand(rows, n, device="cpu", generator=generator)[mask].argsort(dim=1)
        out = hip_lib.shuffle_gather(x, d, idx.to(torch.int32).to(x.device), offsets=no_identity)
    return out if t.dtype == torch.float32 else out.to(t.dtype)


def pattern_break(noise: Tensor, *, percentage: float = 0.5, detail_level: float = 0.0, restore_scale: bool = True,
                  blend_function: Optional[Callable] = None, route: Optional[str] = None) -> Tensor:
    """py/utils.py:575-596 (after Extraltodeus' noise_latent_perlinpinpin): the tensor rescaled to [-1, 1] between its own extremes, every
    value sent through ``erfinv(2 (|v| 1e6 mod 11) / 11 - 1)``, optionally rescaled to the input's extremes, and blended with the input.
    One to three fused launches (csrc/pattern_break.hip) with no read-back on the host; a new tensor, which carries the (sum, sumsq)
    statistics of its values for the ``scale_noise`` that follows.

    ``blend_function`` is one of ``BLENDING_MODES``' values (``lerp`` by default, where the reference has ``torch.lerp``): the blend runs
    inside the kernel, so any other callable raises ``NotImplementedError``.  float16 / bfloat16 and non-contiguous inputs are computed in
    float32 and cast back (the reference's ``lerp`` raises on the mixed dtypes).  A float32 result keeps its statistics tag also when it is
    copied into a non-contiguous input's layout; a result rounded to another dtype carries none.  ``route`` (None, "one", "three") forces the one-launch or
    the three-launch route; the bits are the same."""
    from . import noise_generation

    mode = "lerp" if blend_function is None else next((k for k, f in BLENDING_MODES.items() if f is blend_function), None)
    if mode is None:
        raise NotImplementedError("pattern_break: a Python blend_function would run on the host; only BLENDING_MODES' functions run here")
    _require_device(noise, "pattern_break")
    if noise.numel() == 0:
        raise RuntimeError("min(): Expected reduction dim to be specified for input.numel() == 0. Specify the reduction dim with the 'dim' argument.")
    if noise_generation.current_batch_offset() != 0:
        raise NotImplementedError("pattern_break: this filter reduces across the samples of the batch, which a sharded batch "
                                  "splits (reduce on one rank, or use a per-sample dim)")
    x = as_f32(noise)
    out, partials = hip_lib.pattern_break(x, 1 + detail_level / 10, percentage, mode, restore_scale, route=route)
    if noise.dtype != torch.float32:
        return out.to(noise.dtype)
    if not noise.is_contiguous():  # as_f32 made a contiguous copy: hand the result back in the input's layout (the sums know no order)
        out = torch.empty_like(noise).copy_(out)
    return attach_stats(out, partials)


def tensor_to(tensor: Tensor, dest) -> Tensor:
    """py/utils.py:112-121."""
    device = dest.device if isinstance(dest, Tensor) else dest
    return tensor.to(device, non_blocking=True)


def crop_samples(tensor: Tensor, width: int, height: int, *, mode: str = "center", offset_width: int = 0, offset_height: int = 0) -> Tensor:
    """py/utils.py:513-570 (pure indexing): a (height, width) window of the last two dimensions, anchored per axis at an edge or the
    centre (`center`, or `<top|center|bottom>_<left|center|right>`) and then moved by the offsets as far as the tensor allows."""
    if tensor.ndim < 3:
        raise ValueError("Can only handle >= 3 dimensional tensors")
    th, tw = tensor.shape[-2:]
    if (tw, th) == (width, height):
        return tensor
    if tw < width or th < height:
        raise ValueError("Can't crop sample smaller than requested width or height")
    parts = ("center", "center") if mode == "center" else tuple(mode.split("_"))
    if len(parts) != 2:
        raise ValueError("Bad composite mode")
    starts = []
    for which, size, want, names in ((parts[0], th, height, ("top", "center", "bottom")), (parts[1], tw, width, ("left", "center", "right"))):
        if which not in names:
            raise ValueError("Bad height mode in composite mode" if names[0] == "top" else "Bad width mode in composite mode")
        starts.append({names[0]: 0, names[1]: (size - want) // 2, names[2]: size - want}[which])

    def shifted(start, want, size, off):
        if off < 0:
            return start - min(start, -off)
        return start + min(size - (start + want), off)

    y0 = shifted(starts[0], height, th, offset_height)
    x0 = shifted(starts[1], width, tw, offset_width)
    return tensor[..., y0:y0 + height, x0:x0 + width]


def tensor_item(val, *, collapse_function=torch.max) -> float:
    if isinstance(val, Tensor):
        return float(collapse_function(val).detach().cpu().item())
    return float(val)


# --------------------------------------------------------------------------------------------------
# quantile filtering (py/utils.py:123-449)
class QuantileStrategy:
    """How one entry of ``quantile_handlers`` runs on the device: a row-kernel strategy code (include/sonar_hip.h SONAR_Q_*), or the
    replace* parameters (count, flip, sign_mode).  ``per_row`` strategies reduce along ``dim`` a second time (the reference calls
    ``max`` / ``median`` / ``mode`` with ``dim``, which refuses ``dim=None``)."""

    __slots__ = ("name", "op", "replace", "per_row")

    def __init__(self, name: str, op: int = 0, replace: Optional[tuple] = None, per_row: bool = False):
        self.name, self.op, self.replace, self.per_row = name, op, replace, per_row

    def __repr__(self):
        return f"QuantileStrategy({self.name!r})"


def _quantile_strategies() -> dict:
    out = {}

    def add(name, *args, **kw):
        out[name] = QuantileStrategy(name, *args, **kw)

    def waves(fn_name, cos_flag):
        for wrong in (False, True):
            stem = f"{fn_name}_wrong" if wrong else fn_name
            for suffix, flag in (("", 0), ("_wholepi", hip_lib.Q_WAVE_WHOLEPI), ("_keepsign", hip_lib.Q_WAVE_KEEPSIGN)):
                add(stem + suffix, hip_lib.Q_WAVE | cos_flag | flag | (hip_lib.Q_WAVE_WRONG if wrong else 0))

    add("clamp", hip_lib.Q_CLAMP)
    add("scale_down", hip_lib.Q_SCALE_DOWN, per_row=True)
    add("tanh", hip_lib.Q_TANH)
    add("tanh_outliers", hip_lib.Q_TANH_OUTLIERS)
    add("sigmoid_keepsign", hip_lib.Q_SIGMOID_KEEPSIGN)
    add("sigmoid", hip_lib.Q_SIGMOID)
    add("sigmoid_outliers", hip_lib.Q_SIGMOID_OUTLIERS)
    waves("sin", 0)
    waves("cos", hip_lib.Q_WAVE_COS)
    add("atan", hip_lib.Q_ATAN)
    add("tenth", hip_lib.Q_TENTH)
    add("half", hip_lib.Q_HALF)
    add("zero", hip_lib.Q_ZERO)
    add("reverse_zero", hip_lib.Q_REVERSE_ZERO)
    add("mean", hip_lib.Q_MEAN)
    add("median", hip_lib.Q_MEDIAN, per_row=True)
    add("mode_1dec", hip_lib.Q_MODE_1DEC, per_row=True)
    add("mode_2dec", hip_lib.Q_MODE_2DEC, per_row=True)
    for count in (1, 2, 3):
        stem = "replace" if count == 1 else f"replace_{count}pt"
        for flip in ((False,) if count == 1 else (False, True)):
            for sign_mode, suffix in ((0, ""), (1, "_keepsign"), (2, "_avoidsign")):
                add(stem + ("_flip" if flip else "") + suffix, replace=(count, flip, sign_mode))
    order = ("clamp", "scale_down", "tanh", "tanh_outliers", "sigmoid_keepsign", "sigmoid", "sigmoid_outliers", "sin", "sin_wholepi",
             "sin_keepsign", "sin_wrong", "sin_wrong_wholepi", "sin_wrong_keepsign", "cos", "cos_wholepi", "cos_keepsign", "cos_wrong",
             "cos_wrong_wholepi", "cos_wrong_keepsign", "atan", "tenth", "half", "zero", "reverse_zero", "mean", "median", "mode_1dec",
             "mode_2dec", "replace", "replace_keepsign", "replace_avoidsign", "replace_2pt", "replace_3pt", "replace_2pt_flip",
             "replace_3pt_flip", "replace_2pt_keepsign", "replace_3pt_keepsign", "replace_2pt_flip_keepsign", "replace_3pt_flip_keepsign",
             "replace_2pt_avoidsign", "replace_3pt_avoidsign", "replace_2pt_flip_avoidsign", "replace_3pt_flip_avoidsign")
    assert sorted(order) == sorted(out)
    return {k: out[k] for k in order}


# the reference's 43 strategies, in its order (the node dropdown is tuple(quantile_handlers.keys()))
quantile_handlers = _quantile_strategies()


def _quantile_check_dim(nd: int, dim: Optional[int], flatten: bool) -> None:
    """What the reference's torch calls raise for this dim (flatten(start_dim=None), a dim out of range)."""
    if nd > 1 and flatten and dim is None:
        raise TypeError("flatten(): argument 'start_dim' must be int, not NoneType")
    nd1 = max(nd, 1)
    if dim is not None and not -nd1 <= dim < nd1:
        raise IndexError(f"Dimension out of range (expected to be in range of [{-nd1}, {nd1 - 1}], but got {dim})")


def _quantile_layout(noise: Tensor, dim: Optional[int], flatten: bool):
    """(rows tensor with contiguous rows, rows, inner, inverse permutation or None, row length along the original layout, stride of a row's
    values in the original layout).  Raises what the reference's torch calls raise for the same arguments."""
    nd = noise.ndim
    _quantile_check_dim(nd, dim, flatten)
    if nd > 1 and flatten:
        d = dim % nd
        inner = 1
        for s in noise.shape[d:]:
            inner *= s
        return noise.contiguous(), noise.numel() // inner, inner, None, inner, 1
    if dim is None:
        return noise.contiguous(), 1, noise.numel(), None, noise.numel(), 1
    if nd == 0:
        return noise.reshape(1).contiguous(), 1, 1, None, 1, 1
    d = dim % nd
    length = noise.shape[d]
    stride = 1
    for s in noise.shape[d + 1:]:
        stride *= s
    rows_last, inverse = dims_last(noise, [d])
    return rows_last, noise.numel() // length, length, inverse, length, stride


def _quantile_once(noise: Tensor, q: float, dim, flatten: bool, nq_fac: float, pow_fac: float, strategy: QuantileStrategy, eps: float) -> Tensor:
    from . import noise_generation

    _quantile_check_dim(noise.ndim, dim, flatten)
    if strategy.per_row and dim is None:
        raise RuntimeError("Please look up dimensions by name, got: name = None.")
    _require_device(noise, "quantile_normalize")
    x = noise if noise.dtype == torch.float32 else noise.to(torch.float32)
    rows_t, rows, inner, inverse, length, stride = _quantile_layout(x, dim, flatten)
    across = dim is None or strategy.replace is not None or dim % max(x.ndim, 1) == 0  # reductions that mix the batch's samples
    if across and noise_generation.current_batch_offset() != 0:
        raise NotImplementedError("quantile_normalize: this dim / strategy reduces across the samples of the batch, which a sharded batch "
                                  "splits (reduce on one rank, or use a per-sample dim)")
    centered = q < 0
    aq = abs(q)
    if strategy.replace is None:
        out = torch.empty_like(rows_t)
        hip_lib.quantile_rows(rows_t, rows, inner, aq, nq_fac, eps, strategy.op, centered, pow_fac, out)
        out = dims_restore(out, inverse)
    else:
        stats = hip_lib.quantile_rows(rows_t, rows, inner, aq, nq_fac, eps, hip_lib.Q_CLAMP, centered, pow_fac, None)
        src = x.contiguous()
        out = torch.empty_like(src)
        count, flip, sign_mode = strategy.replace
        if hip_lib.quantile_replace(src, stats, length, stride, centered, count, flip, sign_mode, pow_fac, out) == 0:
            raise RuntimeError("ZeroDivisionError")  # the reference's `arange(n) % n_candidates` with no candidate
    out = out.reshape(noise.shape)
    return out if noise.dtype == torch.float32 else out.to(noise.dtype)


def quantile_normalize(noise: Tensor, *, quantile=0.75, dim: Optional[int] = 1, flatten: bool = True, nq_fac: float = 1.0,
                       pow_fac: float = 0.5, strategy: str = "clamp", strategy_handler=None, eps: float = 1e-08) -> Tensor:
    """py/utils.py:367-449 on the device: per-row |x| quantile (radix select), one of ``quantile_handlers``, the "centered" mapping for a
    negative quantile and the sign-preserving power.  Returns a new tensor (the input is left as it is), or ``noise`` itself where the
    reference returns early.  Unlike torch.quantile, rows of more than 2^24 values are fine."""
    if noise.numel() == 0:
        return noise
    if isinstance(quantile, (tuple, list)):
        for q in quantile:
            noise = quantile_normalize(noise, quantile=q, dim=dim, flatten=flatten, nq_fac=nq_fac, pow_fac=pow_fac, strategy=strategy,
                                       strategy_handler=strategy_handler)
        return noise
    if quantile is None or quantile >= 1 or quantile <= -1:
        return noise
    if strategy_handler is not None:
        raise NotImplementedError("quantile_normalize: a Python strategy_handler would run on the host; only the built-in strategies run here")
    if noise.ndim > 1 and flatten and dim is None:
        raise TypeError("flatten(): argument 'start_dim' must be int, not NoneType")
    handler = quantile_handlers.get(strategy)
    if handler is None:
        raise ValueError("Unknown strategy")
    return _quantile_once(noise, float(quantile), dim, flatten, float(nq_fac), float(pow_fac), handler, float(eps))
