"""FreeU Extreme on MI355X (the reference's ``py/nodes/freeu_extreme.py``), through the Python API.

``ffilter`` (:10-29): ``irfft2(rfft2(x) * filter)`` on an arbitrary feature map is ONE call of the LDS-resident forward + filter + inverse
kernel (``sonar_spectral_filter_f32``).  ``FreeUExtremeConfig`` (:113-255) applies the whole effect -- hidden-mean scale map, channel
slice, filter, blend -- in place on the UNet's fp32 / fp16 / bf16 feature map: the hidden-mean launches and ONE fused apply launch
(csrc/freeu.hip) instead of the casts, copies and torch reductions the composition costs.  ``make_block_patches`` restates the handler
(:293-334) and ``patch_model`` does what ``FreeUExtremeNode.go`` does on a duck-typed model.  There is no node: the registry keys
``FreeUExtreme`` / ``FreeUExtremeConfig`` exist and raise.
"""
from __future__ import annotations

import torch

from ... import hip_lib
from ..utils import host_setup_threads
from .powernoise import PowerFilter


def ffilter(x: torch.Tensor, pfilter: PowerFilter, normalization_factor: float = 1.0, cfg_idx=None, filter_cache=None) -> torch.Tensor:
    """py/nodes/freeu_extreme.py:10-29.  The normalised half-spectrum filter is built once per (cfg_idx, plane size) and kept on the
    device in ``filter_cache``; a hit is used whatever ``pfilter`` says, like the reference.  fp16 / bf16 inputs are filtered in fp32
    and cast back."""
    cache_key = None
    if filter_cache is not None and cfg_idx is not None:
        cache_key = (cfg_idx, x.shape[-2:])
        filter_rfft = filter_cache.get(cache_key)
    else:
        # the reference reads `filter_rfft` before binding it when there is no cache key (:12-16): same failure, not a silent rebuild
        raise UnboundLocalError("local variable 'filter_rfft' referenced before assignment")
    if not x.is_cuda:
        raise hip_lib.SonarHipError(f"ffilter: got a {x.device} tensor; this implementation only runs on a ROCm device")
    if filter_rfft is None:
        with host_setup_threads():
            filter_rfft = PowerFilter.normalize(pfilter.build(x.shape), x.shape, normalization_factor=normalization_factor)
        filter_rfft = filter_rfft.to(x.device, torch.float32)
    filter_cache[cache_key] = filter_rfft
    h, w = x.shape[-2:]
    if not hip_lib.power_supported(h, w):
        raise hip_lib.SonarHipError(f"ffilter: plane {h}x{w} is beyond the spectral kernels (sides of at most 2048)")
    x32 = x if x.dtype == torch.float32 else x.to(torch.float32)
    out = hip_lib.spectral_filter(x32.contiguous(), filter_rfft.reshape(h, w // 2 + 1).contiguous())
    return out if x.dtype == torch.float32 else out.to(x.dtype)


# Planes (H, W) of kind 1 / 2 that take the pre-filtered route (the tuned fixed-size ``sonar_spectral_filter_f32`` into an fp32 temporary,
# then one finishing sweep) because it measured faster than the fused kernel there: SDXL's three stages, profiles/freeu_extreme.md (fp16,
# batch 2: 61 / 67 / 88 us against 81 / 75 / 146 us fused at slice 1.0).  Every other LDS-resident plane takes the fused kernel.
PREFILTERED_PLANES: frozenset = frozenset({(32, 32), (64, 64), (128, 128)})


class FreeUExtremeConfig:
    """py/nodes/freeu_extreme.py:113-255.  ``apply`` runs on the device, in place, whatever ``cpu_fft`` says."""

    _keys = ("target", "stage_1", "stage_2", "stage_3", "start", "end", "slice", "slice_offset", "filter_norm", "scale", "blend", "blend_mode",
             "hidden_mean", "final", "sonar_power_filter", "frux_config")

    def __init__(self, *, target, stage_1=False, stage_2=False, stage_3=False, start=0.0, end=1.0, slice=1.0, slice_offset=0.0,  # noqa: A002
                 filter_norm=1.0, scale=1.0, blend=1.0, blend_mode=None, hidden_mean=True, final=True, sonar_power_filter_opt=None,
                 frux_config_opt=None):
        self.target = target
        self.stage_1 = stage_1
        self.stage_2 = stage_2
        self.stage_3 = stage_3
        self.start = start
        self.end = end
        self.slice = slice
        self.slice_offset = slice_offset
        self.filter_norm = filter_norm
        self.scale = scale
        self.blend = blend
        self.blend_mode = blend_mode
        self.hidden_mean = hidden_mean
        self.final = final
        self.sonar_power_filter = sonar_power_filter_opt
        self.frux_config = frux_config_opt

    def get_config_list(self):
        """:170-184, quirks kept: the head is always kept, later entries are dropped by the start / end / blend / stage test, reversed."""
        result = [self]
        curr = self
        while cfg := curr.frux_config:
            curr = cfg
            if cfg.start >= 1 or cfg.end <= 0 or cfg.blend == 0 or not (cfg.stage_1 or cfg.stage_2 or cfg.stage_3):
                continue
            result.append(cfg)
        result.reverse()
        return result

    def get_scale(self, h: torch.Tensor):
        """:187-197: the scalar, or the map 1 + (scale - 1) * (m - min_b) / (max_b - min_b) [B, 1, H, W] of the channel mean m, in ``h``'s
        dtype (computed in fp32 and rounded once).  ``apply`` does not call this: its kernel forms the same map on the fly."""
        if not self.hidden_mean:
            return self.scale
        mean, ext = _hidden(h)
        b, _c, hh, ww = h.shape
        m = (mean - ext[:, :1]) / (ext[:, 1:] - ext[:, :1])
        return (1.0 + (self.scale - 1.0) * m).reshape(b, 1, hh, ww).to(h.dtype)

    def check_match(self, pct, stage, is_skip=False):
        if pct < self.start or pct > self.end:
            return False
        if not getattr(self, f"stage_{stage}"):
            return False
        return not self.target not in {"skip" if is_skip else "backbone", "both"}

    def slice_bounds(self, features: int):
        """(first channel, channel count) of ``x[:, offs : offs + size]`` with size = int(C * slice), offs = int(C * slice_offset), clamped
        the way Python slicing clamps."""
        size = int(features * self.slice)
        offs = int(features * self.slice_offset)
        c0, c1, _ = slice(offs, offs + size).indices(features)  # noqa: A002
        return c0, max(c1 - c0, 0)

    def apply(self, idx, x, filter_cache, cpu_fft=False):
        """:206-230, in place on ``x`` (the returned object).  ``cpu_fft`` is accepted and ignored: everything runs on the device.  Half
        tensors are computed in fp32 and rounded once.  A layout whose planes are not contiguous goes through a dense copy and back."""
        lay = hip_lib.freeu_layout(x, "FreeUExtremeConfig.apply")
        c0, cn = self.slice_bounds(x.shape[1])
        if self.blend != 1.0 and self.blend_mode not in hip_lib.BLEND_IDS:
            raise KeyError(self.blend_mode)
        if cn == 0 or x.numel() == 0:
            return x
        work = x if lay is not None else x.contiguous()
        b, _c, h, w = work.shape
        hidden = _hidden(work) if self.hidden_mean else None
        kw = dict(hidden=hidden, scale=self.scale, blend_mode=None if self.blend == 1.0 else self.blend_mode, blend=self.blend)
        if self.sonar_power_filter is None:
            hip_lib.freeu_apply_(work, c0, cn, mode=hip_lib.FREEU_PLAIN, **kw)
        else:
            filt = _cached_filter(self.sonar_power_filter, (b, cn, h, w), work.device, self.filter_norm, idx, filter_cache, "FreeUExtremeConfig.apply")
            if hip_lib.power_plane_kind(h, w) in (1, 2) and (h, w) not in PREFILTERED_PLANES:
                hip_lib.freeu_apply_(work, c0, cn, mode=hip_lib.FREEU_FUSED, filt=filt, **kw)
            else:  # odd sides / a half-spectrum beyond LDS (the direct passes) or a plane routed here: a temporary, one finishing sweep
                tmp = hip_lib.spectral_filter(work[:, c0:c0 + cn].to(torch.float32).contiguous(), filt)
                hip_lib.freeu_apply_(work, c0, cn, mode=hip_lib.FREEU_FILTERED, filtered=tmp, **kw)
        if work is not x:
            x.copy_(work)
        return x

    def apply_filter(self, idx, xslice, filter_cache, cpu_fft=False):
        """:232-248 as a function of its own (a new tensor); ``cpu_fft`` is ignored."""
        filt = self.sonar_power_filter
        if filt is None:
            return xslice
        return ffilter(xslice, filt, normalization_factor=self.filter_norm, cfg_idx=idx, filter_cache=filter_cache)

    def clone(self):
        """:250-251.  The reference hands ``_keys`` straight to a constructor whose last two keywords end in ``_opt`` and raises TypeError;
        here the two names are mapped, so a clone is a copy."""
        kw = {k: getattr(self, k) for k in self._keys}
        kw["sonar_power_filter_opt"] = kw.pop("sonar_power_filter")
        kw["frux_config_opt"] = kw.pop("frux_config")
        return self.__class__(**kw)

    def __repr__(self):
        meh = {k: getattr(self, k) for k in self._keys}
        return f"<FRUXConfig: {meh}>"


def _hidden(x: torch.Tensor):
    lay = hip_lib.freeu_layout(x, "FreeUExtremeConfig.get_scale")
    return hip_lib.freeu_hidden_mean(x if lay is not None else x.contiguous())


def _cached_filter(pfilter, shape, device, normalization_factor, cfg_idx, filter_cache, what):
    """ffilter's filter look-up (:11-22): keyed (cfg_idx, plane size), a hit wins over ``pfilter``, no key fails as the reference does."""
    if filter_cache is None or cfg_idx is None:
        raise UnboundLocalError("local variable 'filter_rfft' referenced before assignment")
    h, w = shape[-2:]
    key = (cfg_idx, torch.Size((h, w)))
    filt = filter_cache.get(key)
    if filt is None:
        with host_setup_threads():
            filt = PowerFilter.normalize(pfilter.build(torch.Size(shape)), torch.Size(shape), normalization_factor=normalization_factor)
        filt = filt.to(device, torch.float32)
    filter_cache[key] = filt
    if not hip_lib.power_supported(h, w):
        raise hip_lib.SonarHipError(f"{what}: plane {h}x{w} is beyond the spectral kernels (sides of at most 2048)")
    return filt.reshape(h, w // 2 + 1).contiguous()


def make_block_patches(*, model_channels, timestep, input_config=None, middle_config=None, output_config=None):
    """The handler of FreeUExtremeNode.go (:293-334) as three closures ``(in_patch, mid_patch, out_patch)``; an entry is None where its
    config is None.  ``timestep``: the model sampling object's ``timestep(sigma)``.  One filter cache serves the three patches; the
    largest sigma comes to the host through ``max_to_host`` (one launch, one stream wait)."""
    stages = {model_channels * 4: 1, model_channels * 2: 2, model_channels: 3}
    icfg, mcfg, ocfg = (() if cfg is None else cfg.get_config_list() for cfg in (input_config, middle_config, output_config))
    filter_cache = {}

    def max_sigma(sigmas):
        if not sigmas.is_cuda:
            return sigmas.max().detach()
        s = sigmas.detach()
        return torch.tensor(hip_lib.max_to_host(s if s.dtype == torch.float32 else s.to(torch.float32)))

    def handler(_typ, h_shape, cfg, x, toptions, is_skip=False):
        stage = stages.get(h_shape[1])
        if stage is None:
            return x
        pct = 1.0 - (timestep(max_sigma(toptions["sigmas"])) / 999.0)
        for idx, ci in enumerate(cfg):
            if not ci.check_match(pct, stage, is_skip):
                continue
            x = ci.apply(idx, x, filter_cache)
            if ci.final:
                break
        return x

    def in_patch(h, toptions):
        return handler("input", h.shape, icfg, h, toptions)

    def mid_patch(h, toptions):
        return handler("middle", h.shape, mcfg, h, toptions)

    def out_patch(h, hsp, toptions):
        h = handler("output", h.shape, ocfg, h, toptions)
        hsp = handler("output", h.shape, ocfg, hsp, toptions, is_skip=True)
        return h, hsp

    return (in_patch if input_config is not None else None, mid_patch if middle_config is not None else None,
            out_patch if output_config is not None else None)


def patch_model(model, cpu_fft=False, input_config=None, middle_config=None, output_config=None):
    """FreeUExtremeNode.go (:285-334) on a duck-typed ComfyUI model patcher: ``clone()``, ``get_model_object("model_sampling")`` and one
    ``set_model_*patch`` call per given config.  ``cpu_fft`` is accepted and ignored.  Returns the patched clone."""
    model_channels = model.model.model_config.unet_config["model_channels"]
    m = model.clone()
    ms = m.get_model_object("model_sampling")
    in_patch, mid_patch, out_patch = make_block_patches(model_channels=model_channels, timestep=ms.timestep, input_config=input_config,
                                                        middle_config=middle_config, output_config=output_config)
    if in_patch is not None:
        m.set_model_input_block_patch(in_patch)
    if mid_patch is not None:
        m.set_model_patch(mid_patch, "middle_block_patch")
    if out_patch is not None:
        m.set_model_output_block_patch(out_patch)
    return m
