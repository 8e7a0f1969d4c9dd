"""Sigma-gated latent operations (API of the reference's ``py/latent_ops.py``); the arithmetic (scale, difference, blend,
noise add) runs through the HIP elementwise kernels.  ``LatentOperationCFG`` is the sampling-time patch that applies them
(``SonarApplyLatentOperationCFG``, py/nodes/latent_operations.py:22-314)."""
from __future__ import annotations

import math
import random
from typing import Sequence

import torch

from .. import hip_lib
from . import utils


class SonarLatentOperation:
    """py/latent_ops.py:15-58."""

    EXTENDED_LATENT_OPERATION = True

    def __init__(self, *, start_sigma: float = math.inf, end_sigma: float = 0.0, op=None):
        self.start_sigma = start_sigma if start_sigma >= 0 else math.inf
        self.end_sigma = end_sigma
        self.op = op

    def enabled(self, sigma=None) -> bool:
        if isinstance(sigma, torch.Tensor):
            sigma = sigma.detach().max().cpu().item()
        return sigma is None or self.end_sigma <= sigma <= self.start_sigma

    def call_op(self, t, *args, op=None, **kwargs):
        op = self.op if op is None else op
        if op is None:
            return t
        if not getattr(op, "EXTENDED_LATENT_OPERATION", False):
            return op(latent=t)
        return op(*args, latent=t, **kwargs)

    def __call__(self, latent, *, sigma=None, **kwargs):
        if not self.enabled(sigma=sigma):
            return latent
        return self.call_op(latent, sigma=sigma, **kwargs)


class SonarLatentOperationAdvanced(SonarLatentOperation):
    """py/latent_ops.py:61-106: blend(t, ops(t * in) [* out] - t) * diff_mul, strength).  ``output_multiplier`` is applied
    only when it equals 1.0 (reference :101-103; reproduced, not fixed)."""

    def __init__(self, *, blend_mode: str, blend_strength: float, input_multiplier: float, output_multiplier: float,
                 difference_multiplier: float, ops: Sequence, op_alt=None, **kwargs):
        super().__init__(**kwargs)
        self.blend_function = utils.BLENDING_MODES[blend_mode]
        self.blend_strength = blend_strength
        self.input_multiplier, self.output_multiplier, self.difference_multiplier = input_multiplier, output_multiplier, difference_multiplier
        self.op_alt = op_alt
        self.ops = ops

    def __call__(self, latent, *, sigma=None, **kwargs):
        t = latent
        if not self.enabled(sigma):
            return t if self.op_alt is None else self.call_op(t, sigma=sigma, op=self.op_alt, **kwargs)
        t32 = utils.as_f32(t)
        output = hip_lib.mul_scalar(t32, self.input_multiplier) if self.input_multiplier != 1.0 else t32
        for op in self.ops:
            output = self.call_op(output, sigma=sigma, op=op, **kwargs)
        scaled = hip_lib.mul_scalar(utils.as_f32(output), self.output_multiplier) if self.output_multiplier == 1.0 else utils.as_f32(output)
        diff = hip_lib.blend("subtract_b", scaled, t32, 1.0)
        if self.difference_multiplier != 1.0:
            hip_lib.scale_noise_(diff, self.difference_multiplier, False, None)
        return self.blend_function(t32, diff, self.blend_strength)


class SonarLatentOperationNoise(SonarLatentOperation):
    """py/latent_ops.py:109-186: noise (optionally * sigma) + latent."""

    def __init__(self, *args, custom_noise, scale_to_sigma: bool = False, cpu_noise: bool = False, normalize: bool = True,
                 lazy_noise_sampler: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.custom_noise = custom_noise
        self.normalize, self.scale_to_sigma, self.cpu_noise = normalize, scale_to_sigma, cpu_noise
        self.lazy_noise_sampler = lazy_noise_sampler
        self.noise_sampler = None
        self.cache_id = None

    def __call__(self, latent, *, sigma=None, **kwargs):
        t = latent
        if not self.enabled(sigma):
            return t
        if isinstance(sigma, float):
            sigma = torch.full((1,), sigma)
        make_ns = not self.lazy_noise_sampler or self.noise_sampler is None
        sigma_min = sigma_max = sigma_next = None
        sample_sigmas = kwargs.get("raw_args", {}).get("model_options", {}).get("transformer_options", {}).get("sample_sigmas")
        if sample_sigmas is not None and sigma is not None:
            sig_host = sigma.detach().max().cpu()
            ss = sample_sigmas.detach().cpu()
            step = int((ss - sig_host).abs().argmin())
            if ss[step].max().item() == sig_host.item() and step + 1 < len(ss):
                sigma_next = ss[step + 1]
        if self.lazy_noise_sampler and not make_ns:
            cache_id = id(sample_sigmas) if isinstance(sample_sigmas, torch.Tensor) else None
            make_ns = cache_id is None or cache_id != self.cache_id
            self.cache_id = cache_id
            if make_ns and sample_sigmas is not None:
                pos = sample_sigmas[sample_sigmas > 0]
                sigma_min = pos.min().item() if pos.numel() else 0.0
                sigma_max = sample_sigmas.max().item()
        t32 = utils.as_f32(t)
        if make_ns:
            ns = self.custom_noise.make_noise_sampler(t32, sigma_min=sigma_min, sigma_max=sigma_max, normalized=self.normalize,
                                                      seed=torch.randint(1, 1 << 31, (), device="cpu").item(), cpu=self.cpu_noise)
        else:
            ns = self.noise_sampler
        if make_ns and self.lazy_noise_sampler:
            self.noise_sampler = ns
        noise = ns(sigma, sigma if sigma_next is None else sigma_next)
        utils.pop_stats(noise)
        scale = float(sigma.detach().max()) if (self.scale_to_sigma and sigma is not None) else 1.0
        return hip_lib.axpby_(noise, scale, t32, 1.0)  # noise * sigma + t in one kernel


class SonarLatentOperationSetSeed(SonarLatentOperation):
    """py/latent_ops.py:189-209."""

    def __init__(self, *args, seed: int, restore_rng_state: bool, **kwargs):
        super().__init__(*args, **kwargs)
        self.seed = seed
        self.restore_rng_state = restore_rng_state

    def __call__(self, *args, **kwargs):
        saved = (random.getstate(), torch.random.get_rng_state()) if self.restore_rng_state else None
        try:
            torch.manual_seed(self.seed)
            random.seed(self.seed)
            return super().__call__(*args, **kwargs)
        finally:
            if saved is not None:
                random.setstate(saved[0])
                torch.random.set_rng_state(saved[1])


# ------------------------------------------------------------------------------------------------ operations applied while sampling
CFG_OP_MODES = ("cond_sub_uncond", "denoised_sub_uncond", "uncond_sub_cond", "denoised", "cond", "uncond", "model_input")
BLEND_SCALE_MODES = ("none", "reverse_sampling", "sampling", "reverse_enabled_range", "enabled_range", "sampling_sin", "enabled_range_sin")


def get_blend_scaling(*, model_sampling, scale_mode: str, sigma: float, sigma_t_max: torch.Tensor, start_sigma: float, end_sigma: float,
                      offset: float, min_pct: float, max_pct: float) -> float:
    """py/nodes/latent_operations.py:120-155: the factor on blend_strength.  Host arithmetic throughout."""
    if scale_mode == "none":
        return 1.0
    if scale_mode in {"sampling", "sampling_sin", "reverse_sampling"}:
        rev_sampling_pct = (model_sampling.timestep(sigma_t_max) / 999).clamp(0, 1).detach().item()
        result = 1.0 - rev_sampling_pct if scale_mode == "sampling" else rev_sampling_pct
    elif scale_mode in {"enabled_range", "enabled_range_sin", "reverse_enabled_range"}:
        rev_range_pct = (sigma - end_sigma) / (start_sigma - end_sigma)
        result = 1.0 - rev_range_pct if scale_mode == "enabled_range" else rev_range_pct
    else:
        raise ValueError("Bad blend_scale_mode")
    if scale_mode.endswith("_sin"):
        result = math.sin(result * math.pi)
    return max(min_pct, min(result + offset, max_pct))


class LatentOperationCFG:
    """py/nodes/latent_operations.py:197-300: the function the node installs as a pre-CFG or post-CFG hook (and calls from its UNet wrapper
    for ``model_input``).  Per call: one value read from the device (the largest sigma, as in the reference), ``hip_lib.cfg_op_prepare``,
    the operations on fp32 tensors, ``hip_lib.cfg_op_finish``.  Inputs are never written; float32 / float16 / bfloat16 predictions go to the
    kernels as they are and the result has the dtype of the tensor it replaces.

    The reference keeps ``mode`` in a closure variable that the fallback of the ``*_sub_uncond`` modes rewrites, and its uncond gate reads
    that variable BEFORE the call's own rewrite -- so the gate sees the mode the previous enabled call ended with.  ``self.mode`` is that
    variable; reproduced as it is."""

    NEEDS_UNCOND = frozenset({"uncond", "uncond_sub_cond", "denoised_sub_uncond"})

    def __init__(self, *, model_sampling, operations: Sequence, mode: str, pred_flip_mode: bool, require_uncond: bool, start_sigma: float,
                 end_sigma: float, blend_mode: str, blend_strength: float, blend_scale_mode: str, blend_scale_offset: float,
                 blend_scale_min: float, blend_scale_max: float, immediate_blend: bool, blend_scaling=get_blend_scaling):
        if blend_mode not in hip_lib.BLEND_IDS:
            raise KeyError(blend_mode)
        self.operations = tuple(operations)
        self.blend_scaling = blend_scaling  # the node hands in its own static method (the reference calls cls.get_blend_scaling)
        self.orig_mode = self.mode = mode
        self.post_cfg_mode = mode in {"denoised", "denoised_sub_uncond"}
        self.pred_flip_mode, self.require_uncond, self.immediate_blend = pred_flip_mode, require_uncond, immediate_blend
        self.blend_mode, self.blend_strength = blend_mode, blend_strength
        self.blend_scale_offset, self.blend_scale_min, self.blend_scale_max = blend_scale_offset, blend_scale_min, blend_scale_max
        sigma_max, sigma_min = model_sampling.sigma_max.detach().item(), model_sampling.sigma_min.detach().item()
        if start_sigma < 0:
            start_sigma = sigma_max
        start_sigma = max(sigma_min, min(sigma_max, start_sigma))
        end_sigma = max(sigma_min, min(sigma_max, end_sigma))
        if end_sigma > start_sigma:
            start_sigma, end_sigma = end_sigma, start_sigma
        if start_sigma == end_sigma:
            blend_scale_mode = "none"
        self.sigma_max, self.sigma_min = sigma_max, sigma_min
        self.start_sigma, self.end_sigma, self.blend_scale_mode = start_sigma, end_sigma, blend_scale_mode

    @staticmethod
    def _operand(t: torch.Tensor, dtype=None) -> torch.Tensor:
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t if t.is_contiguous() else t.contiguous()

    def __call__(self, args: dict):
        x = args["input"]
        cond_scale = args.get("cond_scale")
        sigma_t = args["sigma"]
        sigma = sigma_t.detach().max().item()  # the call's one read from the device
        enabled = self.end_sigma <= sigma <= self.start_sigma
        conds_out = args.get("conds_out", ())
        post_cfg_mode = self.post_cfg_mode
        uncond = args.get("uncond_denoised") if post_cfg_mode else (conds_out[1] if len(conds_out) > 1 else None)
        if uncond is None and (self.require_uncond or self.mode in self.NEEDS_UNCOND):
            enabled = False
        if not enabled:
            if self.mode == "model_input":
                return x
            return args["denoised"] if post_cfg_mode else conds_out
        cond = conds_out[0] if not post_cfg_mode and len(conds_out) else None
        if uncond is None and self.mode.endswith("_sub_uncond"):
            self.mode = self.orig_mode.split("_", 1)[0]
        else:
            self.mode = self.orig_mode
        mode = self.mode
        if mode == "model_input":
            t1, t2 = x, None
        elif mode in {"cond", "cond_sub_uncond"}:
            t1, t2 = cond, (uncond if mode == "cond_sub_uncond" else None)
        elif mode in {"uncond", "uncond_sub_cond"}:
            t1, t2 = uncond, (cond if mode == "uncond_sub_cond" else None)
        else:
            t1, t2 = args["denoised"], (uncond if mode == "denoised_sub_uncond" else None)
        clamped = max(self.sigma_min, min(sigma, self.sigma_max))
        curr_blend = self.blend_strength * self.blend_scaling(
            scale_mode=self.blend_scale_mode, offset=self.blend_scale_offset, min_pct=self.blend_scale_min, max_pct=self.blend_scale_max,
            model_sampling=args["model"].model_sampling, start_sigma=self.start_sigma, end_sigma=self.end_sigma, sigma=clamped,
            # a host tensor of the value already read: timestep() then never waits for the device, wherever the model keeps its tables
            sigma_t_max=torch.tensor(clamped, dtype=sigma_t.dtype if sigma_t.dtype.is_floating_point else torch.float32))
        t1_orig = self._operand(t1)
        dtype = t1_orig.dtype
        t2c = None if t2 is None else self._operand(t2, dtype)
        xc = sig = None
        if self.pred_flip_mode:
            xc = self._operand(x, dtype)
            sig = sigma_t.detach().reshape(-1).to(device=t1_orig.device, dtype=torch.float32).contiguous()
        result, t2f = hip_lib.cfg_op_prepare(xc, t1_orig, t2c, sig)  # result is the patch's own buffer, t2 or not
        for operation in self.operations:
            curr_result = utils.as_f32(operation(result, sigma=sigma, t2=t2f, cond=cond, uncond=uncond, cond_scale=cond_scale, raw_args=args))
            result = hip_lib.blend(self.blend_mode, result, curr_result, curr_blend) if self.immediate_blend else curr_result
        result = hip_lib.cfg_op_finish(result, t2f, xc, sig, t1_orig, None if self.immediate_blend else self.blend_mode, curr_blend)
        if post_cfg_mode or mode == "model_input":
            return result
        conds_out = conds_out.copy()
        conds_out[0 if mode.startswith("cond") else 1] = result
        return conds_out
