"""Case table and host stand-ins shared by tests/golden/make_latent_op_cfg_golden.py (which runs the cases through the REAL reference's
SonarApplyLatentOperationCFG) and the tests (which run them through this package's node).  Inputs only: the expected values live in
latent_op_cfg.npz.
"""
from __future__ import annotations

import types

import torch

from tests.golden.wavelet_cases import DiscreteSampling

SHAPE = (2, 4, 10, 14)
MODES = ("cond_sub_uncond", "denoised_sub_uncond", "uncond_sub_cond", "denoised", "cond", "uncond", "model_input")
BLEND_SCALE_MODES = ("none", "reverse_sampling", "sampling", "reverse_enabled_range", "enabled_range", "sampling_sin", "enabled_range_sin")
COND_SCALE = 7.0


# ------------------------------------------------------------------------------------------------ the model side
class ModelPatcher:
    """What the node asks of ComfyUI's model patcher: ``clone``, ``get_model_object``, ``model.model_sampling`` and the three setters."""

    def __init__(self, model=None, cloned_from=None):
        self.model = types.SimpleNamespace(model_sampling=DiscreteSampling()) if model is None else model
        self.cloned_from = cloned_from
        self.post_cfg, self.pre_cfg, self.unet_wrapper = [], [], None

    def clone(self):
        return ModelPatcher(self.model, cloned_from=self)

    def get_model_object(self, name):
        assert name == "model_sampling"
        return self.model.model_sampling

    def set_model_sampler_post_cfg_function(self, fn):
        self.post_cfg.append(fn)

    def set_model_sampler_pre_cfg_function(self, fn):
        self.pre_cfg.append(fn)

    def set_model_unet_function_wrapper(self, fn):
        self.unet_wrapper = fn

    def hooks(self):
        return {"post_cfg": len(self.post_cfg), "pre_cfg": len(self.pre_cfg), "unet_wrapper": int(self.unet_wrapper is not None)}


def inputs():
    g = torch.Generator().manual_seed(4321)
    return {k: torch.randn(SHAPE, generator=g) for k in ("x", "cond", "uncond", "denoised")}


def run_patched(model: ModelPatcher, tensors: dict, sigma: torch.Tensor, has_uncond: bool):
    """Calls whichever hook the node installed the way ComfyUI's sampling loop does; returns (what the hook returned, the args it saw)."""
    x, cond, uncond, denoised = tensors["x"], tensors["cond"], tensors["uncond"], tensors["denoised"]
    if model.unet_wrapper is not None:
        args = {"input": x, "timestep": sigma, "c": {}, "cond_or_uncond": [0, 1]}
        return model.unet_wrapper(lambda inp, _timestep, **_c: inp, args), args
    if model.post_cfg:
        args = {"denoised": denoised, "cond_denoised": cond, "uncond_denoised": uncond if has_uncond else None, "input": x, "sigma": sigma,
                "cond_scale": COND_SCALE, "model": model.model, "model_options": {}}
        return model.post_cfg[0](args), args
    args = {"conds_out": [cond, uncond] if has_uncond else [cond], "input": x, "sigma": sigma, "cond_scale": COND_SCALE, "model": model.model,
            "model_options": {}}
    return model.pre_cfg[0](args), args


# ------------------------------------------------------------------------------------------------ the operations
class ExtendedOp:
    """An operation that asks for the extended keyword set and uses ``t2`` (None when the mode has no second tensor)."""

    EXTENDED_LATENT_OPERATION = True

    def __call__(self, latent, sigma=None, t2=None, cond=None, uncond=None, cond_scale=None, raw_args=None, **_kw):
        assert isinstance(sigma, float) and cond_scale == COND_SCALE and raw_args is not None
        return latent * 0.5 + 0.25 * t2 if t2 is not None else latent * 0.5 + 0.05


QUANTILE_KW = dict(quantile=0.85, dim="1", flatten=True, norm_power=0.5, norm_factor=1.0, strategy="clamp")
ADVANCED_KW = dict(start_sigma=-1.0, end_sigma=0.0, input_multiplier=1.2, output_multiplier=1.0, difference_multiplier=0.9, blend_mode="lerp",
                   blend_strength=0.7)


def build_ops(names, node_classes: dict):
    """The operations of a case; the two node-built ones come from ``node_classes`` (the reference's mapping or this package's)."""
    out = []
    for name in names:
        if name == "affine":
            out.append(lambda latent: latent * 0.75 + 0.1)
        elif name == "ext":
            out.append(ExtendedOp())
        elif name == "quantile":
            cls = node_classes["SonarLatentOperationQuantileFilter"]
            out.append(getattr(cls, cls.FUNCTION)(**QUANTILE_KW)[0])
        elif name == "advanced":
            cls = node_classes["SonarLatentOperationAdvanced"]
            out.append(getattr(cls, cls.FUNCTION)(operation=lambda latent: latent * 0.75 + 0.1, **ADVANCED_KW)[0])
        else:
            raise KeyError(name)
    return out


# ------------------------------------------------------------------------------------------------ the cases
DEFAULTS = dict(mode="cond_sub_uncond", pred_flip_mode=False, require_uncond=False, start_sigma=-1.0, end_sigma=0.0, blend_mode="lerp",
                blend_strength=0.5, blend_scale_mode="none", blend_scale_offset=0.0, blend_scale_min=0.0, blend_scale_max=1.0,
                immediate_blend=False)
PER_SAMPLE = [5.0, 3.0]


def _cases():
    cases = {}

    def add(name, ops=("affine",), sigma=PER_SAMPLE, has_uncond=True, **node):
        assert name not in cases and set(node) <= set(DEFAULTS)
        cases[name] = dict(node=DEFAULTS | node, ops=list(ops), sigma=list(sigma), has_uncond=has_uncond)

    for mode in MODES:
        for flip in (False, True):
            if not (flip and mode == "model_input"):
                add(f"mode_{mode}_{'flip' if flip else 'plain'}", mode=mode, pred_flip_mode=flip)
    add("one_sigma_cond_sub_uncond", sigma=[4.0], pred_flip_mode=True)
    add("one_sigma_denoised", sigma=[4.0], mode="denoised", pred_flip_mode=True)
    for blend in ("lerp", "inject", "subtract_b"):
        add(f"blend_{blend}", blend_mode=blend, blend_strength=0.8, pred_flip_mode=True)
    for immediate in (False, True):
        add(f"chain_flip_immediate_{immediate}", ops=("affine", "ext"), pred_flip_mode=True, immediate_blend=immediate, blend_strength=0.3)
        add(f"chain_post_immediate_{immediate}", ops=("ext", "affine"), mode="denoised_sub_uncond", immediate_blend=immediate, blend_mode="inject")
    for scale_mode in BLEND_SCALE_MODES:
        add(f"scale_{scale_mode}", blend_scale_mode=scale_mode, start_sigma=10.0, end_sigma=1.0, blend_scale_offset=0.1, blend_scale_min=0.2,
            blend_scale_max=0.7, blend_strength=0.9)
    add("scale_equal_ends", blend_scale_mode="enabled_range", start_sigma=5.0, end_sigma=5.0, blend_strength=0.9)
    # disabled paths: the hook hands back what it was given
    add("off_window_pre", mode="cond", start_sigma=2.0, end_sigma=1.0)
    add("off_window_post", mode="denoised", start_sigma=2.0, end_sigma=1.0)
    add("off_window_model_input", mode="model_input", start_sigma=2.0, end_sigma=1.0)
    add("off_require_uncond_pre", mode="cond", require_uncond=True, has_uncond=False)
    add("off_require_uncond_post", mode="denoised", require_uncond=True, has_uncond=False)
    add("off_mode_needs_uncond", mode="uncond_sub_cond", has_uncond=False)
    add("off_denoised_sub_uncond_no_uncond", mode="denoised_sub_uncond", has_uncond=False)  # the gate comes before the fallback
    # the fallback to the mode's first word
    add("fallback_cond_plain", has_uncond=False)
    add("fallback_cond_flip", has_uncond=False, pred_flip_mode=True)
    add("ext_without_t2", ops=("ext",), mode="cond", pred_flip_mode=True)
    add("quantile_flip", ops=("quantile",), pred_flip_mode=True, blend_strength=1.0)
    add("advanced_post", ops=("advanced",), mode="denoised_sub_uncond", blend_strength=0.6)
    return cases


CASES = _cases()
HALF_CASES = ("mode_cond_sub_uncond_flip", "chain_post_immediate_False")  # run again on inputs rounded to float16 / bfloat16
HALF_DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}

# One node, its hook called several times: the patch keeps the mode the last enabled call ended with (the reference's ``nonlocal mode``),
# so what a call does may depend on the calls before it.  Each call: (sigma, has_uncond).
def _sequences():
    def seq(ops=("affine",), calls=(), **node):
        assert set(node) <= set(DEFAULTS)
        return dict(node=DEFAULTS | node, ops=list(ops), calls=[dict(sigma=list(s), has_uncond=u) for s, u in calls])

    return {
        # falls back to "cond", then -- the stale "cond" no longer ends in _sub_uncond -- runs as cond_sub_uncond without a t2, then with one
        "seq_fallback_flip": seq(ops=("affine", "ext"), pred_flip_mode=True, blend_strength=0.8,
                                 calls=((PER_SAMPLE, False), ([4.0, 2.0], False), ([3.0, 1.5], True), ([2.0, 1.0], False))),
        "seq_post_gate": seq(mode="denoised_sub_uncond", blend_mode="inject", calls=((PER_SAMPLE, True), ([4.0], False), ([3.0, 1.5], True))),
        "seq_window": seq(mode="uncond_sub_cond", start_sigma=4.5, end_sigma=2.5, blend_scale_mode="reverse_enabled_range", blend_strength=0.9,
                          calls=(([4.0, 3.0], True), (PER_SAMPLE, True), ([3.0], True), ([2.0, 1.0], True), ([4.5, 0.5], False))),
    }


SEQUENCES = _sequences()

# get_blend_scaling table
SCALING_SIGMAS = (0.05, 1.0, 3.3, 5.0, 10.0, 14.6)
SCALING_KW = dict(start_sigma=10.0, end_sigma=1.0, offset=0.1, min_pct=0.05, max_pct=0.95)


def run_case(node_classes: dict, case: dict, tensors: dict):
    """Builds the node from ``node_classes`` for one case and runs its hook once: (model handed in, model returned, result, hook args)."""
    cls = node_classes["SonarApplyLatentOperationCFG"]
    ops = build_ops(case["ops"], node_classes)
    base = ModelPatcher()
    (model,) = getattr(cls, cls.FUNCTION)(model=base, **case["node"], **{f"operation_{i + 1}": op for i, op in enumerate(ops)})
    sigma = torch.tensor(case["sigma"], dtype=torch.float32, device=tensors["x"].device)
    result, args = run_patched(model, tensors, sigma, case["has_uncond"])
    return base, model, result, args


def run_sequence(node_classes: dict, seq: dict, tensors: dict):
    """Builds the node once and calls its hook for every call of the sequence: [(result, hook args), ...]."""
    cls = node_classes["SonarApplyLatentOperationCFG"]
    ops = build_ops(seq["ops"], node_classes)
    (model,) = getattr(cls, cls.FUNCTION)(model=ModelPatcher(), **seq["node"], **{f"operation_{i + 1}": op for i, op in enumerate(ops)})
    out = []
    for call in seq["calls"]:
        sigma = torch.tensor(call["sigma"], dtype=torch.float32, device=tensors["x"].device)
        out.append(run_patched(model, tensors, sigma, call["has_uncond"]))
    return out
