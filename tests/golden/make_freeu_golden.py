"""Generates tests/golden/freeu_extreme.npz by running the REAL reference's FreeUExtremeConfig / FreeUExtremeNode (imported through
oracle/ref_import.py) on the CPU, in the build container only:

    python tests/golden/make_freeu_golden.py

Recorded: inputs, the normalised filter the reference built, apply() outputs in float32 / float16 / bfloat16 (tests/freeu_refs.py lists
the cases), and the reference's answers to the host-logic questions: get_config_list, check_match, and which configs the handler applies.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import load_reference  # noqa: E402
from tests import freeu_refs as R  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ref = load_reference()
fx = importlib.import_module("sonar_ref.nodes.freeu_extreme")
PF = ref.powernoise.PowerFilter
TORCH_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def config(kw, fname, **more):
    return fx.FreeUExtremeConfig(target="both", stage_1=True, sonar_power_filter_opt=None if fname is None else PF(**R.FILTERS[fname]), **kw, **more)


def main():
    out = {}
    for n, (tag, (shape, kw, fname)) in enumerate(R.CASES.items()):
        x = torch.from_numpy(R.make_input(shape, 100 + n))
        out[f"{tag}_x"] = x
        for dname, dt in TORCH_DTYPES.items():
            cache = {}
            xin = x.clone().to(dt)
            got = config(kw, fname).apply(0, xin, cache)
            assert got is xin
            out[f"{tag}_out_{dname}"] = got.float()
            if fname is not None and dname == "float32" and cache:
                (filt,) = cache.values()
                out[f"{tag}_filter"] = filt.float().reshape(shape[-2], shape[-1] // 2 + 1)
        assert torch.isfinite(out[f"{tag}_out_float32"]).all(), tag

    # two stacked non-final configs, in order
    shape, (kw1, f1), (kw2, f2) = R.STACK
    x = torch.from_numpy(R.make_input(shape, 200))
    cache = {}
    y = x.clone()
    for idx, (kw, fname) in enumerate(((kw1, f1), (kw2, f2))):
        y = config(kw, fname).apply(idx, y, cache)
    out["stack_x"], out["stack_out"] = x, y
    out["stack_filter"] = cache[(0, torch.Size(shape[-2:]))].float().reshape(shape[-2], shape[-1] // 2 + 1)

    # a cache hit wins over the config's own filter
    shape, kw, f_cfg, f_cached = R.CACHE_HIT
    x = torch.from_numpy(R.make_input(shape, 300))
    cache = {}
    config(kw, f_cached).apply(7, x.clone(), cache)
    held = cache[(7, torch.Size(shape[-2:]))]
    out["hit_x"], out["hit_out"] = x, config(kw, f_cfg).apply(7, x.clone(), cache)
    out["hit_filter"] = held.float().reshape(shape[-2], shape[-1] // 2 + 1)
    assert cache[(7, torch.Size(shape[-2:]))] is held

    # an all-zero map: the hidden mean is constant, 0 / 0
    z = torch.zeros(1, 4, 8, 8)
    out["zero_out"] = config(dict(scale=1.3, hidden_mean=True), None).apply(0, z, {})
    assert torch.isnan(out["zero_out"]).all()

    # ---- host logic
    def chain(spec):
        nxt = None
        made = []
        for i in reversed(range(len(spec))):
            nxt = fx.FreeUExtremeConfig(**spec[i], frux_config_opt=nxt)
            nxt.tag = i
            made.append(nxt)
        return nxt, made[::-1]

    head, cfgs = chain(R.CHAIN)
    out["chain_list"] = np.array([c.tag for c in head.get_config_list()], dtype=np.int64)
    bad_head, _ = chain(R.CHAIN_BAD_HEAD)
    out["chain_bad_head_list"] = np.array([c.tag for c in bad_head.get_config_list()], dtype=np.int64)
    out["check_match"] = np.array([[bool(c.check_match(*q)) for q in R.QUERIES] for c in cfgs], dtype=np.bool_)

    # the handler: which configs apply, in order, for (channels, sigma) through each patch; apply() is replaced by a recorder
    applied = []
    fx.FreeUExtremeConfig.apply = lambda self, idx, x, filter_cache, cpu_fft=False: (applied.append((idx, self.tag)), x)[1]

    class Model:
        model = types.SimpleNamespace(model_config=types.SimpleNamespace(unet_config={"model_channels": R.MODEL_CHANNELS}))

        def __init__(self):
            self.patches = {}

        def clone(self):
            return self

        def get_model_object(self, name):
            assert name == "model_sampling"
            return types.SimpleNamespace(timestep=lambda sigma: sigma)

        def set_model_input_block_patch(self, p):
            self.patches["input"] = p

        def set_model_patch(self, p, name):
            self.patches[name] = p

        def set_model_output_block_patch(self, p):
            self.patches["output"] = p

    (m,) = fx.FreeUExtremeNode.go(Model(), False, input_config=head, output_config=head)
    assert set(m.patches) == {"input", "output"}
    rows = []
    for ch in R.HANDLER_CHANNELS:
        for sg in R.HANDLER_SIGMAS:
            top = {"sigmas": torch.tensor([sg, sg * 0.5])}
            h = torch.zeros(1, ch, 2, 2)
            applied.clear()
            assert m.patches["input"](h, top) is h
            seq_in = list(applied)
            applied.clear()
            hsp = torch.zeros(1, ch + 1, 2, 2)  # the skip tensor's own channel count must not matter: the stage comes from h
            m.patches["output"](h, hsp, top)
            rows.append((seq_in, list(applied)))
    width = max(max(len(a), len(b)) for a, b in rows)
    pack = lambda seq: [t for _i, t in seq] + [-1] * (width - len(seq))  # noqa: E731
    out["handler_input"] = np.array([pack(a) for a, _ in rows], dtype=np.int64)
    out["handler_output"] = np.array([pack(b) for _, b in rows], dtype=np.int64)
    out["handler_output_idx"] = np.array([[i for i, _t in b] + [-1] * (width - len(b)) for _, b in rows], dtype=np.int64)

    conv = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(OUT, "freeu_extreme.npz")
    np.savez_compressed(path, **conv)
    print(f"freeu_extreme.npz  {os.path.getsize(path) / 1024:.1f} KiB; E = {R.reference_error(conv):.3e}")


if __name__ == "__main__":
    main()
