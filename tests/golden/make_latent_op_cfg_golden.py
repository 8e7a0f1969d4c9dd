"""Generates tests/golden/latent_op_cfg.npz by running the REAL reference's SonarApplyLatentOperationCFG (imported through
oracle/ref_import.py, plus its nodes.latent_operations module) on the CPU, behind the model stand-in of latent_op_cfg_cases.py: the inputs,
what the installed hook returned for every case and for every call of the multi-call sequences (or which of its arguments it handed
back), and a table of get_blend_scaling values.

    python tests/golden/make_latent_op_cfg_golden.py
"""
from __future__ import annotations

import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle.ref_import import ALIAS, load_reference  # noqa: E402
from tests.golden import latent_op_cfg_cases as lc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "latent_op_cfg.npz")
load_reference()
ref_ops = importlib.import_module(f"{ALIAS}.nodes.latent_operations")
NODES = {"SonarApplyLatentOperationCFG": ref_ops.SonarApplyLatentOperationCFG,
         "SonarLatentOperationQuantileFilter": ref_ops.SonarLatentOperationQuantileFilter,
         "SonarLatentOperationAdvanced": ref_ops.SonarLatentOperationAdvancedNode}


def returned(result, args):
    """Which of its arguments the hook handed back untouched, or None."""
    for name in ("conds_out", "denoised", "input"):
        if result is args.get(name):
            return name
    return None


def run(case, tensors, arrays, key, entry):
    before = {k: v.clone() for k, v in tensors.items()}
    base, model, result, args = lc.run_case(NODES, case, tensors)
    assert model is not base and model.cloned_from is base and base.hooks() == {"post_cfg": 0, "pre_cfg": 0, "unet_wrapper": 0}
    assert all(torch.equal(tensors[k], before[k]) for k in tensors), key
    entry["hooks"] = model.hooks()
    record(result, args, arrays, key, entry)


def record(result, args, arrays, key, entry):
    """What one hook call returned: the argument it handed back, or the tensor (pre-CFG: the one replaced entry of a new list)."""
    entry["returned"] = returned(result, args)
    if entry["returned"] is not None:
        return
    if isinstance(result, list):
        conds = args["conds_out"]
        changed = [i for i, (a, b) in enumerate(zip(result, conds)) if a is not b]
        assert result is not conds and len(result) == len(conds) and len(changed) == 1, key
        entry["replaced"] = changed[0]
        result = result[changed[0]]
    assert result.dtype == torch.float32 and tuple(result.shape) == lc.SHAPE, key
    arrays[f"out_{key}"] = result.numpy()


def main():
    tensors = lc.inputs()
    arrays = {f"in_{k}": v.numpy() for k, v in tensors.items()}
    meta = {"cases": {}, "half": {}}
    for name, case in lc.CASES.items():
        entry = meta["cases"][name] = dict(case)
        run(case, tensors, arrays, name, entry)
    for name in lc.HALF_CASES:
        for tag, dtype in lc.HALF_DTYPES.items():
            rounded = {k: v.to(dtype).float() for k, v in tensors.items()}  # the reference computes in fp32 on the rounded values
            entry = meta["half"][f"{name}__{tag}"] = dict(lc.CASES[name], case=name, dtype=tag)
            run(lc.CASES[name], rounded, arrays, f"{name}__{tag}", entry)
    meta["sequences"] = {}
    for name, seq in lc.SEQUENCES.items():
        entry = meta["sequences"][name] = dict(seq, results=[])
        for i, (result, args) in enumerate(lc.run_sequence(NODES, seq, tensors)):
            entry["results"].append({})
            record(result, args, arrays, f"{name}__{i}", entry["results"][-1])
        assert any(r["returned"] for r in entry["results"]) or name == "seq_fallback_flip", name
    ms = lc.ModelPatcher().model.model_sampling
    table = {}
    for mode in lc.BLEND_SCALE_MODES:
        for sigma in lc.SCALING_SIGMAS:
            table[f"{mode}/{sigma}"] = float(ref_ops.SonarApplyLatentOperationCFG.get_blend_scaling(
                model_sampling=ms, scale_mode=mode, sigma=sigma, sigma_t_max=torch.tensor(sigma, dtype=torch.float32), **lc.SCALING_KW))
    meta["scaling"] = table
    arrays["meta_json"] = np.array(json.dumps(meta, sort_keys=True))
    with open(OUT, "wb") as fh:  # np.savez_compressed stamps no times into the archive, so a rerun is byte-identical
        np.savez_compressed(fh, **dict(sorted(arrays.items())))
    stored = sum(1 for k in arrays if k.startswith("out_"))
    print(f"{os.path.basename(OUT)}  {len(meta['cases'])} cases + {len(meta['half'])} half + {len(meta['sequences'])} sequences  {stored} outputs  {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
