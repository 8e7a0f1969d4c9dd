"""CPU: SonarApplyLatentOperationCFG's host side -- registration, the socket table against the node ABI, the refusals, which hook each mode
installs, the sigma window, get_blend_scaling against the table read off the reference (tests/golden/make_latent_op_cfg_golden.py), and
the two kernels' entry points against the header."""
import importlib
import inspect
import json
import os
import re

import pytest
import torch

from tests.conftest import GOLDEN
from tests.golden import latent_op_cfg_cases as lc

KEY = "SonarApplyLatentOperationCFG"
ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))[KEY]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sonar_cfg_op_prepare", "sonar_cfg_op_finish")
OPERATIONS = tuple(f"operation_{i}" for i in range(1, 6))


def _registry(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


def _node(pkg):
    return _registry(pkg).NODE_CLASS_MAPPINGS[KEY]


def _meta(golden):
    return json.loads(str(golden("latent_op_cfg")["meta_json"]))


def _go(pkg, **over):
    op = over.pop("operation_1", lambda latent: latent)
    base = lc.ModelPatcher()
    (model,) = _node(pkg).go(model=base, operation_1=op, **(lc.DEFAULTS | over))
    return base, model


def test_node_is_implemented(pkg):
    reg = _registry(pkg)
    assert KEY in reg.IMPLEMENTED_KEYS
    assert not reg.NODE_CLASS_MAPPINGS[KEY].__name__.startswith("OffPath_")
    assert len(reg.NODE_CLASS_MAPPINGS) == 54


def test_sockets_match_the_node_abi(pkg):
    cls = _node(pkg)
    assert tuple(cls.RETURN_TYPES) == ("MODEL",) == tuple(ABI["returns"]) and cls.FUNCTION == "go" == ABI["function"]
    assert cls.CATEGORY == "latent/advanced/operations" == ABI["category"]
    got = cls.INPUT_TYPES()
    for section in ("required", "optional"):
        assert list(got[section]) == [n for n, v in ABI["inputs"].items() if v["section"] == section]
        for name, spec in got[section].items():
            ref = ABI["inputs"][name]
            assert (list(spec[0]) if isinstance(spec[0], tuple) else spec[0]) == ref["type"], name
            for k in ("default", "min", "max"):
                if k in ref:
                    assert spec[1][k] == ref[k], (name, k)
    assert list(got["optional"]) == list(OPERATIONS)
    assert ABI["inputs"]["mode"]["type"] == list(lc.MODES) and ABI["inputs"]["blend_scale_mode"]["type"] == list(lc.BLEND_SCALE_MODES)
    params = inspect.signature(cls.go).parameters
    assert set(params) == set(ABI["inputs"]) and all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params.values())
    assert [n for n, p in params.items() if p.default is not inspect.Parameter.empty] == list(OPERATIONS)


def test_model_input_refusals(pkg):
    for over, text in ((dict(require_uncond=True), "require_uncond"), (dict(pred_flip_mode=True), "pred_flip")):
        base = lc.ModelPatcher()
        with pytest.raises(ValueError, match=text):
            _node(pkg).go(model=base, operation_1=lambda latent: latent, **(lc.DEFAULTS | dict(mode="model_input") | over))
    with pytest.raises(KeyError):
        _go(pkg, blend_mode="no_such_blend")


def test_no_operations_returns_an_unpatched_clone(pkg):
    base = lc.ModelPatcher()
    (model,) = _node(pkg).go(model=base, **lc.DEFAULTS)
    assert model is not base and model.cloned_from is base
    assert model.hooks() == base.hooks() == {"post_cfg": 0, "pre_cfg": 0, "unet_wrapper": 0}


@pytest.mark.parametrize("mode", lc.MODES)
def test_each_mode_installs_its_hook(pkg, golden, mode):
    base, model = _go(pkg, mode=mode)
    want = {"post_cfg": int(mode.startswith("denoised")), "pre_cfg": int(not mode.startswith("denoised") and mode != "model_input"),
            "unet_wrapper": int(mode == "model_input")}
    assert model.hooks() == want == _meta(golden)["cases"][f"mode_{mode}_plain"]["hooks"]
    assert model.cloned_from is base and base.hooks() == {"post_cfg": 0, "pre_cfg": 0, "unet_wrapper": 0}
    latent_ops = importlib.import_module("comfyui_sonar_amd.py.latent_ops")
    for fn in model.post_cfg + model.pre_cfg:
        assert isinstance(fn, latent_ops.LatentOperationCFG) and len(fn.operations) == 1
        assert all(type(o) is latent_ops.SonarLatentOperation for o in fn.operations)


def test_get_blend_scaling_is_the_references(pkg, golden):
    cls = _node(pkg)
    table = _meta(golden)["scaling"]
    assert len(table) == len(lc.BLEND_SCALE_MODES) * len(lc.SCALING_SIGMAS)
    assert list(inspect.signature(cls.get_blend_scaling).parameters) == ["model_sampling", "scale_mode", "sigma", "sigma_t_max", "start_sigma",
                                                                         "end_sigma", "offset", "min_pct", "max_pct"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in inspect.signature(cls.get_blend_scaling).parameters.values())
    ms = lc.ModelPatcher().model.model_sampling
    for mode in lc.BLEND_SCALE_MODES:
        for sigma in lc.SCALING_SIGMAS:
            got = cls.get_blend_scaling(model_sampling=ms, scale_mode=mode, sigma=sigma, sigma_t_max=torch.tensor(sigma, dtype=torch.float32),
                                        **lc.SCALING_KW)
            assert isinstance(got, float) and got == pytest.approx(table[f"{mode}/{sigma}"], rel=1e-6), (mode, sigma)
    with pytest.raises(ValueError, match="blend_scale_mode"):
        cls.get_blend_scaling(model_sampling=ms, scale_mode="no_such_mode", sigma=1.0, sigma_t_max=torch.tensor(1.0), **lc.SCALING_KW)


def test_the_patch_uses_the_nodes_get_blend_scaling(pkg):
    """The reference calls ``cls.get_blend_scaling``: a subclass that overrides the static method changes what its patch scales with."""
    cls = _node(pkg)

    class Halved(cls):
        @staticmethod
        def get_blend_scaling(**kw):
            return 0.5 * cls.get_blend_scaling(**kw)

    (model,) = Halved.go(model=lc.ModelPatcher(), operation_1=lambda latent: latent, **lc.DEFAULTS)
    assert model.pre_cfg[0].blend_scaling is Halved.get_blend_scaling
    assert _go(pkg)[1].pre_cfg[0].blend_scaling is cls.get_blend_scaling


def test_sigma_window_rules(pkg):
    ms = lc.ModelPatcher().model.model_sampling
    smin, smax = ms.sigma_min.item(), ms.sigma_max.item()

    def window(**over):
        (patch,) = _go(pkg, **over)[1].pre_cfg
        return patch.start_sigma, patch.end_sigma, patch.blend_scale_mode

    assert window(start_sigma=-1.0, end_sigma=0.0, blend_scale_mode="sampling") == (smax, smin, "sampling")  # negative start, clamped end
    assert window(start_sigma=1000.0, end_sigma=2.0, blend_scale_mode="sampling") == (smax, 2.0, "sampling")
    assert window(start_sigma=2.0, end_sigma=8.0, blend_scale_mode="enabled_range") == (8.0, 2.0, "enabled_range")  # reversed ends swap
    assert window(start_sigma=5.0, end_sigma=5.0, blend_scale_mode="enabled_range") == (5.0, 5.0, "none")  # no range to take a percentage of
    assert window(start_sigma=0.0, end_sigma=0.0, blend_scale_mode="sampling_sin") == (smin, smin, "none")  # equal after the clamp


def test_entry_points_are_declared_and_exported(pkg):
    hl = pkg.hip_lib
    text = open(os.path.join(ROOT, "include", "sonar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    kinds = {"float": hl.C.c_float, "int": hl.C.c_int, "int64_t": hl.C.c_int64}
    lib = hl.load()
    for name in ENTRY_POINTS:
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert restype is hl.C.c_int and len(params) == len(argtypes) and params[0] == "int dtype" and params[-1] == "void* stream", name
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), (name, p)
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    defs = {m.group(1): int(m.group(2).strip("()")) for m in re.finditer(r"#define SONAR_(DTYPE_\w+|CFG_\w+) (\(?-?\d+\)?)", text)}
    assert defs == {"DTYPE_F32": 0, "DTYPE_F16": 1, "DTYPE_BF16": 2, "CFG_BLEND_NONE": hl.CFG_BLEND_NONE}
    assert hl.DTYPE_IDS == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2} and hl.CFG_BLEND_NONE not in hl.BLEND_IDS.values()
    assert os.path.exists(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "cfg_op.hip"))
