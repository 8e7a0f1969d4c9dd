"""CPU: SonarNoiseImage's host side -- registration, the socket table against the node ABI, the channel-target table against the one read
off the reference's outputs (tests/golden/make_image_noise_golden.py), the refusals that need no device, and the compose entry points
against the header."""
import importlib
import inspect
import json
import os
import re

import pytest
import torch

from tests.conftest import GOLDEN

KEY = "SonarNoiseImage"
ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))[KEY]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sonar_image_channel_mean_f32", "sonar_image_noise_compose_f32", "sonar_image_rescale_f32")


def _registry(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


def _meta(golden):
    return json.loads(str(golden("image_noise")["meta_json"]))


def _sockets(**over):
    kw = {k: v["default"] for k, v in ABI["inputs"].items() if "default" in v}
    kw.update(seed=1, **over)
    return kw


def test_node_is_implemented(pkg):
    reg = _registry(pkg)
    assert KEY in reg.IMPLEMENTED_KEYS
    cls = reg.NODE_CLASS_MAPPINGS[KEY]
    assert not cls.__name__.startswith("OffPath_")
    assert len(reg.NODE_CLASS_MAPPINGS) == 54
    # the nodes that stay outside the path still refuse
    for key in ("SonarAdvancedCollatzNoise", "SonarAdvancedVoronoiNoise"):
        off = reg.NODE_CLASS_MAPPINGS[key]
        with pytest.raises(NotImplementedError):
            getattr(off(), off.FUNCTION)()


def test_sockets_match_the_node_abi(pkg):
    cls = _registry(pkg).NODE_CLASS_MAPPINGS[KEY]
    assert tuple(cls.RETURN_TYPES) == ("IMAGE",) == tuple(ABI["returns"]) and cls.FUNCTION == ABI["function"] and cls.CATEGORY == ABI["category"]
    got = cls.INPUT_TYPES()
    for section in ("required", "optional"):
        assert list(got[section]) == [n for n, v in ABI["inputs"].items() if v["section"] == section]
        for name, spec in got[section].items():
            ref = ABI["inputs"][name]
            assert (list(spec[0]) if isinstance(spec[0], tuple) else spec[0]) == ref["type"], name
            for k in ("default", "min", "max"):
                if k in ref:
                    assert spec[1][k] == ref[k], (name, k)
    # the function takes exactly the sockets, by keyword, and only the optional one has a default
    params = inspect.signature(getattr(cls, cls.FUNCTION)).parameters
    assert set(params) == set(ABI["inputs"])
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params.values())
    assert [n for n, p in params.items() if p.default is not inspect.Parameter.empty] == ["custom_noise_opt"]
    assert len(ABI["inputs"]["channel_mode"]["type"]) == 15


def test_channel_targets_are_the_references(pkg, golden):
    cls = _registry(pkg).NODE_CLASS_MAPPINGS[KEY]
    table = _meta(golden)["targets"]
    modes = ABI["inputs"]["channel_mode"]["type"]
    assert len(table) == 15 * 3
    for channels in (1, 3, 4):
        for mode in modes:
            assert sorted(cls.channel_targets(mode, channels)) == table[f"{mode}/{channels}"], (mode, channels)
            assert cls.channel_targets(mode.lower(), channels) == cls.channel_targets(mode, channels)
    # the quirk, spelled out: "G" is channel 2 and "B" channel 1; "A" on an RGB image selects nothing; other counts take every channel
    assert cls.channel_targets("G", 3) == (2,) and cls.channel_targets("B", 4) == (1,) and cls.channel_targets("A", 3) == ()
    assert cls.channel_targets("R", 2) == (0, 1) and cls.channel_targets("A", 5) == (0, 1, 2, 3, 4)


def test_refusals_need_no_device(pkg, golden):
    cls = _registry(pkg).NODE_CLASS_MAPPINGS[KEY]
    g, meta = golden("image_noise"), _meta(golden)["cases"]
    refused = {name: m for name, m in meta.items() if m["error"]}
    assert sorted(refused) == ["refuse_2d", "refuse_5d"]
    for name, m in refused.items():
        image = g[f"image_{m['image']}"]
        assert image.ndim in (2, 5) and m["error"] == "ValueError"
        with pytest.raises(ValueError, match="3 or 4 dimensions"):
            cls.go(**_sockets(image=image))
    with pytest.raises(NotImplementedError, match="float64"):
        cls.go(**_sockets(image=torch.zeros(1, 4, 4, 3), dtype="float64"))
    with pytest.raises(NotImplementedError, match="float64"):
        cls.go(**_sockets(image=torch.zeros(1, 4, 4, 3, dtype=torch.float64)))
    with pytest.raises(KeyError):
        cls.go(**_sockets(image=torch.zeros(1, 4, 4, 3), blend_mode="no_such_blend"))


def test_entry_points_are_declared_in_the_header(pkg):
    hl = pkg.hip_lib
    text = open(os.path.join(ROOT, "include", "sonar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert len(params) == len(argtypes) and params[-1] == "void* stream", name
        # the ctypes kinds follow the declared types
        kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64, "uint64_t": hl.C.c_uint64}
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), (name, p)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SONAR_(IMAGE_\w+) (\d+)", text)}
    assert defs == {"IMAGE_BLEND_ADD": 3, "IMAGE_NPART": hl.IMAGE_NPART, "IMAGE_MAX_CHANNELS": hl.IMAGE_MAX_CHANNELS}
    assert hl.IMAGE_BLEND_IDS == {"lerp": 0, "inject": 1, "subtract_b": 2, "simple_add": defs["IMAGE_BLEND_ADD"]}
    assert os.path.exists(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "image_noise.hip"))
