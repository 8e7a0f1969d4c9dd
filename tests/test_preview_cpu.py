"""CPU: the host side of the filter previews of SonarPowerNoise / SonarPowerFilterNoise -- the fixture's shapes against the panel-width
rule, the temp-PNG hand-over to the UI (inside ComfyUI and without it), the ``preview`` sockets, and ``preview="none"`` as no preview at
all.  The pictures themselves are composed on the device: tests/test_gpu_preview.py."""
import importlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests.conftest import GOLDEN

ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))
NPZ = np.load(os.path.join(GOLDEN, "preview.npz"), allow_pickle=False)
META = json.loads(str(NPZ["meta_json"]))
SIZES = ((8, 8), (8, 6), (6, 10), (7, 9), (9, 7), (16, 12), (128, 128))


def filter_panel_width(w):
    """The issue's rule, restated: the mirrored half drops column 0 always and the last column only when Wh is odd."""
    wh = w // 2 + 1
    return 2 * wh - 2 if wh % 2 else 2 * wh - 1


@pytest.fixture(scope="module")
def pn(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.powernoise")


def test_panel_width_rule_examples(pkg):
    assert [filter_panel_width(w) for w in (6, 9, 8, 10, 7, 12, 128)] == [7, 8, 8, 11, 7, 12, 128]
    assert all(pkg.hip_lib.preview_filter_width(w) == filter_panel_width(w) for w in range(2, 300))


def test_fixture_shapes_follow_the_panel_width_rule():
    cases = META["cases"]
    assert {tuple(c["size"]) for c in cases.values()} == set(SIZES)
    assert {c["filter"] for c in cases.values()} == {"band", "band_mid", "shaped", "composed", "node"}
    assert {(c["mix"], c["norm"]) for c in cases.values()} == {(1.0, 1.0), (0.5, 1.0), (1.0, 0.5), (0.5, 0.5)}
    for name, case in cases.items():
        h, w = case["size"]
        fw = filter_panel_width(w)
        assert NPZ[f"{name}/filter_panel"].shape == (1, 1, h, fw) and NPZ[f"{name}/filter_panel"].dtype == np.float32, name
        assert NPZ[f"{name}/kernel_panel"].shape == (1, 1, h, w), name
        assert NPZ[f"{name}/image"].shape == (h, fw + 2 * w) and NPZ[f"{name}/image"].dtype == np.uint8, name
        assert NPZ[f"{name}/spectrum"].shape == (1, 1, h, w // 2 + 1) and NPZ[f"{name}/spectrum"].dtype == np.complex64, name
        # what the generator checked before it stored the case
        assert case["fp64_share"] < 0.01 and case["fp64_worst"] <= 1, name
    for h, w in META["small"]:
        assert NPZ[f"fft2/{h}x{w}/in"].shape == (1, 2, h, w // 2 + 1) and NPZ[f"fft2/{h}x{w}/out"].shape == (1, 2, h, filter_panel_width(w))
    assert [tuple(s) for s in META["small"]] == list(SIZES[:5])


def check_result(out, folder, result, size):
    assert set(out) == {"ui", "result"} and out["result"] is result and set(out["ui"]) == {"images"} and len(out["ui"]["images"]) == 1
    entry = out["ui"]["images"][0]
    assert set(entry) == {"filename", "subfolder", "type"} and entry["type"] == "temp" and entry["subfolder"] == ""
    assert entry["filename"].startswith("sonar_temp_") and entry["filename"].endswith("_00000_.png")
    path = os.path.join(folder, entry["filename"])
    with Image.open(path) as img:
        img.load()
        assert img.format == "PNG" and img.size == size and img.mode == "L"
        return path, np.asarray(img).copy()


def test_make_preview_result_inside_and_outside_comfyui(pn, tmp_path, monkeypatch):
    pixels = np.arange(5 * 23, dtype=np.uint8).reshape(5, 23)
    img, result = Image.fromarray(pixels), ("the chain",)
    state = random.getstate()
    # inside ComfyUI: folder_paths names the directory and the file
    calls = []

    def get_save_image_path(prefix, directory):
        calls.append((prefix, directory))
        return directory, prefix, 0, "", prefix

    monkeypatch.setitem(sys.modules, "folder_paths",
                        types.SimpleNamespace(get_temp_directory=lambda: str(tmp_path), get_save_image_path=get_save_image_path))
    path, back = check_result(pn.make_preview_result(img, result), str(tmp_path), result, (23, 5))
    assert np.array_equal(back, pixels) and len(calls) == 1 and calls[0][1] == str(tmp_path) and calls[0][0].startswith("sonar_temp_")
    assert os.listdir(tmp_path) == [os.path.basename(path)]
    # a second picture gets another name
    assert pn.make_preview_result(img, result, prefix="other")["ui"]["images"][0]["filename"].startswith("other_")
    assert len(os.listdir(tmp_path)) == 2
    # outside: the system's temp directory (None in sys.modules makes the import fail)
    monkeypatch.setitem(sys.modules, "folder_paths", None)
    path, back = check_result(pn.make_preview_result(img, result), tempfile.gettempdir(), result, (23, 5))
    os.remove(path)
    assert np.array_equal(back, pixels)
    assert random.getstate() == state, "the file names must not draw from the global random state"


@pytest.mark.parametrize("key,choices", [("SonarPowerNoise", ["none", "no_mix", "mix"]),
                                         ("SonarPowerFilterNoise", ["none", "no_mix", "mix", "custom"])])
def test_preview_socket_choices(pkg, key, choices):
    assert ABI[key]["inputs"]["preview"]["type"] == choices
    spec = pkg.NODE_CLASS_MAPPINGS[key].INPUT_TYPES()["required"]["preview"]
    assert list(spec[0]) == choices


def same_value(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and torch.equal(a, b)
    if hasattr(a, "items") and hasattr(b, "items") and not isinstance(a, dict):  # a chain: item by item
        return same_chain(a, b)
    if hasattr(a, "_FIELDS"):  # a PowerFilter
        return type(a) is type(b) and all(same_value(getattr(a, f), getattr(b, f)) for f in (*a._FIELDS, "compose_with"))
    return type(a) is type(b) and a == b


def same_chain(a, b):
    if type(a) is not type(b) or len(a.items) != len(b.items):
        return False
    return all(type(x) is type(y) and x.factor == y.factor and x.keys == y.keys and all(same_value(getattr(x, k), getattr(y, k)) for k in x.keys)
               for x, y in zip(a.items, b.items))


def power_noise_sockets(**over):
    kw = {k: v["default"] for k, v in ABI["SonarPowerNoise"]["inputs"].items() if "default" in v}
    kw.pop("preview")
    return dict(kw, **over)


def test_preview_none_is_the_call_without_the_argument(pkg):
    M = pkg.NODE_CLASS_MAPPINGS
    nz = importlib.import_module("comfyui_sonar_amd.py.noise")
    kw = power_noise_sockets(alpha=1.0, mix=0.5, rescale=2.0)
    with_none, without = M["SonarPowerNoise"]().go(preview="none", **kw), M["SonarPowerNoise"]().go(**kw)
    assert isinstance(with_none, tuple) and len(with_none) == 1 and same_chain(with_none[0], without[0])
    assert with_none[0].items[0].mix == 0.5 and not hasattr(with_none[0].items[0], "preview_type")
    inner = nz.CustomNoiseChain()
    inner.add(nz.CustomNoiseItem(1.0, noise_type=nz.NoiseType.GAUSSIAN))
    (filt,) = M["SonarPowerFilter"].go(alpha=1.0, max_freq=0.5, min_freq=0.0, stretch=1.0, rotate=0.0, pnorm=2.0, oversample=4, blur=0.125, scale=1.0,
                                       compose_mode="max")
    kw = dict(factor=1.0, rescale=0.0, mix=1.0, common_mode=0.0, channel_correlation="1, 1, 1, 1, 1, 1", sonar_custom_noise=inner,
              sonar_power_filter=filt, filter_norm_factor=0.5, normalize_result="default", normalize_noise="forced")
    with_none, without = M["SonarPowerFilterNoise"]().go(preview="none", **kw), M["SonarPowerFilterNoise"]().go(**kw)
    assert isinstance(with_none, tuple) and len(with_none) == 1 and same_chain(with_none[0], without[0])
    assert with_none[0].items[0].filter_norm_factor == 0.5 and with_none[0].items[0].normalize_noise is True


def test_custom_preview_names_the_missing_module(pn, pkg, monkeypatch):
    """Outside ComfyUI the colour preview has nothing to decode with: refused before any device work, so this needs no GPU."""
    nz = importlib.import_module("comfyui_sonar_amd.py.noise")
    inner = nz.CustomNoiseChain()
    inner.add(nz.CustomNoiseItem(1.0, noise_type=nz.NoiseType.GAUSSIAN))
    monkeypatch.setitem(sys.modules, "latent_preview", None)
    item = pn.PowerFilterNoiseItem(1.0, noise=inner, normalize_noise=None, normalize_result=None, power_filter=pn.PowerFilter(), mix=1.0,
                                   common_mode=0.0, channel_correlation="1, 1, 1, 1, 1, 1", time_brownian=True, preview_type="custom")
    with pytest.raises(NotImplementedError, match="latent_preview"):
        item.preview()


def test_a_broken_host_module_is_not_taken_for_a_missing_one(pn, tmp_path, monkeypatch):
    """folder_paths exists but cannot import something of its own: that failure surfaces, the picture is not quietly saved elsewhere."""
    (tmp_path / "folder_paths.py").write_text("import sonar_preview_test_no_such_dependency\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    monkeypatch.delitem(sys.modules, "folder_paths", raising=False)
    before = set(os.listdir(tempfile.gettempdir()))
    with pytest.raises(ModuleNotFoundError, match="sonar_preview_test_no_such_dependency"):
        pn.make_preview_result(Image.new("L", (4, 4)), ("chain",))
    assert not [f for f in set(os.listdir(tempfile.gettempdir())) - before if f.startswith("sonar_temp_")]
    sys.modules.pop("folder_paths", None)
    assert pn._host_module("sonar_preview_test_no_such_package.sub") is None and pn._host_module("sonar_preview_test_no_such_module") is None
