"""CPU: SonarCustomNoiseParameters' host side -- the node is registered with the reference's sockets, the dtypes this build does not
carry are refused by name, the item clones its inner chain, and RNGStates round-trips the host generators."""
import importlib
import json
import os
import random

import pytest
import torch

KEY = "SonarCustomNoiseParameters"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


def _chain(nz):
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    return chain


def _defaults(reg):
    kw = {}
    for name, spec in reg.NODE_ABI[KEY]["inputs"].items():
        if "default" in spec:
            kw[name] = spec["default"]
    return kw


def test_node_is_implemented(reg):
    assert KEY in reg.IMPLEMENTED_KEYS
    assert not reg.NODE_CLASS_MAPPINGS[KEY].__name__.startswith("OffPath_")


def test_sockets_match_the_reference_abi(reg):
    abi = json.load(open(os.path.join(ROOT, "tests", "golden", "node_abi.json")))[KEY]
    cls = reg.NODE_CLASS_MAPPINGS[KEY]
    types = cls.INPUT_TYPES()
    assert list(types["required"]) == [n for n, s in abi["inputs"].items() if s["section"] == "required"]
    assert not types["optional"]
    for name, spec in abi["inputs"].items():
        got = types["required"][name]
        want = tuple(spec["type"]) if isinstance(spec["type"], list) else spec["type"]
        assert got[0] == want, name
        if "default" in spec:
            assert got[1]["default"] == spec["default"], name
    assert cls.RETURN_TYPES == tuple(abi["returns"]) and cls.FUNCTION == abi["function"] and cls.CATEGORY == abi["category"]


def test_the_registry_still_has_54_keys_and_the_refused_ones_refuse(reg, nz):
    assert len(reg.NODE_CLASS_MAPPINGS) == 54 and len(reg.IMPLEMENTED_KEYS) == 42
    for name in ("collatz", "voronoi_fuzz"):
        with pytest.raises(NotImplementedError):
            nz.get_noise_sampler(name, torch.zeros(1, 4, 8, 8), 0.03, 14.6, cpu=True)


def test_node_builds_the_item_from_its_default_sockets(reg, nz):
    node = reg.NODE_CLASS_MAPPINGS[KEY]()
    chain = node.go(custom_noise=_chain(nz), **_defaults(reg))[0]
    assert len(chain.items) == 1
    item = chain.items[0]
    assert isinstance(item, nz.CustomNoiseParametersNoise)
    assert item.override_dtype is None and item.override_device is None and item.normalize is None
    assert (item.rng_mode, item.rng_offset_mode, item.fix_invalid) == ("default", "disabled", False)
    forced = node.go(custom_noise=_chain(nz), **(_defaults(reg) | {"normalize": "forced", "override_device": "cpu", "override_dtype": "bfloat16"}))[0]
    assert forced.items[0].normalize is True and forced.items[0].override_device == "cpu" and forced.items[0].override_dtype is torch.bfloat16


@pytest.mark.parametrize("name", ["float64", "float8_e4m3fn", "float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz", "float8_e8m0fnu", "int64", "int32",
                                  "int16", "int8"])
def test_unsupported_dtypes_are_refused_by_name(reg, nz, name):
    if getattr(torch, name, None) is None:  # this torch build does not have the type: the node refuses it as the reference does
        with pytest.raises(ValueError, match="Bad dtype"):
            reg.NODE_CLASS_MAPPINGS[KEY]().go(custom_noise=_chain(nz), **(_defaults(reg) | {"override_dtype": name}))
        return
    with pytest.raises(NotImplementedError, match=name):
        reg.NODE_CLASS_MAPPINGS[KEY]().go(custom_noise=_chain(nz), **(_defaults(reg) | {"override_dtype": name}))
    with pytest.raises(NotImplementedError, match=name):
        nz.CustomNoiseParametersNoise.resolve_dtype(getattr(torch, name))


def test_a_bad_dtype_name_is_a_value_error(reg, nz):
    for bad in ("float128", "complex64", "default "):
        with pytest.raises(ValueError, match="Bad dtype"):
            reg.NODE_CLASS_MAPPINGS[KEY]().go(custom_noise=_chain(nz), **(_defaults(reg) | {"override_dtype": bad}))
    for ok, want in (("default", None), ("float32", torch.float32), ("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        chain = reg.NODE_CLASS_MAPPINGS[KEY]().go(custom_noise=_chain(nz), **(_defaults(reg) | {"override_dtype": ok}))[0]
        assert chain.items[0].override_dtype is want


def test_clone_clones_the_inner_chain(reg, nz):
    inner = _chain(nz)
    item = reg.NODE_CLASS_MAPPINGS[KEY]().go(custom_noise=inner, **(_defaults(reg) | {"override_dtype": "float16", "rng_state_offset": 5}))[0].items[0]
    assert item.noise is not inner and item.noise.items[0] is not inner.items[0]
    twin = item.clone()
    assert type(twin) is type(item) and twin.keys == item.keys
    assert twin.noise is not item.noise and twin.noise.items[0] is not item.noise.items[0]
    assert twin.noise.items[0].noise_type == item.noise.items[0].noise_type
    assert (twin.factor, twin.override_dtype, twin.rng_state_offset) == (item.factor, torch.float16, 5)
    twin.noise.items[0].set_factor(3.0)
    assert item.noise.items[0].factor == 1.0


def test_square_side(nz):
    side = nz.CustomNoiseParametersNoise.square_side
    assert side(torch.zeros(2, 4, 10, 14)) == (2, 10, 14, 12)
    assert side(torch.zeros(2, 4, 77)) == (1, 1, 77, 9)
    assert side(torch.zeros(1, 4, 6, 24)) == (2, 6, 24, None)
    assert side(torch.zeros(1, 4, 3, 6, 10)) == (2, 6, 10, 8)


def test_rng_states_round_trip_the_host_generators(nz):
    random.seed(11)
    torch.manual_seed(12)
    saved = nz.RNGStates("cpu")
    want = (random.random(), torch.randn(3))
    random.random()
    torch.randn(5)
    saved.set_states()
    got = (random.random(), torch.randn(3))
    assert got[0] == want[0] and torch.equal(got[1], want[1])
    # update() takes the generators as they are now; set_states() puts that back, any number of times
    saved.update()
    nxt = (random.random(), torch.randn(2))
    for _ in range(2):
        saved.set_states()
        assert random.random() == nxt[0] and torch.equal(torch.randn(2), nxt[1])
    # a snapshot does not follow later draws
    other = nz.RNGStates("cpu")
    torch.randn(7)
    other.set_states()
    saved.set_states()
    assert torch.equal(torch.randn(2), nxt[1])
