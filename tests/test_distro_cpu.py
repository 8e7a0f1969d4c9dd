"""CPU: Distro noise's host side -- the family table against the node ABI, node registration, the result_index trimming against torch
indexing, the family codes against the header, and the numpy statement of the generate-mode stream (key / counter layout and word
conversions) that tests/test_gpu_distro.py compares the kernel with."""
import importlib
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from oracle.device_streams import philox4x32
from tests.conftest import GOLDEN

ABI = json.load(open(os.path.join(GOLDEN, "node_abi.json")))["SonarAdvancedDistroNoise"]["inputs"]
DOMAIN = 0x44495354


# ------------------------------------------------------------------------------------------------ the stream contract in numpy
def distro_block(seed: int, stream: int, idx, block: int):
    """The four words of block ``block`` of global elements ``idx``: Philox4x32-10, key (seed_lo, seed_hi ^ DOMAIN), counter
    (idx_lo, idx_hi | stream_hi << 16, block, stream_lo)."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & (2**64 - 1)
    c1 = (idx >> np.uint64(32)) | np.uint64(((stream >> 32) << 16) & 0xFFFFFFFF)
    return philox4x32(idx & np.uint64(0xFFFFFFFF), c1, np.full_like(idx, block), np.full_like(idx, stream & 0xFFFFFFFF),
                      seed & 0xFFFFFFFF, (seed >> 32) ^ DOMAIN)


def u_open(w):
    """((w >> 9) + 1/2) 2^-23 in (0, 1), exact in fp32 (24 significant bits)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0**-23


def u_half(w):
    """(w >> 8) 2^-24 in [0, 1), exact in fp32."""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0**-24


def normal_of(words):
    """Box-Muller, cosine branch, of words 0 and 1."""
    return np.sqrt(-2.0 * np.log(u_open(words[0]))) * np.cos(2.0 * np.pi * u_half(words[1]))


def _pkg_modules(pkg):
    return (importlib.import_module("comfyui_sonar_amd.py.noise_generation"), importlib.import_module("comfyui_sonar_amd.py.nodes.registry"))


def test_family_table_is_the_node_abi(pkg):
    ng, _ = _pkg_modules(pkg)
    gen = ng.DistroNoiseGenerator
    assert tuple(sorted(gen.FAMILIES)) == tuple(ABI["distribution"]["type"])
    assert ABI["distribution"]["default"] == "uniform"
    params = gen.build_params()
    sockets = [k for k in ABI if k.split("_")[0] in {f.split("_")[0] for f in gen.FAMILIES} and k != "distribution"]
    assert list(params) == sockets  # names and order
    for key, default in params.items():
        assert default == ABI[key]["default"] and type(default) is type(ABI[key]["default"]), key
        assert ABI[key]["type"] == ("STRING" if isinstance(default, str) else "INT" if isinstance(default, int) else "FLOAT"), key
    ngp = gen.ng_params()
    assert ngp["distro"] == "normal" and ngp["result_index"] == "-1" and ngp["quantile_norm_dim"] == 1
    assert set(gen.SIMPLE) == {"exponential", "cauchy", "geometric", "log_normal", "normal"}


def test_node_is_implemented(pkg):
    _, reg = _pkg_modules(pkg)
    assert "SonarAdvancedDistroNoise" in reg.IMPLEMENTED_KEYS
    cls = reg.NODE_CLASS_MAPPINGS["SonarAdvancedDistroNoise"]
    assert not cls.__name__.startswith("OffPath_")
    assert len(reg.NODE_CLASS_MAPPINGS) == 54
    noise = importlib.import_module("comfyui_sonar_amd.py.noise")
    item = noise.AdvancedDistroNoise(1.0, distro="beta", result_index=(0,))
    assert item.sampler_factory is not None and "beta_concentration0" in noise.AdvancedDistroNoise.ns_factory_arg_keys


def test_node_modes_and_result_index(pkg):
    """The node maps quantile_norm_mode to (dim, flatten) and parses result_index into ints; the chain item carries them."""
    _, reg = _pkg_modules(pkg)
    node = reg.NODE_CLASS_MAPPINGS["SonarAdvancedDistroNoise"]()
    kw = {k: v["default"] for k, v in ABI.items() if "default" in v}
    want = {"global": (None, True), "batch": (0, True), "channel": (1, True), "batch_row": (2, True), "batch_col": (3, True),
            "nonflat_row": (2, False), "nonflat_col": (3, False)}
    for mode, (dim, flat) in want.items():
        chain = node.go(**(kw | {"quantile_norm_mode": mode, "result_index": " 2 -1  0", "distribution": "gamma"}))[0]
        item = chain.items[0]
        assert (getattr(item, "quantile_norm_dim", None), item.quantile_norm_flatten) == (dim, flat)
        assert item.result_index == (2, -1, 0) and item.distro == "gamma"


@pytest.mark.parametrize("trial", range(40))
def test_trimming_matches_torch_indexing(pkg, trial):
    ng, _ = _pkg_modules(pkg)
    rnd = random.Random(trial)
    lead = tuple(rnd.randint(1, 3) for _ in range(rnd.randint(1, 3)))
    extra = tuple(rnd.randint(1, 5) for _ in range(rnd.randint(0, 3)))
    ri = tuple(rnd.randint(-7, 7) for _ in range(rnd.randint(1, 3)))
    x = torch.randn(lead + extra)
    got = ng.trim_result_index(x, len(lead), ri)
    want = x
    for t in range(len(extra)):  # trailing dims from the last: index ri[t % len], negative from the end, clamped
        size = want.shape[-1]
        i = ri[t % len(ri)]
        i = min(max(i + size if i < 0 else i, 0), size - 1)
        want = want.select(-1, i)
    assert torch.equal(got, want)
    assert ng.trim_result_index(x, x.ndim, ()) is x  # nothing to trim: the list is not looked at
    if extra:
        with pytest.raises(ValueError):
            ng.trim_result_index(x, len(lead), ())
        with pytest.raises(TypeError):
            ng.trim_result_index(x, len(lead), "-1")


def test_parameter_parsing(pkg):
    ng, _ = _pkg_modules(pkg)
    p = ng.DistroNoiseGenerator._param
    assert p("0.5  2.0", None).tolist() == [0.5, 2.0] and p("0.5  2.0", None).dtype == torch.float32
    assert p(3, None).tolist() == [3.0]
    assert p("2.5", float) == 2.5 and p(3, int) == 3 and p("4", int) == 4
    with pytest.raises(ValueError, match="Couldn't return result as float"):
        p("1.0 2.0", float)


def test_family_codes_match_the_header(pkg):
    hl = pkg.hip_lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "sonar_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define SONAR_(DISTRO_\w+) (0x[0-9a-fA-F]+u?|\d+)", header.replace("u\n", "\n"))}
    assert len(defs) == 29
    for name, val in defs.items():
        assert getattr(hl, name) == val, name
    ng, _ = _pkg_modules(pkg)
    codes = [getattr(hl, f"DISTRO_{f.upper()}") for f in ng.DistroNoiseGenerator.FAMILIES]
    assert codes == list(range(26))
    assert DOMAIN == hl.DISTRO_DOMAIN
    import ctypes

    assert ctypes.sizeof(hl.DistroParams) == 4 * 4 + 3 * 4 + 16 * 4


def test_stream_statement(pkg):
    """The numpy statement: Random123's known answer through the same function, distinct (seed, stream) pairs that collide under an
    exclusive-or of the two give distinct words, the stream's high word lands in counter word 1, and the conversions' ranges."""
    kat = philox4x32(np.uint64(0), np.uint64(0), np.uint64(0), np.uint64(0), 0, 0)
    assert [int(v) for v in kat] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    idx = np.arange(64, dtype=np.uint64)
    a = np.stack(distro_block(5, 3, idx, 0))
    b = np.stack(distro_block(6, 0, idx, 0))  # 5 ^ 3 == 6 ^ 0
    c = np.stack(distro_block(5, 3, idx, 1))
    d = np.stack(distro_block(5, 3 + (1 << 32), idx, 0))
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)
    e = np.stack(distro_block(5, 3, idx + np.uint64(1 << 48), 0))  # idx and stream share counter word 1: idx < 2^48 keeps them apart
    assert not np.array_equal(a, e)
    w = np.array([0, 255, 256, 0xFFFFFFFF], dtype=np.uint64)
    assert u_open(w).min() > 0.0 and u_open(w).max() < 1.0 and u_half(w)[0] == 0.0 and u_half(w).max() < 1.0
    assert np.all(np.float32(u_open(w)) == u_open(w))
    z = normal_of(distro_block(1, 2, np.arange(1 << 14, dtype=np.uint64), 0))
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05
