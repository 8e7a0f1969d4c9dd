"""CPU: ShuffledNoise / utils.elementwise_shuffle_by_dim -- the exports and their parameter names, the reference's early returns and
refusals, the unchanged registry, the two entry points of csrc/shuffle.hip declared, bound and exported, a launchable call on a CPU tensor,
the golden file against its case table, and the host restatement of the generate-mode contract (tests/shuffle_refs.py), which
tests/test_gpu_shuffle.py holds the kernel to."""
import importlib
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from tests import shuffle_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import shuffle_cases as cases  # noqa: E402

ENTRY_POINTS = ("sonar_shuffle_gather_f32", "sonar_shuffle_generate_f32")
SIG = (torch.tensor(10.0), torch.tensor(5.0))


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


def _item(nz, **kw):
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    args = dict(noise=chain, dims=(-1,), percentages=(1.0,), no_identity=False, fork_rng=False)
    return nz.ShuffledNoise(1.0, **(args | kw))


def test_exports_with_the_reference_parameter_names(nz):
    fn = nz.utils.elementwise_shuffle_by_dim
    params = inspect.signature(fn).parameters
    assert list(params) == ["t", "dim", "prob", "no_identity", "generator", "device_key"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in params.items() if name != "t")
    assert (params["dim"].default, params["prob"].default, params["no_identity"].default, params["generator"].default) == (-1, 1.0, False, None)
    assert issubclass(nz.ShuffledNoise, nz.CustomNoiseItemBase)
    item = _item(nz, dims=(1, -2), percentages=(0.5, 1.0), no_identity=True, fork_rng=True)
    clone = item.clone()
    assert clone.keys == {"noise", "dims", "percentages", "no_identity", "fork_rng"} and clone.noise is not item.noise
    assert (clone.dims, clone.percentages, clone.no_identity, clone.fork_rng, clone.factor) == ((1, -2), (0.5, 1.0), True, True, 1.0)


class _Inner:
    """A chain stand-in whose sampler is one known object."""

    def __init__(self):
        self.sampler = lambda s, sn: None

    def clone(self):
        return self

    def make_noise_sampler(self, *a, **k):
        return self.sampler


@pytest.mark.parametrize("kw", [dict(percentages=()), dict(dims=()), dict(percentages=(0.0, 0)), dict(dims=(), percentages=())])
def test_early_returns_hand_back_the_inner_sampler_itself(nz, kw):
    inner = _Inner()
    ns = _item(nz, noise=inner, **kw).make_noise_sampler(torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)
    assert ns is inner.sampler


@pytest.mark.parametrize("kw, text", [(dict(dims=(4,)), "Dimension out of range"), (dict(dims=(0, -5)), "Dimension out of range"),
                                      (dict(percentages=(1.5,)), "Percentage out of range"), (dict(percentages=(0.5, -0.1)), "Percentage out of range")])
def test_refusals(nz, kw, text):
    with pytest.raises(ValueError, match=text):
        _item(nz, **kw).make_noise_sampler(torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)


def test_the_registry_is_unchanged(reg):
    assert len(reg.NODE_CLASS_MAPPINGS) == 54 and len(reg.IMPLEMENTED_KEYS) == 42
    off = sorted(k for k, cls in reg.NODE_CLASS_MAPPINGS.items() if cls.__name__.startswith("OffPath_"))
    assert len(off) == 12 and not set(off) & set(reg.IMPLEMENTED_KEYS)
    assert "SonarShuffledNoise" not in reg.IMPLEMENTED_KEYS


def test_entry_points_are_declared_bound_and_exported(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64, "uint64_t": hl.C.c_uint64}
    lib = hl.load()
    for name in ENTRY_POINTS:
        decl = re.search(rf"\b(int|int64_t) {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [" ".join(p.split()) for p in decl.group(2).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert restype is kinds[decl.group(1)] and len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), (name, p)
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert int(re.search(r"#define SONAR_SHUFFLE_MAX_N (\d+)", text).group(1)) == hl.SHUFFLE_MAX_N >= 1024
    assert int(re.search(r"#define SONAR_SHUFFLE_DOMAIN 0x([0-9A-Fa-f]+)u", text).group(1), 16) == R.DOMAIN
    assert os.path.exists(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "shuffle.hip"))


def test_bad_arguments_come_back_as_error_codes_without_a_device(pkg):
    """The checks run before anything touches the HIP runtime: the pointers below are never dereferenced."""
    hl = pkg.hip_lib
    lib = hl.load()
    a, b, i = 4096, 8192, 12288
    gather, generate = lib.sonar_shuffle_gather_f32, lib.sonar_shuffle_generate_f32
    shape = (4, 2, 3, 5, 7, 1)  # ndim, s0 .. s4
    assert gather(None, b, *shape, 1, i, 0, None) == hl.ERR_ARG and gather(a, None, *shape, 1, i, 0, None) == hl.ERR_ARG
    assert gather(a, b, *shape, 1, None, 0, None) == hl.ERR_ARG
    assert gather(a, a, *shape, 1, i, 0, None) == hl.ERR_ARG and b"out must not be src" in lib.sonar_last_error()
    assert gather(a, b, *shape, 4, i, 0, None) == hl.ERR_ARG and gather(a, b, *shape, -1, i, 0, None) == hl.ERR_ARG
    assert gather(a, b, 0, 1, 1, 1, 1, 1, 0, i, 0, None) == hl.ERR_ARG and gather(a, b, 6, 1, 1, 1, 1, 1, 0, i, 0, None) == hl.ERR_ARG
    assert gather(a, b, 4, 2, 0, 5, 7, 1, 1, i, 0, None) == hl.ERR_ARG                    # n < 1
    assert gather(a, b, 4, 2, 1, 5, 7, 1, 1, i, 1, None) == hl.ERR_ARG                    # n < 2 with offsets
    assert gather(a, b, 4, 2, -3, 5, 7, 1, 0, i, 0, None) == hl.ERR_ARG
    assert gather(a, b, 3, 1 << 16, 2, (1 << 15) + 1, 1, 1, 1, i, 0, None) == hl.ERR_ARG  # more than 2^31 rows
    assert gather(a, b, 4, 2, 3, 0, 7, 1, 1, i, 0, None) == 0                             # rows == 0: nothing to launch
    key = (0.5, 0, 1, 2, 0, None)
    assert generate(None, b, *shape, 1, *key) == hl.ERR_ARG and generate(a, a, *shape, 1, *key) == hl.ERR_ARG
    assert generate(a, b, *shape, 4, *key) == hl.ERR_ARG and generate(a, b, 4, 2, 0, 5, 7, 1, 1, *key) == hl.ERR_ARG
    assert generate(a, b, 4, 2, 1, 5, 7, 1, 1, 0.5, 1, 1, 2, 0, None) == hl.ERR_ARG        # n < 2 with no_identity
    assert generate(a, b, *shape, 1, float("nan"), 0, 1, 2, 0, None) == hl.ERR_ARG
    assert generate(a, b, *shape, 1, 0.5, 0, 1, 2, -1, None) == hl.ERR_ARG and generate(a, b, *shape, 1, 0.5, 0, 1, 1 << 48, 0, None) == hl.ERR_ARG
    assert generate(a, b, 3, 1 << 16, 2, (1 << 15) + 1, 1, 1, 1, *key) == hl.ERR_ARG
    assert generate(a, b, 2, 3, hl.SHUFFLE_MAX_N + 1, 1, 1, 1, 1, *key) == hl.ERR_UNSUPPORTED
    assert b"at most 4096" in lib.sonar_last_error()
    assert generate(a, b, 4, 2, 3, 0, 7, 1, 1, *key) == 0


def test_a_launchable_call_on_a_cpu_tensor_raises_sonar_hip_error(nz):
    t = torch.arange(24.0).reshape(2, 3, 4)
    for kw in (dict(), dict(no_identity=True), dict(device_key=(1, 2)), dict(dim=0, prob=0.5)):
        with pytest.raises(nz.hip_lib.SonarHipError):
            nz.utils.elementwise_shuffle_by_dim(t, **kw)
    with pytest.raises(nz.hip_lib.SonarHipError):
        _item(nz).make_noise_sampler(torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)(*SIG)


def test_the_golden_file_and_the_case_table_agree():
    g = np.load(os.path.join(ROOT, "tests", "golden", "shuffle.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta_json"]))
    names = [c[0] for c in cases.replay_cases()]
    assert sorted(meta) == sorted(names) and len(names) == len(set(names)) == 102
    for name, shape, dim, prob, no_identity, rng in cases.replay_cases():
        x, out = g[f"in_{'x'.join(map(str, shape))}"], g[f"out_{name}"]
        assert np.array_equal(x.reshape(-1), np.arange(x.size, dtype=np.float32)) and out.shape == tuple(shape) and out.dtype == np.float32
        rows_in = np.moveaxis(x, dim, -1).reshape(-1, shape[dim])
        rows_out = np.moveaxis(out, dim, -1).reshape(-1, shape[dim])
        assert np.array_equal(np.sort(rows_out, axis=1), rows_in)            # a permutation of every row
        moved = (rows_out != rows_in).any(axis=1)
        if prob == 0.0:
            assert not moved.any()
        elif no_identity and prob == 1.0:
            assert moved.all()
        assert g[f"next_{name}"].shape == (4,)
    assert g["out_half"].dtype == np.float16 and g["item_out"].shape == (len(cases.ITEM["sigmas"]), *cases.ITEM["latent"])


# ------------------------------------------------------------------------------------------------ the generate-mode contract, restated
def test_block_layout_by_plain_integers():
    """The counter and key words, one block at a time, against ds.philox4x32_10 called with the words written out."""
    seed, stream, row = 0xFEDCBA9876543210, (0x1234 << 32) | 0x89ABCDEF, (0x0042 << 32) | 7
    got = R.blocks(seed, stream, row, 3)
    for b in range(3):
        want = ds.philox4x32_10(7, 0x0042 | (0x1234 << 16), b, 0x89ABCDEF, 0x76543210, 0xFEDCBA98 ^ 0x53484646)
        assert got[b] == [int(v) for v in want]
    assert R.blocks(seed, stream, row, 1)[0] != R.blocks(seed, stream, row + 1, 1)[0] != R.blocks(seed, stream + 1, row, 1)[0]
    assert R.blocks(-1, 0, 0, 1) == R.blocks(2**64 - 1, 0, 0, 1)  # a negative seed is its 64-bit pattern


def test_row_sources_are_the_contract():
    seed, stream, n = 99, 5, 37
    for row in (0, 1, 2**33 + 5):
        perm = R.row_sources(seed, stream, row, n, 1.0, False)
        words = [w for b in R.blocks(seed, stream + 2, row, 10) for w in b][:n]
        keys = [float(ds.u01(w)) for w in words]
        assert sorted(perm) == list(range(n))
        assert all((keys[perm[k]], perm[k]) < (keys[perm[k + 1]], perm[k + 1]) for k in range(n - 1))  # ascending by (key, index)
        rot = R.row_sources(seed, stream, row, n, 1.0, True)
        off = rot[0]
        assert 1 <= off < n and rot == [(j + off) % n for j in range(n)]
        assert off == 1 + int(float(ds.u01(R.blocks(seed, stream + 1, row, 1)[0][0])) * (n - 1))
    # the mask: u01 of its word against prob rounded to fp32; prob 0 never, prob 1 always (no draw)
    rows = range(200)
    u = [float(ds.u01(R.blocks(seed, stream, r, 1)[0][0])) for r in rows]
    for prob in (0.0, 0.3, 0.5, 1.0):
        moved = [R.row_sources(seed, stream, r, n, prob, True) != list(range(n)) for r in rows]
        assert moved == [prob >= 1.0 or u[r] < float(np.float32(prob)) for r in rows]
    assert 0.35 < sum(ui < 0.5 for ui in u) / 200 < 0.65
    assert R.row_sources(seed, stream, 0, 1, 1.0, False) == [0]
    # every offset of a short row is reached, none is 0
    assert {R.row_sources(seed, stream, r, 4, 1.0, True)[0] for r in range(100)} == {1, 2, 3}


def test_equal_keys_rank_by_index(monkeypatch):
    words = [[5 << 8, 3 << 8, (5 << 8) | 0xFF, 3 << 8], [1 << 8, 5 << 8, 0, 0]]  # keys 5 3 5 3 1 5: the low 8 bits do not count
    monkeypatch.setattr(R, "blocks", lambda seed, stream, row, count: words[:count])
    assert R.row_sources(0, 0, 0, 6, 1.0, False) == [4, 1, 3, 0, 2, 5]


def test_shuffled_rows_are_row_major_positions_of_the_other_dimensions():
    x = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    for dim in (0, 1, 2, -1):
        out = R.shuffled(x, dim, 1.0, False, 11, 3)
        d = dim % 3
        others = [s for k, s in enumerate(x.shape) if k != d]
        for r in range(x.size // x.shape[d]):
            pos = list(np.unravel_index(r, others))
            sel = tuple(pos[:d] + [slice(None)] + pos[d:])
            assert list(out[sel]) == [x[sel][j] for j in R.row_sources(11, 3, r, x.shape[d], 1.0, False)]
    # a shard of the batch is the slice of the whole: rows keep their global index
    whole = R.shuffled(x, 2, 0.5, False, 11, 3)
    assert np.array_equal(R.shuffled(x[1:], 2, 0.5, False, 11, 3, row_offset=3), whole[1:])
    assert not np.array_equal(R.shuffled(x, 2, 1.0, False, 11, 3), R.shuffled(x, 2, 1.0, False, 11, 6))  # another stream, another shuffle
