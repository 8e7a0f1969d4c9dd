"""CPU: the host side of the row-keyed fill (``sonar_philox_rows_f32`` -> ``hip_lib.philox_rows`` -> ``CustomNoiseChain.make_row_seeded_sampler``
-> ``CustomNOISE.generate_noise`` with ``batch_index``) -- the declaration / binding / export, the refusals, which come back before anything
touches the HIP runtime, which chains qualify, and which calls keep the per-index loop."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sonar_philox_rows_f32"


@pytest.fixture(scope="module")
def mods(pkg):
    return (pkg.hip_lib, importlib.import_module("comfyui_sonar_amd.py.noise"), importlib.import_module("comfyui_sonar_amd.py.nodes.registry"))


def _header():
    return open(os.path.join(ROOT, "include", "sonar_hip.h")).read()


def test_entry_point_is_declared_bound_and_exported(mods):
    hl = mods[0]
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(rf"\bint {NAME}\s*\(([^)]*)\)\s*;", text)
    assert decl is not None, f"{NAME} is not declared in include/sonar_hip.h"
    kinds = {"float": C.c_float, "int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = hl.SIGNATURES[NAME]
    assert restype is C.c_int and len(params) == len(argtypes)
    for p, a in zip(params, argtypes):
        typ = p.rsplit(" ", 1)[0]
        assert a is (C.c_void_p if "*" in typ else kinds[typ]), p
    assert [p.rsplit(" ", 1)[1].lstrip("*") for p in params] == [
        "out", "rows", "inner", "row_seed", "row_stream", "uniform", "stream_id", "sub", "mul", "add", "factor", "normalized",
        "threshold_std_devs", "stream"]
    assert hasattr(hl.load(), NAME), f"{NAME} is not exported by the built library"
    for k, v in (("NONE", hl.ROWS_NORM_NONE), ("SCALE_NOISE", hl.ROWS_NORM_SCALE_NOISE), ("FUSED", hl.ROWS_NORM_FUSED)):
        assert int(re.search(rf"#define SONAR_ROWS_NORM_{k} (\d+)", _header()).group(1)) == v
    assert hl.load().sonar_philox_rows_max_inner() == hl.NPART * 4 * 4096
    assert "sonar_philox_rows_max_inner" in hl._HOST_QUERIES
    src = open(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "noise_rows.hip")).read()
    assert '#include "noise_stream.h"' in src and "philox4x32" not in src  # the generator is the shared one, not restated


def test_refusals_come_back_without_a_device(mods):
    """Every call below is refused by the argument checks or has no rows: the pointers are never dereferenced, nothing is launched."""
    hl = mods[0]
    fn = getattr(hl.load(), NAME)
    OK, ARG, UNSUPPORTED = (int(re.search(rf"#define SONAR_{k} \(?(-?\d+)", _header()).group(1)) for k in ("OK", "ERR_ARG", "ERR_UNSUPPORTED"))
    limit = hl.load().sonar_philox_rows_max_inner()

    def call(out=0x1000, rows=3, inner=256, seeds=0x2000, streams=None, uniform=0, normalized=1):
        return fn(out, rows, inner, seeds, streams, uniform, 5, 0.5, 3.46, 0.0, 1.0, normalized, 2.5, None)

    assert call(rows=0) == OK and call(rows=0, seeds=None, out=None) == OK  # no rows: success, nothing launched
    assert call(rows=-1) == UNSUPPORTED
    assert call(inner=0) == UNSUPPORTED and call(inner=-4) == UNSUPPORTED and call(rows=0, inner=0) == UNSUPPORTED
    assert call(inner=limit + 1) == UNSUPPORTED
    assert call(seeds=None) == UNSUPPORTED
    assert b"sonar_philox_rows_f32" in hl.load().sonar_last_error()
    assert call(out=None) == ARG and call(out=0x1002) == ARG
    assert call(normalized=3) == ARG and call(normalized=-1) == ARG


def test_wrapper_checks_its_arguments_before_the_device(mods):
    hl = mods[0]
    err = hl.SonarHipError
    with pytest.raises(err, match="rows dimension"):
        hl.philox_rows(False, (), "cuda", [], 0, 1.0, True)
    with pytest.raises(err, match="at least one element"):
        hl.philox_rows(False, (2, 0, 8), "cuda", [1, 2], 0, 1.0, True)
    with pytest.raises(err, match="at most"):
        hl.philox_rows(False, (1, hl.NPART * 4 * 4096 + 1), "cuda", [1], 0, 1.0, True)
    with pytest.raises(err, match="unknown normalisation"):
        hl.philox_rows(False, (2, 8), "cuda", [1, 2], 0, 1.0, 3)
    with pytest.raises(err, match="expected 2 values, got 3"):
        hl.philox_rows(False, (2, 8), "cuda", [1, 2, 3], 0, 1.0, True)
    with pytest.raises(err, match="int64 or uint64"):
        hl.philox_rows(False, (2, 8), "cuda", torch.zeros(2, dtype=torch.int32), 0, 1.0, True)
    with pytest.raises(err, match="lives on cpu"):
        hl.philox_rows(False, (2, 8), "cuda", torch.zeros(2, dtype=torch.int64), 0, 1.0, True)


def _chain(noise, *types, factor=1.0, **kwargs):
    return noise.CustomNoiseChain([noise.CustomNoiseItem(factor, noise_type=t, **kwargs) for t in types])


def test_only_exact_chains_get_a_row_sampler(mods):
    _, noise, _ = mods
    NT = noise.NoiseType
    x = torch.zeros(1, 4, 8, 8)
    seeds = [7, 8, 9]
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for t in (NT.GAUSSIAN, NT.UNIFORM):
            for normalized in (True, False):
                assert callable(_chain(noise, t).make_row_seeded_sampler(x.to(dtype), seeds, normalized=normalized))
    assert callable(_chain(noise, NT.GAUSSIAN, factor=0.5).make_row_seeded_sampler(x, seeds, normalized=False, multiplier=0.5))
    none = lambda chain, xx=x, **kw: chain.make_row_seeded_sampler(xx, seeds, **({"normalized": True} | kw)) is None  # noqa: E731
    assert none(_chain(noise, NT.GAUSSIAN, NT.GAUSSIAN))                       # two items
    assert none(noise.CustomNoiseChain([]))
    assert none(_chain(noise, NT.PERLIN)) and none(_chain(noise, NT.PYRAMID))  # other generators
    assert none(_chain(noise, NT.GAUSSIAN), cpu=True)                          # host draws: the generator's draw order is the contract
    wrapped = noise.CustomNoiseChain([noise.RepeatedNoise(1.0, noise=_chain(noise, NT.GAUSSIAN), repeat_length=2, max_recycle=4,
                                                          normalize=None, permute=False)])
    assert none(wrapped)                                                       # a wrapper item
    assert none(_chain(noise, NT.GAUSSIAN), x.double())                        # fp64
    assert none(_chain(noise, NT.UNIFORM, yaml_parameters="mul_fac: 2.0"))     # parameters that change the draw
    assert none(_chain(noise, NT.GAUSSIAN, normalize=True))                    # an item-level normalisation
    assert none(_chain(noise, NT.GAUSSIAN, factor=0.5))                        # normalised after scaling: another statistics sweep
    assert none(_chain(noise, NT.GAUSSIAN), positions=[0, 1])                  # one position per row
    assert none(_chain(noise, NT.GAUSSIAN), positions=[0, -1, 2])


@pytest.mark.parametrize("latent, cpu_noise", [({"batch_index": None}, False), ({}, False), ({"batch_index": [2, 0, 2]}, True)])
def test_other_calls_keep_the_loop(mods, monkeypatch, latent, cpu_noise):
    """No ``batch_index``: one whole-batch call; host draws: one call per index up to the largest, as before -- never the row sampler."""
    _, noise, reg = mods
    calls = []

    def sample(self, latent_image, seed):
        calls.append((tuple(latent_image.shape), seed))
        return torch.full(latent_image.shape, float(seed))

    def never(self, *a, **k):
        raise AssertionError("the row sampler was asked for")

    monkeypatch.setattr(reg.CustomNOISE, "_sample_noise", sample)
    monkeypatch.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", never)
    nobj = reg.CustomNOISE(_chain(noise, noise.NoiseType.GAUSSIAN), 40, cpu_noise=cpu_noise)
    out = nobj.generate_noise({"samples": torch.zeros(3, 4, 8, 8)} | latent)
    if latent.get("batch_index") is None:
        assert calls == [((3, 4, 8, 8), 40)]
    else:
        assert calls == [((1, 4, 8, 8), 40), ((1, 4, 8, 8), 41), ((1, 4, 8, 8), 42)]
        assert out[:, 0, 0, 0].tolist() == [42.0, 40.0, 42.0]


def test_registry_counts_are_unchanged(pkg):
    assert len(pkg.NODE_CLASS_MAPPINGS) == 54 and len(pkg.nodes.IMPLEMENTED_KEYS) == 42
