"""CPU: the host side of the row-keyed Perlin launch (``sonar_perlin_rows_f32`` -> ``hip_lib.perlin_rows`` ->
``CustomNoiseChain.make_row_seeded_sampler``) -- the declaration / binding / export, the refusals, which come back before anything touches
the HIP runtime, which Perlin chains get the row sampler, the keys and multipliers the sampler hands to the launch, and the host
statement of a row (tests/perlin_rows_refs.py) against the batch-1 call it restates."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc
from tests import perlin_rows_refs as refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sonar_perlin_rows_f32"


@pytest.fixture(scope="module")
def mods(pkg):
    return (pkg.hip_lib, importlib.import_module("comfyui_sonar_amd.py.noise"), importlib.import_module("comfyui_sonar_amd.py.noise_generation"))


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
        "out", "lattice", "rows", "C", "H", "W", "iters", "blend_mode", "div_fac", "row_seed", "row_stream", "stream_id", "factor", "normalized",
        "threshold_std_devs", "stream"]
    assert hasattr(hl.load(), NAME), f"{NAME} is not exported by the built library"
    assert hl.load().sonar_abi_version() == 1  # a new symbol, not a new ABI


def test_refusals_come_back_without_a_device(mods):
    """Every call below is refused by the argument checks or has no rows: the pointers are never dereferenced, nothing is launched."""
    hl = mods[0]
    fn = getattr(hl.load(), NAME)
    OK, ARG, UNSUPPORTED = (int(re.search(rf"#define SONAR_{k} \(?(-?\d+)", _header()).group(1)) for k in ("OK", "ERR_ARG", "ERR_UNSUPPORTED"))
    limit = hl.load().sonar_philox_rows_max_inner()

    def call(out=0x1000, lattice=0x2000, rows=3, c=1, h=16, w=16, iters=2, blend=0, seeds=0x3000, streams=None, normalized=2):
        return fn(out, lattice, rows, c, h, w, iters, blend, 2.0, seeds, streams, 5, 1.0, normalized, 2.5, None)

    assert call(rows=0) == OK and call(rows=0, seeds=None, out=None, lattice=None) == OK  # no rows: success, nothing launched
    assert call(rows=-1) == UNSUPPORTED
    assert call(seeds=None) == UNSUPPORTED                                              # rows without seeds
    assert b"sonar_perlin_rows_f32" in hl.load().sonar_last_error()
    assert call(c=1, h=1, w=limit + 1) == UNSUPPORTED and call(c=limit + 1, h=1, w=1) == UNSUPPORTED  # a row too long
    assert call(c=4, h=2048, w=2049) == UNSUPPORTED and call(c=2**40, h=2**19, w=2**19) == UNSUPPORTED
    assert call(h=2**20) == UNSUPPORTED and call(w=2**20) == UNSUPPORTED               # a plane too large
    assert call(c=0) == ARG and call(h=0) == ARG and call(w=-1) == ARG and call(rows=0, c=0) == ARG
    assert call(iters=-1) == ARG and call(iters=2**20) == ARG
    assert call(blend=3) == ARG and call(blend=-1) == ARG                               # a bad blend
    assert call(normalized=1) == ARG and call(normalized=3) == ARG and call(normalized=-1) == ARG  # scale_noise's form is no Perlin form
    assert call(out=None) == ARG and call(out=0x1002) == ARG
    assert call(lattice=None) == ARG and call(lattice=0x2004) == ARG and call(lattice=0x1000) == ARG


def test_wrapper_checks_its_arguments_before_the_device(mods):
    hl = mods[0]
    err = hl.SonarHipError
    kw = dict(iterations=2, div_fac=2.0, blend_mode="lerp", factor=1.0, normalized=True)
    with pytest.raises(err, match=r"\(rows, C, H, W\)"):
        hl.perlin_rows((2, 8), "cuda", [1, 2], 0, **kw)
    with pytest.raises(err, match="at least one element"):
        hl.perlin_rows((2, 1, 0, 8), "cuda", [1, 2], 0, **kw)
    with pytest.raises(err, match="at most"):
        hl.perlin_rows((1, 1, 1, hl.NPART * 4 * 4096 + 1), "cuda", [1], 0, **kw)
    with pytest.raises(err, match="unknown normalisation"):
        hl.perlin_rows((2, 1, 2, 2), "cuda", [1, 2], 0, **(kw | {"normalized": hl.ROWS_NORM_SCALE_NOISE}))
    with pytest.raises(err, match="unknown blend mode"):
        hl.perlin_rows((2, 1, 2, 2), "cuda", [1, 2], 0, **(kw | {"blend_mode": "slerp"}))
    with pytest.raises(err, match="expected 2 values, got 3"):
        hl.perlin_rows((2, 1, 2, 2), "cuda", [1, 2, 3], 0, **kw)
    with pytest.raises(err, match="int64 or uint64"):
        hl.perlin_rows((2, 1, 2, 2), "cuda", torch.zeros(2, dtype=torch.int32), 0, **kw)
    with pytest.raises(err, match="lives on cpu"):
        hl.perlin_rows((2, 1, 2, 2), "cuda", torch.zeros(2, dtype=torch.int64), 0, **kw)


def _chain(noise, *types, factor=1.0, **kwargs):
    return noise.CustomNoiseChain([noise.CustomNoiseItem(factor, noise_type=t, **kwargs) for t in types])


def test_which_perlin_chains_get_a_row_sampler(mods):
    """The latent only lends its shape, dtype and device: a meta tensor stands in for a device latent here (no GPU); a latent in host
    memory is one of the refused cases."""
    _, noise, ng = mods
    P = noise.NoiseType.PERLIN
    x, x5 = torch.zeros(1, 4, 8, 8, device="meta"), torch.zeros(1, 16, 2, 6, 6, device="meta")
    seeds = [7, 8, 9]
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for normalized in (True, False):
            assert callable(_chain(noise, P).make_row_seeded_sampler(x.to(dtype), seeds, normalized=normalized))
            assert callable(_chain(noise, P).make_row_seeded_sampler(x5.to(dtype), seeds, normalized=normalized, positions=[4, 0, 2]))
    for factor in (0.5, -1.0, 2.0):
        assert callable(_chain(noise, P, factor=factor).make_row_seeded_sampler(x, seeds, normalized=False, multiplier=0.5))
    none = lambda chain, xx=x, **kw: chain.make_row_seeded_sampler(xx, seeds, **({"normalized": True} | kw)) is None  # noqa: E731
    assert none(_chain(noise, P), cpu=True)                                     # host draws
    assert none(_chain(noise, P, P)) and none(_chain(noise, P, noise.NoiseType.GAUSSIAN))  # more than one item
    wrapped = noise.CustomNoiseChain([noise.RepeatedNoise(1.0, noise=_chain(noise, P), repeat_length=2, max_recycle=4, normalize=None,
                                                          permute=False)])
    assert none(wrapped)                                                        # not a plain CustomNoiseItem
    assert none(_chain(noise, P, yaml_parameters="div_fac: 3.0"))               # ns_kwargs
    assert none(_chain(noise, P, normalize=True)) and none(_chain(noise, P, normalize=False))  # an item-level normalisation
    assert none(_chain(noise, P, factor=0.5)) and none(_chain(noise, P, factor=-1.0))          # normalised, item factor other than 1
    with ng.shard_offset(2):
        assert none(_chain(noise, P)) and none(_chain(noise, P), normalized=False)              # a sharded batch
    assert not none(_chain(noise, P))
    assert none(_chain(noise, P), torch.zeros(1, 2**15, 2**8, 2**8, device="meta"))             # chw = 2^31
    limit = mods[0].load().sonar_philox_rows_max_inner()
    assert none(_chain(noise, P), torch.zeros(1, 1, 1, limit + 1, device="meta"))               # longer than the row kernel takes
    assert not none(_chain(noise, P), torch.zeros(1, 1, 1, limit, device="meta"))
    assert none(_chain(noise, P), torch.zeros(1, 4, 8, device="meta")) and none(_chain(noise, P), x.double())  # what the generator itself refuses
    assert none(_chain(noise, P), torch.zeros(1, 4, 8, 8)) and none(_chain(noise, P), torch.zeros(1, 4, 8, 8), normalized=False)  # a host latent
    assert none(_chain(noise, P), positions=[0, 1]) and none(_chain(noise, P), positions=[0, -1, 2])


class _FakeRNG:
    """DeviceRNG.take without a device: a position that moves by the count taken."""

    def __init__(self, seed, position):
        self.seed, self.position, self.takes = seed, position, []

    def take(self, count=1):
        at = self.position
        self.takes.append(int(count))
        self.position += int(count)
        return self.seed, at


@pytest.mark.parametrize("shape, out_shape", [((1, 4, 8, 8), (3, 4, 8, 8)), ((1, 16, 2, 6, 6), (3, 16, 2, 6, 6))], ids=["4d", "5d"])
@pytest.mark.parametrize("normalized, item_factor, multiplier, folded, later", [
    (True, 1.0, 1.0, 1.0, []), (True, 1.0, 0.5, 0.5, []),
    (False, 1.0, 1.0, 1.0, []), (False, 1.0, 0.5, 0.5, []), (False, 0.5, 0.3, 0.5, [0.5, 0.3]), (False, -1.0, 1.0, -1.0, []),
    (False, 2.0, 1.0, 2.0, [2.0]),
])
def test_keys_and_multipliers_handed_to_the_launch(mods, monkeypatch, shape, out_shape, normalized, item_factor, multiplier, folded, later):
    """Positions [5, 0, 3]: 2 * (5 + 1) stream ids in ONE take, row streams 2 p, the loop's position afterwards; the first multiplier other
    than 1 rides in the launch, each further one is a scale_noise_ over all rows; a 5-D latent is drawn as (rows, C * F, H, W)."""
    hl, noise, _ = mods
    rng = _FakeRNG(seed=1234, position=40)
    calls, scaled = [], []

    def perlin_rows(shp, device, row_seeds, stream_id, **kw):
        calls.append((tuple(shp), list(row_seeds), stream_id, kw))
        return torch.zeros(tuple(shp))

    monkeypatch.setattr(noise.DeviceRNG, "take", rng.take)
    monkeypatch.setattr(hl, "perlin_rows", perlin_rows)
    monkeypatch.setattr(hl, "scale_noise_", lambda t, f, normalized, partials: scaled.append((f, normalized, partials)) or t)
    sampler = _chain(noise, noise.NoiseType.PERLIN, factor=item_factor).make_row_seeded_sampler(
        torch.zeros(shape, device="meta"), [1234 + p for p in (5, 0, 3)], normalized=normalized, positions=[5, 0, 3], multiplier=multiplier)
    assert rng.takes == []  # nothing is taken before the call
    out = sampler(None, None)
    assert rng.takes == [12] and rng.position == 52  # where the loop's six samplers, two ids each, leave the generator
    assert len(calls) == 1
    shp, seeds, stream_id, kw = calls[0]
    c = shape[1] * (shape[2] if len(shape) == 5 else 1)
    assert shp == (3, c, *shape[-2:]) and tuple(out.shape) == out_shape
    assert seeds == [1234] * 3 and stream_id == 40 and list(kw["row_streams"]) == [10, 0, 6]
    defaults = mods[2].PerlinOldNoiseGenerator.ng_params()
    assert (kw["iterations"], kw["div_fac"], kw["blend_mode"]) == (defaults["iterations"], defaults["div_fac"], defaults["blend_mode"]) == (2, 2.0, "lerp")
    assert kw["normalized"] is bool(normalized) and kw["factor"] == folded
    assert scaled == [(m, False, None) for m in later]


@pytest.mark.parametrize("shape, iterations, div_fac, blend", [((3, 5, 7), 2, 2.0, "lerp"), ((1, 16, 16), 5, -1.7, "inject"), ((2, 8, 8), 0, 1.5, "subtract_b")])
def test_a_row_of_the_refs_is_the_batch_of_one_call(shape, iterations, div_fac, blend):
    """refs.row: the lattice on stream + 1, the values on stream, ONE latent, element offset 0 -- what ds.perlin_values gives for a batch-1
    call over ds.perlin_lattice -- then the oracle's scale_noise."""
    seed, stream = 2**63 + 11, 2**32 + 6
    chw = math.prod(shape)
    lattice = ds.perlin_lattice(seed, stream + 1, iterations, *shape, blend)
    assert np.array_equal(refs.row_lattice(seed, stream, shape, iterations, blend), lattice) and (iterations > 0 or not lattice.any())
    want, _ = ds.perlin_values(seed, stream, lattice.reshape(1, chw), chw, div_fac, chw, 0)
    assert np.array_equal(refs.row_raw(seed, stream, shape, iterations, div_fac, blend), want)
    assert not np.array_equal(want, ds.perlin_values(seed, stream + 2, lattice.reshape(1, chw), chw, div_fac, chw, 0)[0])
    kw = dict(iterations=iterations, div_fac=div_fac, blend_mode=blend)
    assert np.array_equal(refs.row(seed, stream, shape, factor=1.0, normalized=refs.NONE, **kw), want)
    assert np.array_equal(refs.row(seed, stream, shape, factor=0.5, normalized=refs.NONE, **kw), want * 0.5)
    seen = {}
    got = refs.row(seed, stream, shape, factor=0.7, normalized=refs.FUSED, decisions=seen, **kw)
    assert np.array_equal(got, orc.scale_noise(torch.from_numpy(want.copy()), 0.7, normalized=True).numpy())
    assert seen["sub"]  # a Perlin row's mean is 0.5 / div_fac: far from zero
    # the wrapped stream id: the lattice of stream 2^64 - 1 is drawn on stream 0
    assert np.array_equal(refs.row_lattice(seed, 2**64 - 1, shape, max(iterations, 1), blend), ds.perlin_lattice(seed, 0, max(iterations, 1), *shape, blend))
