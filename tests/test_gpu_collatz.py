"""GPU: CollatzNoiseGenerator and AdvancedCollatzNoise (csrc/collatz.hip).

The chain stage is exact: every step is one correctly rounded fp32 operation, so the two kernels are held to the numpy restatement
(tests/collatz_refs.py) and to the reference's own outputs (tests/golden/collatz.npz, written by make_collatz_golden.py on the CPU) with
torch.equal, in replay mode -- and the host generator must stand where the reference's stands after the call.  Cases with quantile
normalisation (or adjust_scale) on go through the one inexact stage and take the tolerance tests/test_gpu_quantile.py applies to
quantile_normalize against the reference: rtol = 4e-6, atol = 4e-6 * max(1, peak); the iteration weights sum to 1 in magnitude, so the
accumulation does not widen it.  Generate mode is held to the restatement fed with the uniforms of the streams the call must have taken."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import collatz_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import collatz_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = cases.cases()
EXACT = [(n, p) for n, p in CASES if cases.is_exact(p)]
SIG = (torch.tensor(10.0), torch.tensor(5.0))
GENERATE = ("layout_dims_off5", "layout_flat_off0_rot", "layout_flat_values_rot", "mode_noise_x_ratios", "mode_noise_x_adds_flat_off0",
            "mode_seed_x_mults", "seed_force_odd", "unit_multipliers", "defaults")


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def ng(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise_generation")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "collatz.npz"), allow_pickle=False)


def golden_draws(g, name):
    flat, at = g[f"draws_{name}"], [0]

    def draw(_kind, shape):
        n = int(np.prod(shape))
        part = flat[at[0]:at[0] + n]
        at[0] += n
        return part.reshape(shape)

    return draw


def close(got, want):
    torch.testing.assert_close(got, want, rtol=4e-6, atol=4e-6 * max(1.0, float(want.abs().max())))


def generator(nz, params, *, cpu, latent=cases.LATENT, **kw):
    return nz.CollatzNoiseGenerator(torch.zeros(latent, device=DEV), cpu=cpu, normalized=False, **(params | kw))


# ------------------------------------------------------------------------------------------------ 1. the two kernels, launch by launch
@pytest.mark.parametrize("name, params", EXACT, ids=[n for n, _ in EXACT])
def test_kernels_equal_the_restatement_and_the_reference(pkg, g, name, params):
    hl = pkg.hip_lib
    p = R.DEFAULTS | params
    shape = cases.LATENT
    draw = golden_draws(g, name)
    dims = tuple(d % len(shape) for d in p["dims"])
    kept, second = R.OUTPUT_MODES[p["output_mode"]]
    keys = ("even_multiplier", "even_addition", "odd_multiplier", "odd_addition", "integer_math", "break_loops", "add_preserves_sign", "seed_mode")
    acc = torch.zeros(shape, device=DEV)
    want_acc = None
    for it in range(p["iterations"]):
        dim, chain_length = dims[it % len(dims)], p["chain_length"][it % len(p["chain_length"])]
        outer, length, inner, cl, n_chunks, len_p = R.view(shape, dim, p["flatten"], chain_length)
        assert hl.collatz_view(outer, length, inner, chain_length) == (cl, n_chunks, len_p)
        chunk_shape = (*shape[:dim], n_chunks) if p["flatten"] else (*shape[:dim], n_chunks, *shape[dim + 1:])
        seeds_h = np.ascontiguousarray(draw("seeds", chunk_shape)).reshape(outer, n_chunks, inner)
        seeds = torch.from_numpy(seeds_h).to(DEV)
        before = seeds.clone()
        ext = seeds.max().reshape(1)
        out1 = hl.collatz_chain(seeds, ext, outer, length, inner, chain_length, p["chain_offset"], span=p["rmax"] - p["rmin"] + 1, rmin=p["rmin"],
                                output=kept, **{k: p[k] for k in keys})
        want1 = R.chain(seeds_h, cl, **(p | dict(output=kept)))
        assert out1.shape == (outer * len_p * inner,) and torch.equal(seeds, before)
        assert torch.equal(out1.cpu(), torch.from_numpy(want1).flatten()), f"iteration {it}: dim {dim}, chain length {chain_length}"
        mix_h = np.ascontiguousarray(draw("mix", shape)) if second == "mix" else None
        other = seeds if second == "seeds" else torch.from_numpy(mix_h).to(DEV) if second == "mix" else None
        scale = (1.0 / p["iterations"]) * (-1 if p["iteration_sign_flipping"] and it & 1 else 1)
        assert hl.collatz_mix_(acc, out1, other, second, outer, length, inner, chain_length, scale) is acc
        want_acc = R.mix(np.zeros((outer, length, inner), np.float32) if want_acc is None else want_acc.reshape(outer, length, inner), want1,
                         seeds_h if second == "seeds" else mix_h, second, length, cl, scale)
        assert torch.equal(acc.cpu().flatten(), torch.from_numpy(want_acc).flatten()), f"iteration {it}: the accumulator"
    assert torch.equal(acc.cpu(), torch.from_numpy(g[f"out_{name}"]))


# ------------------------------------------------------------------------------------------------ 2. the generator, replay mode
@pytest.mark.parametrize("name, params", CASES, ids=[n for n, _ in CASES])
def test_replay_equals_the_reference(nz, g, name, params):
    gen = generator(nz, params, cpu=True)
    torch.manual_seed(cases.SEED)
    out = gen.generate(*SIG)
    after = torch.rand(4)
    want = torch.from_numpy(g[f"out_{name}"])
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == cases.LATENT
    if cases.is_exact(params):
        assert torch.equal(out.cpu(), want)
    else:
        close(out.cpu(), want)
    assert torch.equal(after, torch.from_numpy(g[f"next_{name}"])), "the host generator is not where the reference leaves it"


def test_item_replay_equals_the_reference_item(nz, g):
    it = cases.ITEM
    chains = []
    for _ in range(2):
        chain = nz.CustomNoiseChain()
        chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
        chains.append(chain)
    item = nz.AdvancedCollatzNoise(it["factor"], seed_custom_noise=chains[0], mix_custom_noise=chains[1], **it["params"]).clone()
    torch.manual_seed(it["global_seed"])
    ns = item.make_noise_sampler(torch.zeros(it["latent"], device=DEV), it["sigma_min"], it["sigma_max"], seed=it["seed"], cpu=True, normalized=True)
    want = torch.from_numpy(g["item_out"])
    for i, (s, sn) in enumerate(it["sigmas"]):
        got = ns(torch.tensor(s), torch.tensor(sn))
        assert got.is_cuda and tuple(got.shape) == tuple(want[i].shape)
        close(got.cpu(), want[i])
    assert torch.equal(torch.rand(4), torch.from_numpy(g["item_next"]))


# ------------------------------------------------------------------------------------------------ 3. generate mode: which stream each draw takes
def device_position():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset() // 4


@pytest.mark.parametrize("name", GENERATE)
def test_generate_equals_the_restatement_on_its_streams(pkg, nz, name):
    hl = pkg.hip_lib
    params = dict(CASES)[name]
    gen = generator(nz, params, cpu=False)
    torch.manual_seed(4321)
    seed, stream = device_position()
    host_state = torch.get_rng_state()
    out = gen.generate(*SIG)
    taken = [0]

    def draw(kind, shape):  # draw k of the call is stream + k: uniforms for the seeds, normals for the mix noise
        fn = hl.philox_uniform if kind == "seeds" else hl.philox_normal
        t = fn(tuple(shape), DEV, seed, stream + taken[0])
        taken[0] += 1
        return t.cpu().numpy()

    want = R.generate(cases.LATENT, params, draw)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    assert device_position() == (seed, stream + taken[0]) and torch.equal(torch.get_rng_state(), host_state)
    torch.manual_seed(4321)
    assert torch.equal(gen.generate(*SIG), out)          # the same seed, the same bits
    assert not torch.equal(gen.generate(*SIG), out)      # the next call draws on


def test_shard_rows_equal_the_rows_of_the_full_batch(nz, ng):
    params = dict(CASES)["mode_values"] | dict(dims=(-1, -2))
    for flatten in (False, True):
        p = params | dict(flatten=flatten)
        torch.manual_seed(99)
        whole = generator(nz, p, cpu=False).generate(*SIG)
        for first in (0, 1):
            torch.manual_seed(99)
            with ng.shard_offset(first):
                part = generator(nz, p, cpu=False, latent=(1, *cases.LATENT[1:])).generate(*SIG)
            assert torch.equal(part, whole[first:first + 1]), (flatten, first)


# ------------------------------------------------------------------------------------------------ 4. refusals, before any draw or launch
def test_generator_refusals_draw_and_launch_nothing(nz, ng):
    base = dict(CASES)["mode_values"]

    def refused(exc, text, *, shard=0, cpu=False, **kw):
        gen = generator(nz, base, cpu=cpu, **kw)
        torch.manual_seed(5)
        host, dev = torch.get_rng_state(), device_position()
        with ng.shard_offset(shard), pytest.raises(exc, match=text):
            gen.generate(*SIG)
        assert torch.equal(torch.get_rng_state(), host) and device_position() == dev

    for cpu in (False, True):
        refused(NotImplementedError, "float64", cpu=cpu, noise_dtype=torch.float64)
        refused(NotImplementedError, "float16", cpu=cpu, noise_dtype=torch.float16)
        refused(ValueError, "Dimension out of range", cpu=cpu, dims=(-1, 4))
        refused(ValueError, "Dimension out of range", cpu=cpu, dims=(-5,))
        refused(ValueError, "Bad output mode", cpu=cpu, output_mode="noise_x_values")
    refused(NotImplementedError, "across the samples of the batch", shard=1, quantile=0.5)
    refused(NotImplementedError, "across the samples of the batch", shard=1, dims=(-1, 0))
    refused(NotImplementedError, "across the samples of the batch", shard=2, dims=(-4,), flatten=True)
    # the same calls are fine on the first shard, and per-sample dims with the quantile off on any
    with ng.shard_offset(0):
        generator(nz, base, cpu=False, quantile=0.5, dims=(-1, 0)).generate(*SIG)
    with ng.shard_offset(3):
        generator(nz, base, cpu=False, dims=(-1, -2, 1)).generate(*SIG)


def test_kernel_refusals_leave_the_accumulator_untouched(pkg):
    hl = pkg.hip_lib
    lib = hl.load()
    outer, length, inner, chain_length, offset = 6, 6, 10, 4, 5     # cl 4, 2 chunks, len_p 8
    seeds = torch.rand(outer * 2 * inner, device=DEV)
    ext = seeds.max().reshape(1)
    out1 = torch.full((outer * 8 * inner,), -1.0, device=DEV)
    acc = torch.full((outer * length * inner,), -1.0, device=DEV)
    st = hl._stream()
    ps, pe, po, pa = seeds.data_ptr(), ext.data_ptr(), out1.data_ptr(), acc.data_ptr()
    tail = (16001.0, -8000.0, 0.5, 0.0, 3.0, 1.0, 7, 0, 0, st)
    chain, mix = lib.sonar_collatz_chain_f32, lib.sonar_collatz_mix_f32

    def refused(fn, *args):
        with pytest.raises(hl.SonarHipError):
            hl._check(fn(*args), "collatz")

    for bad in ((None, pe, po), (ps, None, po), (ps, pe, None), (ps, pe, ps)):            # a null pointer, out == seeds
        refused(chain, *bad, outer, length, inner, chain_length, offset, *tail)
    for view in ((-1, length, inner), (outer, -1, inner), (outer, length, -1), (1 << 16, 1 << 16, 1)):
        refused(chain, ps, pe, po, *view, 1, offset, *tail)                               # a negative size, more than 2^31 chains
        refused(mix, pa, po, ps, 1, *view, 1, 0.25, st)
    refused(chain, ps, pe, po, outer, length, inner, 0, offset, *tail)
    refused(chain, ps, pe, po, outer, length, inner, chain_length, -1, *tail)
    for bad in ((None, po, ps), (pa, None, ps), (pa, po, None), (pa, pa, ps), (pa, po, pa)):
        refused(mix, *bad, 1, outer, length, inner, chain_length, 0.25, st)
    refused(mix, pa, po, ps, 3, outer, length, inner, chain_length, 0.25, st)
    with pytest.raises(hl.SonarHipError):                                                 # the wrappers check the buffers against the view
        hl.collatz_chain(seeds[:-1], ext, outer, length, inner, chain_length, offset, span=16001.0, rmin=-8000.0, even_multiplier=0.5,
                         even_addition=0.0, odd_multiplier=3.0, odd_addition=1.0, integer_math=True, break_loops=True,
                         add_preserves_sign=True, seed_mode="default", output="ratios", out=out1)
    with pytest.raises(hl.SonarHipError):
        hl.collatz_mix_(acc, out1[:-1], seeds, "seeds", outer, length, inner, chain_length, 0.25)
    for empty in ((0, length, inner), (outer, 0, inner), (outer, length, 0)):             # an empty view launches nothing and succeeds
        assert chain(ps, pe, po, *empty, chain_length, offset, *tail) == 0 and mix(pa, po, ps, 1, *empty, chain_length, 0.25, st) == 0
    torch.cuda.synchronize()
    assert bool((acc == -1.0).all()) and bool((out1 == -1.0).all())
