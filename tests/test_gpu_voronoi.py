"""GPU: VoronoiNoiseGenerator and AdvancedVoronoiNoise (csrc/voronoi.hip).

The kernel is held to the fp64 statement of tests/voronoi_refs.py on the golden cases' own draws: per call, over the elements the statement
does not flag as ambiguous, |kernel - fp64 statement| <= 8 x |fp32 statement - fp64 statement| (floor 1e-6 of the output range), and the
flagged share stays under the cases' caps (1e-3; 1e-2 for the direction-sensitive distances and cellid).  The same bound holds against the
reference's own outputs (tests/golden/voronoi.npz), and the host generator and the z position must stand where the reference leaves them.
Generate mode is replay mode fed with the uniforms of the streams the call must have taken, bit for bit."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import voronoi_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import voronoi_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = cases.cases()
IDS = [n for n, _l, _p in CASES]
BY_NAME = {n: (l, p) for n, l, p in CASES}
SIG = (torch.tensor(10.0), torch.tensor(5.0))
GUARD = 64
KERNEL = ("d_euclidean", "d_minkowski", "d_angle_tanh", "d_nested", "r_sum_rscale", "r_cellid", "n1_clamps", "n5_small", "n257_small", "n257")
GENERATE = ("d_sum_dscale", "d_fuzz", "d_fuzz_sum", "preset_fuzz", "r_cellid", "r_fuzz", "r_fuzz_sum", "r_gradient_two", "oct3_lac2_new", "oct3_same_roll_chan_up", "z_max0_range", "z_reset", "n257_small", "preset_mix")


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def ng(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise_generation")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "voronoi.npz"), allow_pickle=False)


def golden_draws(g, name):
    flat, at = g[f"draws_{name}"], [0]

    def draw(shape):
        n = int(np.prod(shape))
        part = flat[at[0]:at[0] + n]
        at[0] += n
        return part.reshape(shape)

    return draw


_statements = {}


def statements(g, name):
    """Per call of the case: (fp64 statement, ambiguous, fp32 statement's error); computed once."""
    if name not in _statements:
        latent, params = BY_NAME[name]
        g64, g32 = (R.Generator(latent, params, golden_draws(g, name), t) for t in (np.float64, np.float32))
        calls = []
        for _ in range(cases.CALLS):
            want, amb = g64.generate()
            calls.append((want, amb, R.error(g32.generate()[0], want, amb)))
        _statements[name] = calls
    return _statements[name]


def generator(nz, name, *, cpu, latent=None, **kw):
    lat, params = BY_NAME[name]
    return nz.VoronoiNoiseGenerator(torch.zeros(latent or lat, device=DEV), cpu=cpu, normalized=False, **(params | kw))


def device_position():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset() // 4


# ------------------------------------------------------------------------------------------------ 1. one launch against the statement
@pytest.mark.parametrize("name", KERNEL)
def test_the_kernel_against_the_fp64_statement_with_guard_floats(pkg, nz, g, name):
    """The first call of a one-octave case as a single launch into the middle of a larger buffer: 5 x 7 is a ragged tile, 257 points one
    past the staging chunk; the floats around the output keep their value."""
    hl = pkg.hip_lib
    latent, params = BY_NAME[name]
    p = R.DEFAULTS | params
    assert p["octaves"] == 1
    want, amb, err32 = statements(g, name)[0]
    n = max(2, p["n_points"][0])
    fp = torch.from_numpy(np.ascontiguousarray(golden_draws(g, name)((latent[0], latent[1], n, 3)))).to(DEV)
    before = fp.clone()
    numel = int(np.prod(latent))
    buf = torch.full((numel + 2 * GUARD,), -7.0, device=DEV)
    out = buf[GUARD:GUARD + numel].view(latent)
    out.zero_()
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes(p["distance_mode"][0], p["result_mode"][0])
    prog = hl.voronoi_program(dterms, rterms)
    z_range = max(latent[2], latent[3])
    z_norm = (p["z_initial"] % z_range) / z_range
    aux = None
    if rterms[0]["op"] == "cellid":
        raw = hl.voronoi_program(dterms, [{"op": "cellid_raw"}])
        ids = hl.voronoi_octave_(torch.zeros(latent, device=DEV), fp, raw, scale=1.0, z_norm=z_norm, amplitude=1.0)
        assert float(ids.max()) <= n - 1 and torch.equal(ids, ids.round())
        aux = torch.ones(hl.VORONOI_MAX_TERMS, device=DEV)
        aux[0] = ids.max()
    assert hl.voronoi_octave_(out, fp, prog, scale=1.0, z_norm=z_norm, amplitude=1.0, final_div=1.0, aux=aux) is out
    got = out.cpu().numpy()
    err = R.error(got, want, amb)
    print(f"{name}: kernel {err:.3e}  fp32 statement {err32:.3e}  bound {R.bound(err32, want):.3e}  ambiguous {amb.mean():.2e}")
    assert amb.mean() <= (1e-2 if name in cases.WIDE else 1e-3)
    assert err <= R.bound(err32, want)
    assert torch.equal(fp, before) and bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + numel:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ 2. the generator, replay mode
@pytest.mark.parametrize("name", IDS)
def test_replay_lies_within_the_bound_of_the_statement_and_of_the_reference(nz, g, name):
    torch.manual_seed(cases.SEED)
    gen = generator(nz, name, cpu=True)
    latent = BY_NAME[name][0]
    for i, (want, amb, err32) in enumerate(statements(g, name)):
        out = gen.generate(*SIG)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == latent
        got = out.cpu().numpy()
        err, err_ref, limit = R.error(got, want, amb), R.error(got, g[f"out_{name}"][i], amb), R.bound(err32, want)
        print(f"{name} call {i}: kernel {err:.3e}  to the reference {err_ref:.3e}  fp32 statement {err32:.3e}  bound {limit:.3e}  ambiguous {amb.mean():.2e}")
        assert amb.mean() <= (1e-2 if name in cases.WIDE else 1e-3)
        assert err <= limit and err_ref <= limit, f"call {i}"
    assert torch.equal(torch.rand(4), torch.from_numpy(g[f"next_{name}"])), "the host generator is not where the reference leaves it"
    assert np.array_equal(g[f"z_{name}"], np.array([gen.z_curr, gen.z_increment]))


def test_item_replay_equals_the_reference_item(nz, g):
    """The feature points come from a Gaussian chain through normalize_to_scale, whose three roundings per value (2^-24 relative each) move
    every distance by up to ~2e-7; diff2 divides by v1 + v2, at 33 points rarely below 0.05 (4e-6), and the normalisation by the standard
    deviation of diff2 (~0.25) scales that to ~2e-5 of a unit-variance output: atol 2e-5 x max(1, peak)."""
    it = cases.ITEM
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.AdvancedVoronoiNoise(it["factor"], custom_noise=chain, **it["params"]).clone()
    torch.manual_seed(it["global_seed"])
    ns = item.make_noise_sampler(torch.zeros(it["latent"], device=DEV), it["sigma_min"], it["sigma_max"], seed=it["seed"], cpu=True, normalized=True)
    want = torch.from_numpy(g["item_out"])
    for i, (s, sn) in enumerate(it["sigmas"]):
        got = ns(torch.tensor(s), torch.tensor(sn))
        assert got.is_cuda and tuple(got.shape) == tuple(want[i].shape)
        torch.testing.assert_close(got.cpu(), want[i], rtol=0, atol=2e-5 * max(1.0, float(want[i].abs().max())))
    assert torch.equal(torch.rand(4), torch.from_numpy(g["item_next"]))


# ------------------------------------------------------------------------------------------------ 3. generate mode: which stream each draw takes
@pytest.mark.parametrize("name", GENERATE)
def test_generate_is_replay_on_the_uniforms_of_its_streams(pkg, nz, name):
    hl = pkg.hip_lib
    gen = generator(nz, name, cpu=False)
    torch.manual_seed(4321)
    seed, stream = device_position()
    host_state = torch.get_rng_state()
    outs = [gen.generate(*SIG) for _ in range(cases.CALLS)]
    taken = [0]
    twin = generator(nz, name, cpu=True)

    def rand_like(*, fun, shape, **_kw):  # draw k of the generator is stream + k
        assert fun is torch.rand
        t = hl.philox_uniform(tuple(shape), DEV, seed, stream + taken[0])
        taken[0] += 1
        return t

    twin.rand_like = rand_like
    for i in range(cases.CALLS):
        assert torch.equal(twin.generate(*SIG), outs[i]), f"call {i}"
    assert taken[0] >= 1 and device_position() == (seed, stream + taken[0]) and torch.equal(torch.get_rng_state(), host_state)
    after = hl.philox_uniform((4,), DEV, *nz.DeviceRNG.take())  # the next draw: the stream behind the call's, whatever the call did
    assert torch.equal(after, hl.philox_uniform((4,), DEV, seed, stream + taken[0]))
    torch.manual_seed(4321)
    assert torch.equal(generator(nz, name, cpu=False).generate(*SIG), outs[0])  # the same seed, the same bits


def test_shard_rows_equal_the_rows_of_the_full_batch(nz, ng):
    """Expressions without cellid are per-(b, c) functions of the features, and the features are keyed by global batch index."""
    for name in ("oct3_lac2_new", "d_sum_dscale", "r_softmin"):
        latent = BY_NAME[name][0]
        torch.manual_seed(99)
        whole = generator(nz, name, cpu=False).generate(*SIG)
        for first in (0, 1):
            torch.manual_seed(99)
            with ng.shard_offset(first):
                part = generator(nz, name, cpu=False, latent=(1, *latent[1:])).generate(*SIG)
            assert torch.equal(part, whole[first:first + 1]), (name, first)


# ------------------------------------------------------------------------------------------------ 4. refusals, before any draw or launch
def test_generator_refusals_draw_and_launch_nothing(nz):
    def refused(exc, text, **kw):
        for cpu in (False, True):
            gen = generator(nz, "d_euclidean", cpu=cpu, **kw)
            torch.manual_seed(5)
            host, dev = torch.get_rng_state(), device_position()
            with pytest.raises(exc, match=text):
                gen.generate(*SIG)
            assert torch.equal(torch.get_rng_state(), host) and device_position() == dev and gen.feature_points is None

    refused(NotImplementedError, "at most one fuzz term", distance_mode=("fuzz:name=angle_tanh:fuzz=0.1+fuzz",))
    refused(NotImplementedError, "outermost", distance_mode=("weight:name=fuzz",))
    refused(NotImplementedError, "median_distance", result_mode=("f1", "median_distance"), octaves=2)
    refused(NotImplementedError, "use_sorted", result_mode=("softmin:use_sorted=1",))
    refused(NotImplementedError, "idx outside 0..3", result_mode=("f:idx=4",))
    refused(NotImplementedError, "pad_mode=replicate only", result_mode=("gradient_magnitude:pad_mode=reflect",))
    refused(NotImplementedError, "outermost", result_mode=("ridge:name=fuzz",))
    refused(NotImplementedError, "beside a bare f term", result_mode=("f1+fuzz",))
    refused(ValueError, "Bad Voronoi distance mode manhattan", distance_mode=("manhattan",))
    refused(IndexError, "out of bounds", n_points=(3,), result_mode=("f4",))
    refused(IndexError, "out of bounds", n_points=(33, 3), result_mode=("f1", "f4"), octaves=2, octave_mode="new_features")
    # an index is held to the feature set its own octave reads: f4 on 33 points, f1 on 2
    out = generator(nz, "d_euclidean", cpu=True, n_points=(33, 2), result_mode=("f4", "f1"), octaves=2, octave_mode="new_features").generate(*SIG)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(ValueError, match="at most 4 dimension"):
        nz.VoronoiNoiseGenerator(torch.zeros(1, 2, 3, 4, 5, device=DEV))
    with pytest.raises(nz.hip_lib.SonarHipError, match="float32"):
        nz.VoronoiNoiseGenerator(torch.zeros(1, 2, 4, 4, device=DEV, dtype=torch.float16))


def test_the_plane_kernels_one_by_one_with_guard_floats(pkg):
    """gradient (replicate padding, two planes), the fuzz add and the accumulation against the same operations in fp32 on the host (each
    step one correctly rounded operation: equal bits), on 3 x 5 x 7 in the middle of a larger buffer."""
    hl = pkg.hip_lib
    shape, numel = (1, 3, 5, 7), 105
    gen = torch.Generator().manual_seed(3)
    r1, r2, u, x = (torch.rand(shape, generator=gen) for _ in range(4))
    buf = torch.full((numel + 2 * GUARD,), -7.0, device=DEV)
    acc = buf[GUARD:GUARD + numel].view(shape)
    acc.copy_(x)
    f = np.float32  # numpy's fp32 operations are correctly rounded, sqrt included (torch's vectorised CPU sqrt is not everywhere)
    n1, n2, nu, want = r1.numpy(), r2.numpy(), u.numpy(), x.numpy().copy()
    p1, p2 = (np.pad(r, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge") for r in (n1, n2))
    dx, dy = p1[..., 1:-1, 2:] - p2[..., 1:-1, :-2], p1[..., 2:, 1:-1] - p2[..., :-2, 1:-1]
    want = want + np.sqrt(dx * dx + dy * dy) * f(0.3)
    assert hl.voronoi_gradient_(acc, r1.to(DEV), r2.to(DEV), 0.3) is acc and np.array_equal(acc.cpu().numpy(), want)
    want = want + (nu * f(0.2 * 2) - f(0.2))
    hl.voronoi_fuzz_add_(acc, u.to(DEV), 0.2)
    assert np.array_equal(acc.cpu().numpy(), want)
    want = (want + n1 * f(0.75)) / f(1.75)
    hl.voronoi_acc_(acc, r1.to(DEV), 0.75, final_div=1.75)
    assert want.dtype == np.float32 and np.array_equal(acc.cpu().numpy(), want)
    want = torch.from_numpy(want)
    assert bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + numel:] == -7.0).all())
    for call in (lambda: hl.voronoi_gradient_(acc, r1.to(DEV)[:, :2], r2.to(DEV), 1.0), lambda: hl.voronoi_fuzz_add_(acc, u.to(DEV)[:, :2], 0.1),
                 lambda: hl.voronoi_acc_(acc, r1.to(DEV)[:, :2], 1.0)):
        with pytest.raises(hl.SonarHipError):
            call()
    assert torch.equal(acc.cpu(), want)


def test_the_fuzz_passes_write_their_statistics_and_nothing_else(pkg, nz):
    """The three launches one by one on 1 x 2 x 5 x 7 with 5 points, uniforms read by index: pass 0 leaves the inner distance's extremes, pass
    1 the fuzzed distance's per row, both as ordered integers and equal to the same reductions of the same fp32 values on the host; the
    words around the statistics, the uniforms and the feature points keep their value, and only pass 2 writes the output."""
    hl = pkg.hip_lib
    shape, n = (1, 2, 5, 7), 5
    gen = torch.Generator().manual_seed(11)
    fp, u = torch.rand(1, 2, n, 3, generator=gen).to(DEV), torch.rand(*shape, n, generator=gen).to(DEV)
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes("fuzz:fuzz=0.1", "f2")
    prog = hl.voronoi_program(dterms, rterms)
    rows = 10
    fz = hl.VoronoiFuzz(0, 0.1, rows, DEV, u=u)
    buf = torch.full((2 + 2 * rows + 2 * GUARD,), 12345, dtype=torch.int32, device=DEV)
    stats = buf[GUARD:GUARD + 2 + 2 * rows]
    stats.copy_(fz.stats)
    fz.stats = stats
    out = torch.full(shape, -3.0, device=DEV)
    kept = (fp.clone(), u.clone())

    def decode(words):
        w = words.cpu().numpy().view(np.uint32)
        return np.where(w & 0x80000000, w ^ 0x80000000, ~w).astype(np.uint32).view(np.float32)

    # the inner (euclidean) distances [1, 2, 5, 7, 5] in numpy fp32, as tests/voronoi_refs.py states them
    octv = R.Octave(np.float32, None)
    T = np.float32
    grid = np.empty((5, 7, 3), T)
    grid[..., 0], grid[..., 1], grid[..., 2] = (np.arange(5, dtype=T) / T(5))[:, None], (np.arange(7, dtype=T) / T(7))[None, :], T(0.25)
    d = R.rem1(R.rem1(grid)[None, None, :, :, None, :] - R.rem1(fp.cpu().numpy())[:, :, None, None, :, :] + T(0.5)) - T(0.5)
    inner = octv.d_euclidean(d)
    hl.voronoi_octave_(None, fp, prog, scale=1.0, z_norm=0.25, fuzz=fz, fuzz_pass=0, shape=shape)
    got = decode(stats)
    assert got[0] == inner.min() and got[1] == inner.max() and bool((stats[2::2] == -1).all()) and bool((stats[3::2] == 0).all())
    spread = max(abs(float(inner.min())), abs(float(inner.max()))) * 0.1
    fuzzed = inner + (u.cpu().numpy() * T(spread * 2) - T(spread))
    hl.voronoi_octave_(None, fp, prog, scale=1.0, z_norm=0.25, fuzz=fz, fuzz_pass=1, shape=shape)
    got = decode(stats)
    assert np.array_equal(got[2::2], fuzzed.min(axis=(-2, -1)).reshape(-1)) and np.array_equal(got[3::2], fuzzed.max(axis=(-2, -1)).reshape(-1))
    assert bool((out == -3.0).all())
    out.zero_()
    hl.voronoi_octave_(out, fp, prog, scale=1.0, z_norm=0.25, fuzz=fz, fuzz_pass=2)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= float(inner.min()) and float(out.max()) <= float(inner.max())
    assert bool((buf[:GUARD] == 12345).all()) and bool((buf[GUARD + 2 + 2 * rows:] == 12345).all())
    assert torch.equal(fp, kept[0]) and torch.equal(u, kept[1])
    with pytest.raises(hl.SonarHipError):   # statistics sized for another shape
        hl.voronoi_octave_(out, fp, prog, scale=1.0, z_norm=0.25, fuzz=hl.VoronoiFuzz(0, 0.1, rows + 1, DEV, u=u))
    with pytest.raises(hl.SonarHipError):
        hl.voronoi_octave_(None, fp, prog, scale=1.0, z_norm=0.25, fuzz=fz, fuzz_pass=2, shape=shape)


def test_kernel_refusals_leave_the_output_untouched(pkg, nz):
    hl = pkg.hip_lib
    fn = hl.load().sonar_voronoi_octave_f32
    fp = torch.rand(2, 3, 33, 3, device=DEV)
    out = torch.full((2, 3, 8, 12), -1.0, device=DEV)
    prog = hl.voronoi_program(*nz.VoronoiNoiseGenerator.parse_modes("euclidean", "diff2"))
    cell = hl.voronoi_program(*nz.VoronoiNoiseGenerator.parse_modes("euclidean", "cellid"))
    st, pf, po = hl._stream(), fp.data_ptr(), out.data_ptr()

    def code(fp_=pf, out_=po, aux=None, shape=(2, 3, 8, 12), n=33, flags=0, program=prog):
        return fn(fp_, out_, aux, *shape, n, 1.0, 0.25, 1.0, 1.0, flags, hl.C.addressof(program), st)

    assert code(fp_=None) == hl.ERR_ARG and code(out_=None) == hl.ERR_ARG and code(out_=pf) == hl.ERR_ARG and code(aux=po) == hl.ERR_ARG
    assert code(shape=(2, 3, 8, -12)) == hl.ERR_ARG and code(shape=(1 << 10, 1 << 10, 1 << 10, 2)) == hl.ERR_ARG
    assert code(n=1) == hl.ERR_ARG and code(n=hl.VORONOI_MAX_POINTS + 1) == hl.ERR_UNSUPPORTED and code(flags=4) == hl.ERR_ARG
    assert code(program=cell) == hl.ERR_ARG
    bad = hl.voronoi_program(*nz.VoronoiNoiseGenerator.parse_modes("euclidean", "diff2"))
    bad.r[0].op = 9
    assert code(program=bad) == hl.ERR_ARG
    for empty in ((0, 3, 8, 12), (2, 3, 0, 12)):
        assert code(shape=empty) == 0
    with pytest.raises(hl.SonarHipError):   # the wrapper checks the tensors against each other
        hl.voronoi_octave_(out, fp[:1], prog, scale=1.0, z_norm=0.0, amplitude=1.0)
    with pytest.raises(hl.SonarHipError):
        hl.voronoi_octave_(out, fp, cell, scale=1.0, z_norm=0.0, amplitude=1.0, aux=torch.ones(2, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
