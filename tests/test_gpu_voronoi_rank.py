"""GPU: the rank route of VoronoiNoiseGenerator (csrc/voronoi.hip: voronoi_rank_kernel, sonar_voronoi_rank_octave_f32).

The kernel is held to the fp64 statement of tests/voronoi_rank_refs.py on the golden cases' own draws, by the rule of
tests/test_gpu_voronoi.py: per call, over the elements the statement does not flag as ambiguous, |kernel - fp64 statement| <= 8 x |fp32
statement - fp64 statement| (floor 1e-6 of the output range, tests/voronoi_refs.bound), the same bound against the reference's own outputs
(tests/golden/voronoi_rank.npz), and the host generator and the z position where the reference leaves them.  Generate mode is replay mode
fed with the uniforms of the streams the call must have taken, bit for bit.  A program whose ranks lie in 0..3 has the top-four kernel's
bits on this route."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import voronoi_rank_refs as RR
from tests import voronoi_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import voronoi_rank_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = cases.cases()
IDS = [n for n, _l, _p in CASES]
BY_NAME = {n: (l, p) for n, l, p in CASES}
SIG = (torch.tensor(10.0), torch.tensor(5.0))
GUARD = 64
CAP = 1e-3
GENERATE = ("median_n257", "f_idx_last", "softsorted_n33", "gradient_median", "fuzz_f5", "sum_rscale", "oct2_new", "d_fuzz_median")


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "voronoi_rank.npz"), allow_pickle=False)


def statements(g, name, variant=None):
    """Per call: (fp64 statement, ambiguous, the fp32 statement's error); the statements are computed once and shared."""
    latent, params = BY_NAME[name]
    return [(want, amb, R.error(got32, want, amb)) for want, amb, got32 in RR.statements(g, name, latent, params, cases.CALLS, variant)[0]]


def generator(nz, name, *, cpu, **kw):
    latent, params = BY_NAME[name]
    gen = nz.VoronoiNoiseGenerator(torch.zeros(latent, device=DEV), cpu=cpu, normalized=False, **(params | kw))
    gen.rank_route = True
    return gen


def device_position():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset() // 4


def one_launch(pkg, nz, g, name, *, rmode=None):
    """The first call of a one-octave case as a single launch of the rank kernel into the middle of a larger buffer."""
    hl = pkg.hip_lib
    latent, params = BY_NAME[name]
    p = R.DEFAULTS | params
    assert p["octaves"] == 1
    n = max(2, p["n_points"][0])
    fp = torch.from_numpy(np.ascontiguousarray(RR.golden_draws(g, name)((latent[0], latent[1], n, 3)))).to(DEV)
    before = fp.clone()
    numel = int(np.prod(latent))
    buf = torch.full((numel + 2 * GUARD,), -7.0, device=DEV)
    out = buf[GUARD:GUARD + numel].view(latent)
    out.zero_()
    gen = nz.VoronoiNoiseGenerator
    rmode = p["result_mode"][0] if rmode is None else rmode
    dterms, rterms = gen.parse_modes(p["distance_mode"][0], rmode, rank=True)
    prog = hl.voronoi_program(dterms, gen._resolve(rterms, n, rmode))
    z_range = max(latent[2], latent[3])
    z_norm = (p["z_initial"] % z_range) / z_range
    assert hl.voronoi_rank_octave_(out, fp, prog, scale=1.0, z_norm=z_norm, amplitude=1.0, final_div=1.0) is out
    got = out.cpu().numpy()
    assert torch.equal(fp, before) and bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + numel:] == -7.0).all())
    return got


# ------------------------------------------------------------------------------------------------ 1. one launch against the statement
@pytest.mark.parametrize("name", cases.KERNEL)
def test_the_kernel_against_the_fp64_statement_with_guard_floats(pkg, nz, g, name):
    """5 x 7 is a ragged tile (and less than one wave of the row instantiation's workgroup), 2 x 3 x 8 x 12 two workgroups of it per plane;
    257 points one past the staging chunk, 256 the longest row; the floats around the output keep their value."""
    want, amb, err32 = statements(g, name)[0]
    got = one_launch(pkg, nz, g, name)
    err, err_ref = R.error(got, want, amb), R.error(got, g[f"out_{name}"][0], amb)
    print(f"{name}: kernel {err:.3e}  to the reference {err_ref:.3e}  fp32 statement {err32:.3e}  bound {R.bound(err32, want):.3e}  "
          f"ambiguous {amb.mean():.2e}")
    assert amb.mean() <= CAP
    assert err <= R.bound(err32, want) and err_ref <= R.bound(err32, want)


def test_the_upper_median_breaks_the_six_point_case(pkg, nz, g):
    """Negative control: against the statement that takes rank n // 2 instead of (n - 1) // 2, the kernel's output is out of bound."""
    got = one_launch(pkg, nz, g, "median_n6")
    want, amb, err32 = statements(g, "median_n6")[0]
    bad, bad_amb, _ = statements(g, "median_n6", "upper_median")[0]
    assert R.error(got, want, amb) <= R.bound(err32, want) < R.error(got, bad, amb | bad_amb)


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
        print(f"{name} call {i}: kernel {err:.3e}  to the reference {err_ref:.3e}  fp32 statement {err32:.3e}  bound {limit:.3e}  "
              f"ambiguous {amb.mean():.2e}")
        assert amb.mean() <= CAP
        assert err <= limit and err_ref <= limit, f"call {i}"
    assert torch.equal(torch.rand(4), torch.from_numpy(g[f"next_{name}"])), "the host generator is not where the reference leaves it"
    assert np.array_equal(g[f"z_{name}"], np.array([gen.z_curr, gen.z_increment]))


def test_the_switch_off_still_refuses_and_draws_nothing(nz):
    latent, params = BY_NAME["median_n5"]
    for cpu in (False, True):
        gen = nz.VoronoiNoiseGenerator(torch.zeros(latent, device=DEV), cpu=cpu, normalized=False, **params)
        assert gen.rank_route is None   # the environment's value, off unless SONAR_VORONOI_RANK is set
        gen.rank_route = False
        torch.manual_seed(5)
        host, dev = torch.get_rng_state(), device_position()
        with pytest.raises(NotImplementedError, match="median_distance needs the whole sorted row per pixel"):
            gen.generate(*SIG)
        assert torch.equal(torch.get_rng_state(), host) and device_position() == dev and gen.feature_points is None
        gen.rank_route = True   # the instance's switch: the same generator now runs
        assert bool(torch.isfinite(gen.generate(*SIG)).all())


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
    torch.manual_seed(4321)
    assert torch.equal(generator(nz, name, cpu=False).generate(*SIG), outs[0])  # the same seed, the same bits


# ------------------------------------------------------------------------------------------------ 4. ranks inside 0..3: the top-four kernel's bits
@pytest.mark.parametrize("dmode, rmode, n, latent", [
    ("euclidean", "diff2", 33, cases.A), ("euclidean", "f4", 33, cases.A), ("euclidean", "f1", 5, cases.B),
    ("chebyshev+quadratic:dscale=0.5", "diff:idx1=1:idx2=3", 257, cases.B),
    ("weight:name=fractal_norm:__name=chebyshev:_mode=sin:h=0.7", "inv_f3+ridge:rscale=0.25+softmin:temperature=20", 33, cases.A),
    ("minkowski:p=2.5", "fractal_norm:name=f2+fractal_norm:mode=cos:name=ridge:__name=diff2", 33, cases.A),
    ("angle_tanh:idx=0", "cellid+inv_f:idx=2", 33, cases.A)])
def test_ranks_inside_the_top_four_give_the_top_four_kernels_bits(pkg, nz, dmode, rmode, n, latent):
    hl = pkg.hip_lib
    gen = torch.Generator().manual_seed(17)
    fp = torch.rand(latent[0], latent[1], n, 3, generator=gen).to(DEV)
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes(dmode, rmode, rank=False)
    prog = hl.voronoi_program(dterms, rterms)
    aux = torch.full((hl.VORONOI_MAX_TERMS,), float(n - 1), device=DEV) if any(r["op"] == "cellid" for r in rterms) else None
    base = torch.rand(latent, generator=gen).to(DEV)   # the launch accumulates: out = (out + result * amplitude) / final_div
    kw = dict(scale=1.7, z_norm=0.3, amplitude=0.75, final_div=1.75, aux=aux)
    top = hl.voronoi_octave_(base.clone(), fp, prog, **kw)
    rank = hl.voronoi_rank_octave_(base.clone(), fp, prog, **kw)
    assert torch.equal(rank, top) and not torch.equal(top, base)
    assert torch.equal(hl.voronoi_rank_octave_(base.clone(), fp, prog, scale=1.7, z_norm=0.3, amplitude=0.75, aux=aux),
                       hl.voronoi_octave_(base.clone(), fp, prog, scale=1.7, z_norm=0.3, amplitude=0.75, aux=aux))


def test_the_fuzz_distance_on_the_rank_route_gives_the_top_four_kernels_bits(pkg, nz):
    """The fuzz distance term's pass 2 is restated in the rank kernel: after the two reducing passes, both routes see the same distances
    (uniforms read by index, and computed from the stream)."""
    hl = pkg.hip_lib
    shape, n = (1, 2, 5, 7), 5
    gen = torch.Generator().manual_seed(11)
    fp, u = torch.rand(1, 2, n, 3, generator=gen).to(DEV), torch.rand(*shape, n, generator=gen).to(DEV)
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes("chebyshev+fuzz:name=weight:h=0.5:fuzz=0.1:dscale=0.5", "diff:idx1=1:idx2=3")
    prog = hl.voronoi_program(dterms, rterms)
    for kw in (dict(u=u), dict(seed=9, stream_id=3, elem_offset=8)):
        fz = hl.VoronoiFuzz(1, 0.1, 10, DEV, **kw)
        for fuzz_pass in (0, 1):
            hl.voronoi_octave_(None, fp, prog, scale=1.0, z_norm=0.25, fuzz=fz, fuzz_pass=fuzz_pass, shape=shape)
        stats = fz.stats.clone()
        top = hl.voronoi_octave_(torch.zeros(shape, device=DEV), fp, prog, scale=1.0, z_norm=0.25, fuzz=fz)
        rank = hl.voronoi_rank_octave_(torch.zeros(shape, device=DEV), fp, prog, scale=1.0, z_norm=0.25, fuzz=fz)
        assert torch.equal(rank, top) and bool(torch.isfinite(top).all()) and torch.equal(fz.stats, stats)


# ------------------------------------------------------------------------------------------------ 5. refusals, before any launch
def test_wrapper_rejections_leave_the_output_untouched(pkg, nz):
    hl = pkg.hip_lib
    gen = nz.VoronoiNoiseGenerator
    fn = hl.load().sonar_voronoi_rank_octave_f32
    fp = torch.rand(2, 3, 33, 3, device=DEV)
    out = torch.full((2, 3, 8, 12), -1.0, device=DEV)

    def program(rmode, n=33):
        d, r = gen.parse_modes("euclidean", rmode, rank=True)
        return hl.voronoi_program(d, gen._resolve(r, n, rmode))

    prog = program("median_distance")
    st, pf, po = hl._stream(), fp.data_ptr(), out.data_ptr()

    def code(fp_=pf, out_=po, aux=None, u=None, stats=None, shape=(2, 3, 8, 12), n=33, flags=0, program_=prog, term=-1):
        return fn(fp_, out_, aux, u, stats, *shape, n, 1.0, 0.25, 1.0, 1.0, flags, hl.C.addressof(program_), term, 0.1, 7, 0, 0, st)

    assert code(fp_=None) == hl.ERR_ARG and code(out_=None) == hl.ERR_ARG and code(out_=pf) == hl.ERR_ARG and code(aux=po) == hl.ERR_ARG
    assert code(shape=(2, 3, 8, -12)) == hl.ERR_ARG and code(n=1) == hl.ERR_ARG and code(n=hl.VORONOI_MAX_POINTS + 1) == hl.ERR_UNSUPPORTED
    assert code(n=16) == hl.ERR_ARG                       # rank 16 of 16 points
    assert code(program_=program("f:idx=-1"), n=32) == hl.ERR_ARG
    bad = program("diff:idx2=9")
    bad.r[0].idx1 = -1
    assert code(program_=bad) == hl.ERR_ARG
    bad = program("diff:idx2=9")
    bad.n_r = hl.VORONOI_MAX_TERMS + 1
    assert code(program_=bad) == hl.ERR_ARG
    bad = program("diff:idx2=9")
    bad.r[0].op = 8
    assert code(program_=bad) == hl.ERR_ARG
    assert code(program_=program("cellid")) == hl.ERR_ARG
    assert code(u=po + 64) == hl.ERR_ARG and code(term=0) == hl.ERR_ARG   # uniforms without a fuzz term, a fuzz term without statistics
    assert code(program_=program("softmin:use_sorted=1"), n=hl.VORONOI_RANK_ROW_N + 1) == hl.ERR_UNSUPPORTED
    for empty in ((0, 3, 8, 12), (2, 3, 0, 12)):
        assert code(shape=empty) == 0
    with pytest.raises(hl.SonarHipError):   # the wrapper checks the tensors against each other
        hl.voronoi_rank_octave_(out, fp[:1], prog, scale=1.0, z_norm=0.0)
    with pytest.raises(hl.SonarHipError):
        hl.voronoi_rank_octave_(out.transpose(2, 3), fp, prog, scale=1.0, z_norm=0.0)
    with pytest.raises(hl.SonarHipError):
        hl.voronoi_rank_octave_(out, fp, program("cellid"), scale=1.0, z_norm=0.0, aux=torch.ones(2, device=DEV))
    with pytest.raises(hl.SonarHipError, match="ranks"):
        hl.voronoi_rank_octave_(out, fp[:, :, :16].contiguous(), prog, scale=1.0, z_norm=0.0)
    with pytest.raises(hl.SonarHipError):   # statistics sized for another shape
        hl.voronoi_rank_octave_(out, fp, prog, scale=1.0, z_norm=0.0, fuzz=hl.VoronoiFuzz(0, 0.1, 7, DEV))
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())


def test_generator_refusals_draw_and_launch_nothing(nz):
    def refused(exc, text, **kw):
        for cpu in (False, True):
            gen = generator(nz, "f_idx4", cpu=cpu, **kw)
            torch.manual_seed(5)
            host, dev = torch.get_rng_state(), device_position()
            with pytest.raises(exc, match=text):
                gen.generate(*SIG)
            assert torch.equal(torch.get_rng_state(), host) and device_position() == dev and gen.feature_points is None

    refused(NotImplementedError, "past f4 beside a bare f term", result_mode=("f1+median_distance",))
    refused(NotImplementedError, "is built up to", n_points=(257,), result_mode=("softmin:use_sorted=1",))
    refused(IndexError, "index 33 is out of bounds for dimension 5 with size 33", result_mode=("f:idx=33",))
    refused(IndexError, "index -34 is out of bounds for dimension 5 with size 33", result_mode=("diff:idx1=-34",))
    refused(IndexError, "index 5 is out of bounds for dimension 5 with size 5", n_points=(33, 5), result_mode=("f1", "f:idx=5"), octaves=2,
            octave_mode="new_features")
