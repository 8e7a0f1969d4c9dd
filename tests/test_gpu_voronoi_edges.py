"""GPU: the Voronoi kernels (csrc/voronoi.hip) at their tile, grid, wave and stream edges -- the launches of tests/voronoi_edge_cases.py,
which tests/test_voronoi_edges_cpu.py shows to reach those edges and to tell a wrong kernel from a right one.

The cases of tests/test_gpu_voronoi.py and tests/test_gpu_voronoi_rank.py stay below 96 pixels a plane, 6 planes and one stream tile of fuzz
uniforms.  Here a plane has more than one 256-pixel tile with a ragged last one, a workgroup takes a second unit of the grid-stride loop, a
wave lies inside one row and a row in two workgroups (the wave-aggregated statistics of fuzz pass 1), the fuzz distance reads its stream
past a tile, from an element offset and from a chunk base of 256, the points fill 16 staging chunks, and the plane kernels take a second
trip of their loops.

The rules are the existing ones.  Against the fp64 statement (tests/voronoi_refs.py, tests/voronoi_rank_refs.py): over the elements the
statement does not flag, |kernel - fp64 statement| <= 8 x |fp32 statement - fp64 statement| (floor 1e-6 of the output range,
tests/voronoi_refs.bound), the flagged share under the cases' caps.  Everything else is equal bits: the statistics words of the reducing
passes against the same fp32 reductions in numpy, stream mode against replay mode on the host-stated stream
(oracle/device_streams.py), the rank route on ranks 0..3 against the top-four kernel, the plane kernels against numpy's fp32."""
import importlib

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from tests import voronoi_edge_cases as E
from tests import voronoi_edge_refs as X
from tests import voronoi_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIG = (torch.tensor(10.0), torch.tensor(5.0))
GUARD = 64


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def ng(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise_generation")


def device_position():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset() // 4


def guarded(shape, fill, dtype=torch.float32):
    """A tensor of ``shape`` in the middle of a larger buffer, and the check that the words around it kept their value."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)

    def intact():
        return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + numel:] == fill).all())

    return buf[GUARD:GUARD + numel].view(shape), intact


def judge(name, got, st, cap):
    err, share = R.error(got, st.want, st.amb), float(st.amb.mean())
    print(f"{name}: kernel {err:.3e}  fp32 statement {st.err32:.3e}  bound {st.bound:.3e}  ambiguous {share:.2e}")
    assert share <= cap
    assert err <= st.bound


def cap(name):
    return E.CAP_WIDE if name in E.WIDE else E.CAP


def tags(*tables):
    """The tags of the tables' cases, in order: a test per tag runs every case of the tag."""
    return list(dict.fromkeys(case[1] for table in tables for case in table))


def each(cases, run):
    """``run(case)`` for every case, all of them whatever fails; the failures are reported together, by case."""
    assert cases
    failed = []
    for case in cases:
        try:
            run(case)
        except AssertionError as exc:
            failed.append(f"{case[0]}: {exc}")
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ 1. the top-four kernel's launch geometry
@pytest.mark.parametrize("tag", tags(E.OCTAVE))
def test_octave_launch_geometry(pkg, nz, tag):
    """One launch, both instantiations without a fuzz term: tiles and a ragged last one (T3, R192), a second unit per workgroup (G2100),
    sixteen chunks (N4096); accumulated into a random base with an amplitude and the final division."""
    each([c for c in E.OCTAVE if c[1] == tag], lambda case: octave_launch(pkg.hip_lib, nz, case))


def octave_launch(hl, nz, case):
    name, tag, n, dmode, rmode, scale = case
    shape = E.SHAPES[tag]
    fp_np, into, st = X.case_statement(False, case)
    fp = torch.from_numpy(fp_np).to(DEV)
    before = fp.clone()
    out, intact = guarded(shape, -7.0)
    out.copy_(torch.from_numpy(into))
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes(dmode, rmode)
    prog = hl.voronoi_program(dterms, rterms)
    simple = len(dterms) == 1 and len(rterms) == 1 and not dterms[0]["xforms"] and not rterms[0]["fns"]
    assert simple == (dmode == "euclidean")   # the plain instantiation and the general one
    aux = None
    if rmode == "cellid":
        raw = hl.voronoi_program(dterms, [{"op": "cellid_raw"}])
        ids = hl.voronoi_octave_(torch.zeros(shape, device=DEV), fp, raw, scale=scale, z_norm=E.Z_NORM, amplitude=1.0).cpu().numpy()
        first = st.o64.dist.argmin(axis=-1)   # (numpy's argmin is the first of equals, as the kernel's `<`)
        assert np.array_equal(ids[~st.amb], first[~st.amb]) and 0 <= ids.min() and ids.max() <= n - 1
        aux = torch.ones(hl.VORONOI_MAX_TERMS, device=DEV)
        aux[0] = float(ids.max())
    assert hl.voronoi_octave_(out, fp, prog, scale=scale, z_norm=E.Z_NORM, amplitude=E.AMPLITUDE, final_div=E.FINAL_DIV, aux=aux) is out
    judge(name, out.cpu().numpy(), st, cap(name))
    assert torch.equal(fp, before) and intact()


# ------------------------------------------------------------------------------------------------ 2. the fuzz distance, pass by pass
def fuzz_term(dterms):
    term = next(t for t, d in enumerate(dterms) if "fuzz" in d)
    return term, dterms[term]["fuzz"]


def words(stats):
    return stats.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("tag", tags(E.FUZZ_REPLAY))
def test_the_fuzz_passes_at_the_wave_and_tile_edges(pkg, nz, tag):
    """Replay mode.  Pass 0 leaves the inner distance's whole-tensor extremes, pass 1 the fuzzed distance's per (b, c, y) row, as ordered
    integers equal to numpy's fp32 reductions: through the per-thread atomics where a wave straddles rows (T3, G2100), through one atomic
    pair per wave where it lies inside a row (R192, R64), two workgroups into one row's slot (R192), a second unit per workgroup and 4200
    rows (G2100).  Nothing else is written before pass 2, which is held to the fp64 statement."""
    each([c for c in E.FUZZ_REPLAY if c[1] == tag], lambda case: fuzz_passes(pkg.hip_lib, nz, case))


def fuzz_passes(hl, nz, case):
    name, tag, n, dmode, rmode, scale, exact = case
    shape = E.SHAPES[tag]
    rows = shape[0] * shape[1] * shape[2]
    fp_np, u_np, st = X.replay_statement(case)
    fp, u = torch.from_numpy(fp_np).to(DEV), torch.from_numpy(u_np).to(DEV)
    kept = (fp.clone(), u.clone())
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes(dmode, rmode)
    prog = hl.voronoi_program(dterms, rterms)
    fz = hl.VoronoiFuzz(*fuzz_term(dterms), rows, DEV, u=u)
    stats, stats_intact = guarded((2 + 2 * rows,), 12345, torch.int32)
    stats.copy_(fz.stats)
    fz.stats = stats
    out, intact = guarded(shape, -3.0)
    want = X.statistics_words(st.o32)
    kw = dict(scale=scale, z_norm=E.Z_NORM, fuzz=fz)
    hl.voronoi_octave_(None, fp, prog, fuzz_pass=0, shape=shape, **kw)
    got = words(stats)
    assert bool((got[2::2] == 0xFFFFFFFF).all()) and bool((got[3::2] == 0).all())
    if exact:
        assert np.array_equal(got[:2], want[:2])
    hl.voronoi_octave_(None, fp, prog, fuzz_pass=1, shape=shape, **kw)
    got = words(stats)
    if exact:
        wrong = np.flatnonzero((got[2::2] != want[2::2]) | (got[3::2] != want[3::2]))
        assert wrong.size == 0, f"rows {wrong[:8]} of {rows}"
        assert np.array_equal(got, want)
    assert bool((out == -3.0).all())
    out.zero_()
    assert hl.voronoi_octave_(out, fp, prog, **kw) is out
    judge(name, out.cpu().numpy(), st, cap(name))
    assert np.array_equal(words(stats), got) and stats_intact() and intact()
    assert torch.equal(fp, kept[0]) and torch.equal(u, kept[1])


# ------------------------------------------------------------------------------------------------ 3. stream mode is replay mode on the stated stream
def three_passes(hl, nz, case, rank, **source):
    """Passes 0 and 1 and the real pass of a fuzz distance term, the last one on either route: (statistics words, output)."""
    _name, tag, n, dmode, rmode = case
    shape = E.SHAPES[tag]
    gen = nz.VoronoiNoiseGenerator
    fp = torch.from_numpy(X.points(tag, n, rank)).to(DEV)
    dterms, rterms = gen.parse_modes(dmode, rmode, rank=rank)
    fz = hl.VoronoiFuzz(*fuzz_term(dterms), shape[0] * shape[1] * shape[2], DEV, **source)
    reduce = hl.voronoi_program(dterms, [{"op": "f"}])
    for fuzz_pass in (0, 1):
        hl.voronoi_octave_(None, fp, reduce, scale=1.0, z_norm=E.Z_NORM, fuzz=fz, fuzz_pass=fuzz_pass, shape=shape)
    stats = fz.stats.clone()
    out = torch.zeros(shape, device=DEV)
    if rank:
        hl.voronoi_rank_octave_(out, fp, hl.voronoi_program(dterms, gen._resolve(rterms, n, rmode)), scale=1.0, z_norm=E.Z_NORM, fuzz=fz)
    else:
        hl.voronoi_octave_(out, fp, hl.voronoi_program(dterms, rterms), scale=1.0, z_norm=E.Z_NORM, fuzz=fz)
    assert torch.equal(fz.stats, stats)
    return stats, out


def stream_is_replay(hl, nz, case, rank, offset):
    _name, tag, n, _dmode, _rmode = case
    shape = E.SHAPES[tag]
    u = ds.uniform_fill(E.STREAM_SEED, E.STREAM_ID, int(np.prod(shape)) * n, offset).reshape(*shape, n)
    stats_u, out_u = three_passes(hl, nz, case, rank, u=torch.from_numpy(u).to(DEV))
    stats_s, out_s = three_passes(hl, nz, case, rank, seed=E.STREAM_SEED, stream_id=E.STREAM_ID, elem_offset=offset)
    differ = np.flatnonzero(words(stats_u) != words(stats_s))
    assert differ.size == 0, f"statistics words {differ[:8]}"
    bad = torch.nonzero(out_u != out_s)
    assert bad.numel() == 0, f"{bad.shape[0]} outputs differ, the first at {bad[0].tolist()}"
    assert torch.equal(out_s, out_u) and bool(torch.isfinite(out_s).all()) and float(out_s.abs().max()) > 0.0


@pytest.mark.parametrize("tag", tags(E.STREAM, E.RANK_STREAM))
def test_stream_mode_is_replay_mode_on_the_stated_stream(pkg, nz, tag):
    """The uniform the kernel computes for element elem_offset + flat + base + j is the one sonar_philox_uniform_f32 fills there: past the
    first stream tile (every case), from offsets inside a group of four, at a tile's end and beyond 2^33, and with a chunk base of 256
    (N257F).  Equal statistics words and equal outputs, at every offset.  The rank kernel restates the stream addressing (its slot pick
    is two selects), and reads each uniform in all 33 sweeps -- and again in the row instantiation's LDS pass."""
    runs = [(f"{'rank ' if rank else ''}{c[0]} at offset {offset}", rank, c, offset)
            for rank, table in ((False, E.STREAM), (True, E.RANK_STREAM)) for c in table if c[1] == tag for offset in E.OFFSETS]
    assert {r[1] for r in runs} == {False, True}
    each(runs, lambda run: stream_is_replay(pkg.hip_lib, nz, run[2], run[1], run[3]))


# ------------------------------------------------------------------------------------------------ 4. the rank kernel's launch geometry
@pytest.mark.parametrize("tag", tags(E.RANK))
def test_rank_launch_geometry(pkg, nz, tag):
    """One launch of the rank kernel: 256-pixel tiles (the median, diff) and the row instantiation's 64-pixel tiles (softmin:use_sorted),
    three and ten tiles a plane with a ragged last one (T3), a second unit per workgroup (G2100), sixteen chunks in every sweep (N4096)."""
    each([c for c in E.RANK if c[1] == tag], lambda case: rank_launch(pkg.hip_lib, nz, case))


def rank_launch(hl, nz, case):
    gen = nz.VoronoiNoiseGenerator
    name, tag, n, dmode, rmode, scale = case
    shape = E.SHAPES[tag]
    fp_np, into, st = X.case_statement(True, case)
    fp = torch.from_numpy(fp_np).to(DEV)
    before = fp.clone()
    out, intact = guarded(shape, -7.0)
    out.copy_(torch.from_numpy(into))
    dterms, rterms = gen.parse_modes(dmode, rmode, rank=True)
    prog = hl.voronoi_program(dterms, gen._resolve(rterms, n, rmode))
    assert hl.voronoi_rank_octave_(out, fp, prog, scale=scale, z_norm=E.Z_NORM, amplitude=E.AMPLITUDE, final_div=E.FINAL_DIV) is out
    judge(name, out.cpu().numpy(), st, cap(name))
    assert torch.equal(fp, before) and intact()


@pytest.mark.parametrize("tag", tags([(None, *c) for c in E.TOP_FOUR]))
def test_ranks_inside_the_top_four_give_the_top_four_kernels_bits_at_the_edges(pkg, nz, tag):
    each([(f"{d} / {r} on {n} points", t, n, d, r) for t, n, d, r in E.TOP_FOUR if t == tag], lambda case: same_bits(pkg.hip_lib, nz, *case[1:]))


def same_bits(hl, nz, tag, n, dmode, rmode):
    shape = E.SHAPES[tag]
    fp = torch.from_numpy(X.points(tag, n, True)).to(DEV)
    dterms, rterms = nz.VoronoiNoiseGenerator.parse_modes(dmode, rmode, rank=False)
    prog = hl.voronoi_program(dterms, rterms)
    aux = torch.full((hl.VORONOI_MAX_TERMS,), float(n - 1), device=DEV) if any(r["op"] == "cellid" for r in rterms) else None
    base = torch.from_numpy(X.base(tag)).to(DEV)
    kw = dict(scale=1.7, z_norm=0.3, amplitude=E.AMPLITUDE, final_div=E.FINAL_DIV, aux=aux)
    top = hl.voronoi_octave_(base.clone(), fp, prog, **kw)
    rank = hl.voronoi_rank_octave_(base.clone(), fp, prog, **kw)
    bad = torch.nonzero(rank != top)
    assert bad.numel() == 0, f"{bad.shape[0]} outputs differ, the first at {bad[0].tolist()}"
    assert torch.equal(rank, top) and not torch.equal(top, base) and bool(torch.isfinite(top).all())


# ------------------------------------------------------------------------------------------------ 5. the generator under a shard offset, with fuzz
@pytest.mark.parametrize("name, rank, latent, params", E.GENERATOR, ids=[c[0] for c in E.GENERATOR])
def test_generate_under_a_shard_offset_is_replay_on_the_offset_streams(pkg, nz, ng, name, rank, latent, params):
    """The second latent of a larger batch, generate mode: draw k is stream + k from the latent's first element on -- the feature points
    and the [B, C, H, W, N] uniforms the kernel computes (6030 elements in: past a stream tile, inside a group of four).  (A shard is
    NOT the rows of the full batch here: the fuzz extremes are whole-tensor quantities.)"""
    def generator(cpu):
        gen = nz.VoronoiNoiseGenerator(torch.zeros(latent, device=DEV), cpu=cpu, normalized=False, **params)
        gen.rank_route = rank
        return gen

    with ng.shard_offset(1):
        gen = generator(False)
        torch.manual_seed(4321)
        seed, stream = device_position()
        host_state = torch.get_rng_state()
        outs = [gen.generate(*SIG) for _ in range(E.GENERATOR_CALLS)]
        taken = []
        twin = generator(True)

        def rand_like(*, fun, shape, **_kw):
            assert fun is torch.rand and shape[0] == latent[0]
            numel, per_latent = int(np.prod(shape)), int(np.prod(shape[1:]))
            taken.append(tuple(shape))
            return torch.from_numpy(ds.uniform_fill(seed, stream + len(taken) - 1, numel, 1 * per_latent).reshape(shape)).to(DEV)

        twin.rand_like = rand_like
        for i in range(E.GENERATOR_CALLS):
            got = twin.generate(*SIG)
            bad = torch.nonzero(got != outs[i])
            assert bad.numel() == 0, f"call {i}: {bad.shape[0]} outputs differ, the first at {bad[0].tolist()}"
            assert torch.equal(got, outs[i]) and bool(torch.isfinite(got).all())
        n = params["n_points"][0]
        assert taken == [(latent[0], latent[1], n, 3)] + [(*latent, n)] * E.GENERATOR_CALLS   # the points once, the uniforms per call
        assert device_position() == (seed, stream + len(taken)) and torch.equal(torch.get_rng_state(), host_state)
    assert not torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 6. the plane kernels past one grid
def test_the_plane_kernels_past_one_grid(pkg):
    """gradient, fuzz add and accumulation on 3 x 419 x 421: 529197 elements for 2048 x 256 threads, so 4909 threads take a second
    element, 1245 rows and a third further on (the third plane).  Equal bits with the same fp32 operations in numpy."""
    hl = pkg.hip_lib
    shape = E.SHAPES["P"]
    rng = np.random.default_rng(E.SEED_BASE)
    n1, n2, nu, want = (rng.random(shape, dtype=np.float32) for _ in range(4))
    r1, r2, u = (torch.from_numpy(v).to(DEV) for v in (n1, n2, nu))
    acc, intact = guarded(shape, -7.0)
    acc.copy_(torch.from_numpy(want))
    f = np.float32

    def differing(want):
        bad = np.argwhere(acc.cpu().numpy() != want)
        return f"{len(bad)} elements differ" + (f", the first at {bad[0].tolist()}" if len(bad) else "")

    p1, p2 = (np.pad(r, [(0, 0), (0, 0), (1, 1), (1, 1)], mode="edge") for r in (n1, n2))
    dx, dy = p1[..., 1:-1, 2:] - p2[..., 1:-1, :-2], p1[..., 2:, 1:-1] - p2[..., :-2, 1:-1]
    want = want + np.sqrt(dx * dx + dy * dy) * f(0.3)
    assert hl.voronoi_gradient_(acc, r1, r2, 0.3) is acc
    assert np.array_equal(acc.cpu().numpy(), want), differing(want)
    want = want + (nu * f(0.2 * 2) - f(0.2))
    hl.voronoi_fuzz_add_(acc, u, 0.2)
    assert np.array_equal(acc.cpu().numpy(), want), differing(want)
    want = (want + n1 * f(0.75)) / f(1.75)
    hl.voronoi_acc_(acc, r1, 0.75, final_div=1.75)
    assert want.dtype == np.float32 and np.array_equal(acc.cpu().numpy(), want), differing(want)
    assert intact() and np.array_equal(r1.cpu().numpy(), n1) and np.array_equal(r2.cpu().numpy(), n2) and np.array_equal(u.cpu().numpy(), nu)
