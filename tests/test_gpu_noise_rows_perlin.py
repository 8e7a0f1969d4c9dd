"""Row-keyed Perlin noise (-m gpu): ``sonar_perlin_rows_f32`` against the per-call kernels it stands in for (lattice, then generate or the
normalising pair, bit for bit) on every launch route and at the edges of its turn-by-turn statistics, against the host statement of one
row (tests/perlin_rows_refs.py), at its bounds; and ``CustomNOISE.generate_noise`` with ``batch_index`` through it against the per-index
loop (bit for bit), with the launches counted.

Bounds are those of tests/test_gpu_perlin_oracle.py, imported, not restated: the lattice within LATTICE_TOL per iteration of the fp64
lattice; raw values by that file's raw-value rule (``_check_raw``: float32_steps' bits over the device's own lattice); normalised values
within NORMAL_TOL * 2 * max(1, factor) per (1 + |z|) plus the lattice's bound scaled by factor / std, as its generator test allows."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import perlin_rows_refs as refs
from tests.test_gpu_perlin_oracle import INV_SQRT12, LATTICE_TOL, NORMAL_TOL, _check_raw, _route, _tile_grid

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1
STREAM = 2**32 + 3
SEEDS = (3, 2**64 - 1, 3, 2**63, 12345)      # (rows 0 and 2 share a seed: their streams differ)
OFFSETS = (6, 0, 2**40, 2, 10)               # misordered, none a neighbour's lattice stream
DIVISORS = (2.0, 1.5, -1.7)                  # a power of two (WordScale / the exact multiply) and two that divide
LATTICES = ((0, "lerp"), (1, "inject"), (2, "subtract_b"), (5, "lerp"))
FORMS = ((True, 1.0), (True, 0.7), (False, 1.0), (False, 0.37))  # (normalised, factor)
# (shape, route, tile_grid): every route of launch_perlin_generate for ONE latent, and the edges of the row kernel's turns
SHAPES = [
    ((1, 1, 1), "scalar", 1),
    ((3, 5, 7), "scalar", 1),        # 105: rows land on every address residue
    ((1, 2, 2), "vector", 1),
    ((2, 8, 8), "vector", 1),
    ((1, 16, 16), "fast", 1),
    ((1, 13, 20), "fast", 1),        # 260: the tile reaches past the latent
    ((1, 50, 82), "fast", 1),        # 4100: a ragged second tile
    ((1, 64, 64), "aligned", 1),     # one tile
    ((5, 64, 64), "aligned", 2),     # five tiles: the row's workgroup plays two turns
    ((5, 128, 128), "aligned", 5),   # twenty tiles, five turns
    ((1, 260, 260), "fast", 5),      # 67600: seventeen tiles, the last one ragged, five turns
]


@pytest.fixture(scope="module")
def hl(pkg):
    pkg.hip_lib.load()
    return pkg.hip_lib


def _same(a, b):
    """torch.equal with equal_nan=True."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _stream_of(r):
    return (STREAM + OFFSETS[r]) & M64


def _loop_row(hl, seed, stream, shape, iters, blend, d, normalized, factor):
    """(one row, its lattice) as the loop's batch-1 call gives them, on tensors of their own."""
    c, h, w = shape
    terms = hl.perlin_lattice(iters, c, h, w, "cuda", blend, seed, (stream + 1) & M64)
    if normalized:
        return hl.perlin_noise((1, c, h, w), terms, d, seed, stream, 0, factor)[0], terms[0]
    x = hl.perlin_generate((1, c, h, w), terms, d, seed, stream, 0, partials=hl.new_partials("cuda"))
    if factor != 1.0:
        hl.scale_noise_(x, factor, False, None)
    return x[0], terms[0]


@pytest.mark.parametrize("shape, route, grid", SHAPES, ids=["x".join(map(str, s)) for s, _, _ in SHAPES])
def test_rows_are_the_per_call_kernels_bits(hl, shape, route, grid):
    """1, 3 and 5 rows with distinct keys over every (lattice, divisor, form) of the grid at this shape; the reference rows are computed
    once per combination and shared by the three row counts."""
    chw = math.prod(shape)
    assert _route(chw, 1, 0) == route and _tile_grid(hl, chw, 0) == grid  # the launcher's conditions, restated by the per-call tests
    for iters, blend in LATTICES:
        for d in DIVISORS:
            for normalized, factor in FORMS:
                want = [_loop_row(hl, SEEDS[r], _stream_of(r), shape, iters, blend, d, normalized, factor) for r in range(5)]
                for rows in (1, 3, 5):
                    picks = list(range(rows)) if rows != 3 else [4, 1, 2]
                    lattice = torch.full((rows, *shape), float("nan"), device="cuda")
                    got = hl.perlin_rows((rows, *shape), "cuda", [SEEDS[r] for r in picks], STREAM, iterations=iters, div_fac=d, blend_mode=blend,
                                         factor=factor, normalized=normalized, row_streams=[OFFSETS[r] for r in picks], lattice=lattice)
                    for i, r in enumerate(picks):
                        assert torch.equal(lattice[i], want[r][1]), (iters, blend, rows, i)
                        assert _same(got[i], want[r][0]), (iters, blend, d, normalized, factor, rows, i)
                if chw > 1:
                    assert not torch.isnan(got).any() and not _same(got[0], got[2])


def test_device_keys_and_no_row_streams(hl):
    """Device tensors of keys (int64 bit patterns / uint64) are taken as they are; without ``row_streams`` every row draws on ``stream_id``."""
    shape, kw = (2, 8, 8), dict(iterations=2, div_fac=2.0, blend_mode="lerp", factor=1.0, normalized=True)
    want = torch.stack([_loop_row(hl, SEEDS[r], _stream_of(r), shape, 2, "lerp", 2.0, True, 1.0)[0] for r in range(5)])
    as_i64 = lambda v: torch.tensor([x - 2**64 if x >= 2**63 else x for x in v], dtype=torch.int64, device="cuda")  # noqa: E731
    assert _same(hl.perlin_rows((5, *shape), "cuda", as_i64(SEEDS), STREAM, row_streams=as_i64(OFFSETS), **kw), want)
    assert _same(hl.perlin_rows((5, *shape), "cuda", as_i64(SEEDS).view(torch.uint64), STREAM, row_streams=list(OFFSETS), **kw), want)
    flat = hl.perlin_rows((2, *shape), "cuda", [SEEDS[1], SEEDS[4]], _stream_of(3), **kw)
    assert _same(flat[0], _loop_row(hl, SEEDS[1], _stream_of(3), shape, 2, "lerp", 2.0, True, 1.0)[0])
    assert _same(flat[1], _loop_row(hl, SEEDS[4], _stream_of(3), shape, 2, "lerp", 2.0, True, 1.0)[0])


# (shape, iterations, blend, divisor): one per route, both kinds of divisor on the general and on the fast routes; the divisors are ones
# whose rows' decisions are clear of their thresholds on the host (105 elements with div_fac 2: |mean| 0.25 against a threshold of 0.244)
HOST_CASES = [
    ((3, 5, 7), 2, "lerp", 1.5), ((2, 8, 8), 5, "inject", 0.5), ((1, 13, 20), 1, "subtract_b", -1.7), ((1, 64, 64), 2, "lerp", 2.0),
    ((5, 64, 64), 2, "inject", 1.5),
]


def _clear(dec):
    """Mean and std at least 25 % of the threshold away from it (tests/test_gpu_perlin_oracle.py: _clear_decisions)."""
    thr = dec["threshold"]
    return abs(abs(dec["mean"]) - thr) >= 0.25 * thr and abs(abs(1.0 - dec["std"]) - thr) >= 0.25 * thr


@pytest.mark.parametrize("shape, iters, blend, d", HOST_CASES, ids=["x".join(map(str, c[0])) for c in HOST_CASES])
def test_rows_against_the_host_statement(hl, shape, iters, blend, d):
    chw = math.prod(shape)
    picks = [4, 1, 3]
    seeds, offs = [SEEDS[r] for r in picks], [OFFSETS[r] for r in picks]
    kw = dict(iterations=iters, div_fac=d, blend_mode=blend)
    lattice = torch.full((3, *shape), float("nan"), device="cuda")
    raw = hl.perlin_rows((3, *shape), "cuda", seeds, STREAM, factor=1.0, normalized=False, row_streams=offs, lattice=lattice, **kw)
    for i, r in enumerate(picks):
        seed, stream = SEEDS[r], _stream_of(r)
        lat_err = float(np.max(np.abs(lattice[i].cpu().double().numpy() - refs.row_lattice(seed, stream, shape, iters, blend))))
        print(f"{shape} row {i}: lattice max |kernel - fp64| = {lat_err:.3e} (bound {iters * LATTICE_TOL:.2e})")
        assert lat_err <= iters * LATTICE_TOL
        _check_raw(raw[i], lattice[i].view(1, chw), seed, stream, chw, d, chw, 0, family="perlin_rows_raw")  # over the device's own lattice
    for factor in (1.0, 0.7):
        got = hl.perlin_rows((3, *shape), "cuda", seeds, STREAM, factor=factor, normalized=True, row_streams=offs, **kw).cpu().double().numpy()
        for i, r in enumerate(picks):
            dec = {}
            want = refs.row(SEEDS[r], _stream_of(r), shape, factor=factor, normalized=refs.FUSED, decisions=dec, **kw)
            assert dec["sub"] and dec["div"] and _clear(dec), dec
            err = np.abs(got[i].reshape(-1) - want)
            bound = NORMAL_TOL * 2 * max(1.0, factor) * (1.0 + np.abs(want)) + iters * LATTICE_TOL * factor / dec["std"]
            print(f"{shape} factor {factor} row {i}: max err / bound = {float(np.max(err / bound)):.3f}")
            assert np.all(err <= bound)


# Keys of the rows of the subtract-only case, chosen on the host (refs.row's decisions for every shape below: |mean| 6 to 43 thresholds
# above its threshold, |1 - std| at most 0.5 of its threshold); the test asserts it again.
SUB_ONLY_STREAM, SUB_ONLY_SEEDS, SUB_ONLY_OFFSETS = 7, (5, 2**32 + 5, 12345), (0, 2**32 - 4, 3)


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 8, 8), (1, 13, 20), (1, 64, 64)], ids=["scalar", "vector", "fast", "aligned"])
def test_a_row_that_is_shifted_but_not_scaled(hl, shape):
    """No lattice iterations and div_fac = float32(1 / sqrt(12)): u / d has unit variance and mean sqrt(3) -- the decision subtracts and
    does not scale (NormT<true, false> with factor 1, <true, true> with another)."""
    kw = dict(iterations=0, div_fac=INV_SQRT12, blend_mode="lerp")
    for factor in (1.0, 0.7):
        got = hl.perlin_rows((3, *shape), "cuda", SUB_ONLY_SEEDS, SUB_ONLY_STREAM, factor=factor, normalized=True, row_streams=SUB_ONLY_OFFSETS, **kw)
        for i, (seed, off) in enumerate(zip(SUB_ONLY_SEEDS, SUB_ONLY_OFFSETS)):
            dec = {}
            want = refs.row(seed, SUB_ONLY_STREAM + off, shape, factor=factor, normalized=refs.FUSED, decisions=dec, **kw)
            assert dec["sub"] and not dec["div"] and _clear(dec), dec
            err = np.abs(got[i].cpu().double().numpy().reshape(-1) - want)
            assert np.all(err <= NORMAL_TOL * 2 * max(1.0, factor) * (1.0 + np.abs(want)))
            assert _same(got[i], _loop_row(hl, seed, SUB_ONLY_STREAM + off, shape, 0, "lerp", INV_SQRT12, True, factor)[0])


def test_nothing_is_written_outside_the_rows(hl):
    """NaN guards around ``out`` (also with the first row off a 16-byte boundary) and around the rows' slice of the lattice workspace."""
    for rows, shape, lead in ((5, (3, 5, 7), 0), (5, (3, 5, 7), 1), (3, (1, 50, 82), 3), (2, (1, 16, 16), 2), (2, (1, 64, 64), 1), (3, (1, 2, 2), 0)):
        chw = math.prod(shape)
        n = rows * chw
        buf = torch.full((n + 64,), float("nan"), device="cuda")
        out = buf[16 + lead:16 + lead + n].view(rows, *shape)  # lead: the first row itself off a 16-byte boundary
        lbuf = torch.full((n + 2 * chw + 64,), float("nan"), device="cuda")
        first = (chw + 3) // 4 * 4  # a 16-byte aligned slice with a latent or more of guard on either side
        lattice = lbuf[first:first + n].view(rows, *shape)
        seeds, offs = [SEEDS[r] for r in range(rows)], [OFFSETS[r] for r in range(rows)]
        for normalized in (True, False):
            buf.fill_(float("nan"))
            lbuf.fill_(float("nan"))
            hl.perlin_rows((rows, *shape), "cuda", seeds, STREAM, iterations=2, div_fac=1.5, blend_mode="lerp", factor=0.37, normalized=normalized,
                           row_streams=offs, out=out, lattice=lattice)
            assert not out.isnan().any() and not lattice.isnan().any()
            assert buf[:16 + lead].isnan().all() and buf[16 + lead + n:].isnan().all()
            assert lbuf[:first].isnan().all() and lbuf[first + n:].isnan().all()
            for r in range(rows):
                row, terms = _loop_row(hl, seeds[r], _stream_of(r), shape, 2, "lerp", 1.5, normalized, 0.37)
                assert _same(out[r], row) and torch.equal(lattice[r], terms)
    # a launch of fewer rows leaves the workspace of the other rows alone
    ws = torch.full((4, 2, 8, 8), float("nan"), device="cuda")
    hl.perlin_rows((2, 2, 8, 8), "cuda", [1, 2], STREAM, iterations=2, div_fac=2.0, blend_mode="lerp", factor=1.0, normalized=True, lattice=ws[1:3])
    assert not ws[1:3].isnan().any() and ws[0].isnan().all() and ws[3].isnan().all()


def _traced(hl, fn):
    """The names of the library calls ``fn`` makes, host queries left out, through the trace recorder."""
    names = []
    rec = hl._Recorder(hl.load_raw())
    rec.on_call = lambda name, args, rc: names.append(name) if name not in hl._HOST_QUERIES else None
    hl._recorder = rec
    try:
        fn()
    finally:
        hl._recorder = None
    return names


def test_refusals_launch_nothing(hl):
    lib = hl.load()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((4, 1, 8, 8), float("nan"), device="cuda")
    lattice = torch.full((4, 1, 8, 8), float("nan"), device="cuda")
    seeds = torch.zeros(4, dtype=torch.int64, device="cuda")
    limit = lib.sonar_philox_rows_max_inner()

    def call(o=out.data_ptr(), lat=lattice.data_ptr(), rows=4, c=1, h=8, w=8, iters=2, blend=0, row_seed=seeds.data_ptr(), normalized=2):
        return lib.sonar_perlin_rows_f32(o, lat, rows, c, h, w, iters, blend, 2.0, row_seed, None, 5, 1.0, normalized, 2.5, st)

    assert call(rows=-1) == hl.ERR_UNSUPPORTED and call(row_seed=None) == hl.ERR_UNSUPPORTED
    assert call(w=limit + 1) == hl.ERR_UNSUPPORTED and call(h=2**20) == hl.ERR_UNSUPPORTED and call(c=limit, h=2) == hl.ERR_UNSUPPORTED
    assert call(c=0) == hl.ERR_ARG and call(iters=-1) == hl.ERR_ARG and call(blend=3) == hl.ERR_ARG
    assert call(normalized=1) == hl.ERR_ARG and call(normalized=3) == hl.ERR_ARG
    assert call(o=None) == hl.ERR_ARG and call(o=out.data_ptr() + 2) == hl.ERR_ARG
    assert call(lat=None) == hl.ERR_ARG and call(lat=lattice.data_ptr() + 4) == hl.ERR_ARG and call(lat=out.data_ptr()) == hl.ERR_ARG
    assert call(rows=0) == 0 and call(rows=0, row_seed=None) == 0
    torch.cuda.synchronize()
    assert out.isnan().all() and lattice.isnan().all()
    kw = dict(iterations=2, div_fac=2.0, blend_mode="lerp", factor=1.0, normalized=True, out=out, lattice=lattice)

    def refused():
        for bad in (dict(row_seeds=[1, 2, 3]), dict(blend_mode="slerp"), dict(normalized=1), dict(lattice=lattice[:3])):
            with pytest.raises(hl.SonarHipError):
                hl.perlin_rows((4, 1, 8, 8), "cuda", **({"row_seeds": [1, 2, 3, 4], "stream_id": 5} | kw | bad))

    assert _traced(hl, refused) == []  # the wrapper's own refusals never reach the library
    assert out.isnan().all() and lattice.isnan().all()
    assert _traced(hl, lambda: hl.perlin_rows((4, 1, 8, 8), "cuda", [1, 2, 3, 4], 5, **kw)) == ["sonar_perlin_rows_f32"]
    assert not out.isnan().any() and not lattice.isnan().any()


# ------------------------------------------------------------------------------------------------ CustomNOISE.generate_noise
@pytest.fixture(scope="module")
def mods(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise"), importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


def _noise_object(mods, normalize, multiplier, factor=1.0, seed=1234):
    noise, reg = mods
    chain = noise.CustomNoiseChain([noise.CustomNoiseItem(factor, noise_type=noise.NoiseType.PERLIN)])
    return reg.CustomNOISE(chain, seed, cpu_noise=False, normalize=normalize, multiplier=multiplier)


def _position():
    return torch.cuda.default_generators[torch.cuda.current_device()].get_offset()


def _both_routes(mods, monkeypatch, nobj, latent):
    """(the row route's result, the loop's, the samplers the row route was given, the device generator's position after each)."""
    noise = mods[0]
    made = []
    real = noise.CustomNoiseChain.make_row_seeded_sampler

    def spy(self, *a, **k):
        made.append(real(self, *a, **k))
        return made[-1]

    with monkeypatch.context() as m:
        m.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", spy)
        rows = nobj.generate_noise(latent)
    at_rows = _position()
    with monkeypatch.context() as m:
        m.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", lambda self, *a, **k: None)
        loop = nobj.generate_noise(latent)
    return rows, loop, made, at_rows, _position()


@pytest.mark.parametrize("shape", [(5, 4, 8, 8), (3, 16, 2, 6, 6)], ids=["4d", "5d"])
@pytest.mark.parametrize("inds", [[0, 1, 2, 3, 4], [3, 3, 0, 7, 1], [2]], ids=["all", "mixed", "one"])
def test_batch_index_is_the_loops_result(mods, monkeypatch, shape, inds):
    for dtype in (torch.float32, torch.float16):
        for normalize in (True, False):
            for multiplier in (1.0, 0.5):
                nobj = _noise_object(mods, normalize, multiplier)
                latent = {"samples": torch.zeros(shape, dtype=dtype), "batch_index": inds}
                rows, loop, made, at_rows, at_loop = _both_routes(mods, monkeypatch, nobj, latent)
                assert len(made) == 1 and made[0] is not None, "the row route was not taken"
                assert rows.dtype == dtype and rows.device.type == "cpu" and tuple(rows.shape) == (len(inds), *shape[1:])
                assert torch.equal(rows, loop), (dtype, normalize, multiplier)
                assert at_rows == at_loop == 4 * 2 * (max(inds) + 1)  # two stream ids per index up to the largest, on either route
                assert rows.float().abs().max() > 0.1


@pytest.mark.parametrize("factor, normalize, taken", [(0.5, False, True), (-1.0, False, True), (2.0, False, True), (0.5, True, False)])
def test_item_factors_fold_or_stay_on_the_loop(mods, monkeypatch, factor, normalize, taken):
    """Unnormalised chains: item factor, chain factor and multiplier are three roundings in the loop and three here.  A normalised chain
    with an item factor other than 1 stays on the loop."""
    nobj = _noise_object(mods, normalize, 0.3, factor=factor)
    latent = {"samples": torch.zeros(4, 4, 8, 8), "batch_index": [1, 0, 5, 1]}
    rows, loop, made, at_rows, at_loop = _both_routes(mods, monkeypatch, nobj, latent)
    assert (made[0] is not None) == taken
    assert torch.equal(rows, loop) and at_rows == at_loop == 4 * 2 * 6


def test_launches_do_not_grow_with_the_indices(mods, monkeypatch, hl):
    """The row route: ONE library launch for a normalised chain -- lattices, statistics, decision, final values and the multiplier --
    whatever the indices; at most three for an unnormalised one (a rounding per multiplier other than 1).  The loop: three launches or
    more per index up to the largest."""
    def traced(nobj, inds, rows_route):
        noise = mods[0]
        latent = {"samples": torch.zeros(len(inds), 4, 8, 8), "batch_index": inds}
        with monkeypatch.context() as m:
            if not rows_route:
                m.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", lambda self, *a, **k: None)
            return _traced(hl, lambda: nobj.generate_noise(latent))

    loops = []
    for inds in ([2], [3, 3, 0, 7, 1]):
        assert traced(_noise_object(mods, True, 1.0), inds, True) == ["sonar_perlin_rows_f32"]
        assert traced(_noise_object(mods, True, 0.5), inds, True) == ["sonar_perlin_rows_f32"]
        assert traced(_noise_object(mods, False, 0.5, factor=0.7), inds, True) == [
            "sonar_perlin_rows_f32", "sonar_scale_noise_f32", "sonar_scale_noise_f32"]
        loops.append(len(traced(_noise_object(mods, True, 0.5), inds, False)))
        assert loops[-1] >= 2 * (max(inds) + 1)
    assert loops[1] > loops[0]
