"""Row-keyed fills (-m gpu): ``sonar_philox_rows_f32`` against the per-call kernels it stands in for (bit for bit), against the host
statement of one row (tests/noise_rows_refs.py), at a normalisation threshold, at its edges; and ``CustomNOISE.generate_noise`` with
``batch_index`` through it against the per-index loop (bit for bit), with the launches counted.

Tolerances against the fp64 refs are those of tests/test_gpu_generate_oracle.py for the same fills followed by the normalisation:
NORMAL_TOL * 2 * max(1, factor) per (1 + |value|) for Box-Muller normals, NORMAL_TOL * max(1, factor) for uniform draws."""
import importlib

import numpy as np
import pytest
import torch

from tests import noise_rows_refs as refs

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-6  # tests/test_gpu_generate_oracle.py
NPART = 1024
INNERS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4 * 8 * 8, 1023 * 3, NPART * 4 + 1)
ROWS = (1, 2, 7, 300)  # 300: more rows than compute units
SEEDS = (0, 2**63, 2**64 - 1, 12345, 12345, 2**32 + 5, 7, 2**63 - 1, 99)  # (two equal seeds: identical rows)
STREAM = 2**32 + 3
AFFINE = dict(sub=0.25, mul=2.0, add=0.5)
FACTORS = (1.0, 0.37)
NONE, SCALE_NOISE, FUSED = refs.NONE, refs.SCALE_NOISE, refs.FUSED


@pytest.fixture(scope="module")
def hl(pkg):
    pkg.hip_lib.load()
    return pkg.hip_lib


def _same(a, b):
    """torch.equal with equal_nan=True."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _row_seeds(rows):
    return [SEEDS[r % len(SEEDS)] for r in range(rows)]


def _loop_row(hl, uniform, seed, stream, inner, factor, mode):
    """One row as the per-call kernels give it, on a tensor of its own."""
    aff = AFFINE if uniform else {}
    if mode == FUSED:
        return hl.philox_noise(uniform, (inner,), "cuda", seed, stream, 0, factor, **aff)
    partials = hl.new_partials("cuda") if mode == SCALE_NOISE else None
    fill = hl.philox_uniform if uniform else hl.philox_normal
    x = fill((inner,), "cuda", seed, stream, 0, partials=partials, **aff)
    return hl.scale_noise_(x, factor, mode == SCALE_NOISE, partials)


def _modes(uniform, factor):
    # philox_noise's two-pass form is what FUSED restates; N(0,1) with factor 1 takes its one-pass route (the SCALE_NOISE sequence) instead
    return (NONE, SCALE_NOISE, FUSED) if uniform or factor != 1.0 else (NONE, SCALE_NOISE)


@pytest.mark.parametrize("uniform", [False, True], ids=["normal", "uniform"])
@pytest.mark.parametrize("inner", INNERS)
def test_rows_are_the_per_call_kernels_bits(hl, inner, uniform):
    """Every (rows, normalisation, factor) of the grid at this row length; the reference rows are computed once per distinct seed."""
    aff = AFFINE if uniform else {}
    for factor in FACTORS:
        for mode in _modes(uniform, factor):
            want = {seed: _loop_row(hl, uniform, seed, STREAM, inner, factor, mode) for seed in set(SEEDS)}
            for rows in ROWS:
                seeds = _row_seeds(rows)
                got = hl.philox_rows(uniform, (rows, inner), "cuda", seeds, STREAM, factor, mode, **aff)
                for r in (range(rows) if rows <= 7 else (0, 1, 2, 8, 150, 151, 298, 299)):
                    assert _same(got[r], want[seeds[r]]), (inner, uniform, factor, mode, rows, r)
                if rows == 300:  # every row, through the seeds' period
                    ref = torch.stack([want[s] for s in SEEDS])
                    assert _same(got[:297].view(33, len(SEEDS), inner), ref.expand(33, -1, -1))
                if rows >= 5:
                    assert _same(got[3], got[4])  # equal seeds
    if inner > 1:
        assert not torch.isnan(got).any()


def test_row_streams_and_device_keys(hl):
    """``row_streams`` is added to the stream id per row; device tensors (int64 bit patterns / uint64) are taken as they are."""
    inner, rows = 257, 5
    seeds, offs = [3, 2**64 - 1, 3, 3, 2**63], [0, 5, 1, 2**40, 2]
    want = torch.stack([_loop_row(hl, False, s, (STREAM + o) & (2**64 - 1), inner, 1.0, SCALE_NOISE) for s, o in zip(seeds, offs)])
    assert _same(hl.philox_rows(False, (rows, inner), "cuda", seeds, STREAM, 1.0, True, row_streams=offs), want)
    as_i64 = lambda v: torch.tensor([x - 2**64 if x >= 2**63 else x for x in v], dtype=torch.int64, device="cuda")  # noqa: E731
    assert _same(hl.philox_rows(False, (rows, inner), "cuda", as_i64(seeds), STREAM, 1.0, True, row_streams=as_i64(offs)), want)
    assert _same(hl.philox_rows(False, (rows, inner), "cuda", as_i64(seeds).view(torch.uint64), STREAM, 1.0, True, row_streams=offs), want)


@pytest.mark.parametrize("uniform", [False, True], ids=["normal", "uniform"])
@pytest.mark.parametrize("inner", [257, 4 * 8 * 8, 1023 * 3, NPART * 4 + 1])
def test_rows_against_the_host_statement(hl, inner, uniform):
    aff = AFFINE if uniform else {}
    seeds = [0, 2**64 - 1, 2**32 + 5]
    for factor in FACTORS:
        tol = NORMAL_TOL * (1 if uniform else 2) * max(1.0, factor)
        for mode in _modes(uniform, factor):
            got = hl.philox_rows(uniform, (len(seeds), inner), "cuda", seeds, STREAM, factor, mode, **aff).cpu().double().numpy()
            for r, seed in enumerate(seeds):
                seen = {}
                want = refs.row(uniform, seed, STREAM, inner, factor, mode, decisions=seen, **aff)
                if mode != NONE:  # (a statistic within rounding of its threshold would be the device's to decide: none of these rows)
                    assert min(abs(abs(seen["mean"]) - seen["threshold"]), abs(abs(1 - seen["std"]) - seen["threshold"])) > 1e-5
                err = float(np.max(np.abs(got[r] - want) / (1.0 + np.abs(want))))
                print(f"inner {inner} uniform {uniform} factor {factor} mode {mode} seed {seed}: {err:.3e} (bound {tol:.1e})")
                assert err < tol


# Seeds of N(0,1) rows of 256 elements (stream id 11) whose |mean| lies within 1e-3, relative, of the threshold 2.5 / sqrt(256), below
# and above it: found on the host by walking the seeds 0 .. 2^16 - 1 through noise_rows_refs.row_draw (14 seeds qualify; these two are the
# nearest on each side, 2.0e-4 below and 1.8e-4 above, with a std well inside its own threshold).  The test checks them again.
EDGE_STREAM, EDGE_INNER = 11, 256
EDGE_SEEDS = {"below": 40291, "above": 64854}


@pytest.mark.parametrize("side", ["below", "above"])
def test_a_mean_at_its_threshold_takes_the_loops_branch(hl, side):
    seed = EDGE_SEEDS[side]
    mean, sd, thr = refs.row_moments(refs.row_draw(False, seed, EDGE_STREAM, EDGE_INNER))
    rel = (abs(mean) - thr) / thr
    print(f"seed {seed}: |mean| = {abs(mean):.9f}, threshold {thr:.9f}, relative distance {rel:+.3e}, std {sd:.6f}")
    assert abs(rel) < 1e-3 and (rel < 0) == (side == "below")
    seeds = [5, seed, 6]
    got = hl.philox_rows(False, (3, EDGE_INNER), "cuda", seeds, EDGE_STREAM, 1.0, True)
    want = _loop_row(hl, False, seed, EDGE_STREAM, EDGE_INNER, 1.0, SCALE_NOISE)
    raw = hl.philox_normal((EDGE_INNER,), "cuda", seed, EDGE_STREAM, 0)
    assert _same(got[1], want)
    assert torch.equal(want, raw) == (side == "below")  # the existing pair subtracts the mean above the threshold only: so does the row


def test_nothing_is_written_outside_the_rows(hl):
    for rows, inner, lead in ((7, 65, 0), (7, 65, 1), (3, 4 * 4096 + 3, 3), (2, 256, 2)):
        n = rows * inner
        buf = torch.full((n + 64,), float("nan"), device="cuda")
        out = buf[16 + lead:16 + lead + n].view(rows, inner)  # lead: the first row itself off a 16-byte boundary
        hl.philox_rows(True, (rows, inner), "cuda", _row_seeds(rows), STREAM, 0.37, True, out=out, **AFFINE)
        assert not out.isnan().any()
        assert buf[:16 + lead].isnan().all() and buf[16 + lead + n:].isnan().all()
        want = torch.stack([_loop_row(hl, True, s, STREAM, inner, 0.37, SCALE_NOISE) for s in _row_seeds(rows)])
        assert _same(out, want)


def test_refusals_launch_nothing(hl):
    lib = hl.load()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((4, 64), float("nan"), device="cuda")
    seeds = torch.zeros(4, dtype=torch.int64, device="cuda")
    limit = lib.sonar_philox_rows_max_inner()

    def call(rows=4, inner=64, row_seed=seeds.data_ptr(), normalized=1):
        return lib.sonar_philox_rows_f32(out.data_ptr(), rows, inner, row_seed, None, 0, 5, 0.0, 1.0, 0.0, 1.0, normalized, 2.5, st)

    assert call(rows=-1) == hl.ERR_UNSUPPORTED and call(inner=0) == hl.ERR_UNSUPPORTED and call(inner=-1) == hl.ERR_UNSUPPORTED
    assert call(inner=limit + 1) == hl.ERR_UNSUPPORTED and call(row_seed=None) == hl.ERR_UNSUPPORTED
    assert call(normalized=3) == hl.ERR_ARG
    assert call(rows=0) == 0 and call(rows=0, row_seed=None) == 0
    torch.cuda.synchronize()
    assert out.isnan().all()
    with pytest.raises(hl.SonarHipError):
        hl.philox_rows(False, (4, 64), "cuda", [1, 2, 3], 5, 1.0, True, out=out)
    assert out.isnan().all()
    assert call() == 0 and not out.isnan().any()


# ------------------------------------------------------------------------------------------------ CustomNOISE.generate_noise
@pytest.fixture(scope="module")
def mods(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise"), importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


def _noise_object(mods, kind, normalize, multiplier, factor=1.0, seed=1234):
    noise, reg = mods
    chain = noise.CustomNoiseChain([noise.CustomNoiseItem(factor, noise_type=getattr(noise.NoiseType, kind))])
    return reg.CustomNOISE(chain, seed, cpu_noise=False, normalize=normalize, multiplier=multiplier)


def _both_routes(mods, monkeypatch, nobj, latent):
    """(the row route's result, the loop's, the device generator's position after each)."""
    noise = mods[0]
    made = []
    real = noise.CustomNoiseChain.make_row_seeded_sampler

    def spy(self, *a, **k):
        made.append(real(self, *a, **k))
        return made[-1]

    with monkeypatch.context() as m:
        m.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", spy)
        rows = nobj.generate_noise(latent)
    at_rows = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
    with monkeypatch.context() as m:
        m.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", lambda self, *a, **k: None)
        loop = nobj.generate_noise(latent)
    at_loop = torch.cuda.default_generators[torch.cuda.current_device()].get_offset()
    return rows, loop, made, at_rows, at_loop


@pytest.mark.parametrize("shape", [(5, 4, 8, 8), (3, 16, 2, 6, 6)], ids=["4d", "5d"])
@pytest.mark.parametrize("inds", [[0, 1, 2, 3, 4], [3, 3, 0, 7, 1], [2]], ids=["all", "mixed", "one"])
@pytest.mark.parametrize("kind", ["GAUSSIAN", "UNIFORM"])
def test_batch_index_is_the_loops_result(mods, monkeypatch, shape, inds, kind):
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        for normalize in (True, False):
            for multiplier in (1.0, 0.5):
                nobj = _noise_object(mods, kind, normalize, multiplier)
                latent = {"samples": torch.zeros(shape, dtype=dtype), "batch_index": inds}
                rows, loop, made, at_rows, at_loop = _both_routes(mods, monkeypatch, nobj, latent)
                assert len(made) == 1 and made[0] is not None, "the row route was not taken"
                assert rows.dtype == dtype and rows.device.type == "cpu" and tuple(rows.shape) == (len(inds), *shape[1:])
                assert torch.equal(rows, loop), (dtype, normalize, multiplier)
                assert at_rows == at_loop == 4 * (max(inds) + 1)  # later device draws continue where the loop would leave them
                assert rows.float().abs().max() > 0.1


@pytest.mark.parametrize("factor, normalize, taken", [(0.5, False, True), (-1.0, False, True), (2.0, False, True), (0.5, True, False)])
def test_item_factors_fold_or_stay_on_the_loop(mods, monkeypatch, factor, normalize, taken):
    """Unnormalised chains: item factor, chain factor and multiplier are three roundings in the loop and three here.  A normalised chain
    with an item factor other than 1 normalises from a separate statistics sweep: it keeps the loop."""
    nobj = _noise_object(mods, "GAUSSIAN", normalize, 0.3, factor=factor)
    latent = {"samples": torch.zeros(4, 4, 8, 8), "batch_index": [1, 0, 5, 1]}
    rows, loop, made, at_rows, at_loop = _both_routes(mods, monkeypatch, nobj, latent)
    assert (made[0] is not None) == taken
    assert torch.equal(rows, loop) and at_rows == at_loop


def test_launches_do_not_grow_with_the_indices(mods, monkeypatch, hl):
    """The row route: ONE library launch for a normalised chain (the draw with its normalisation and the multiplier), whatever the number
    of indices; at most three for an unnormalised one (a rounding per multiplier other than 1).  The loop: a launch or more per index up
    to the largest."""
    def traced(nobj, latent, rows_route):
        noise = mods[0]
        names = []
        rec = hl._Recorder(hl.load_raw())
        rec.on_call = lambda name, args, rc: names.append(name) if name not in hl._HOST_QUERIES else None
        with monkeypatch.context() as m:
            if not rows_route:
                m.setattr(noise.CustomNoiseChain, "make_row_seeded_sampler", lambda self, *a, **k: None)
            hl._recorder = rec
            try:
                nobj.generate_noise(latent)
            finally:
                hl._recorder = None
        return names

    for count in (2, 64):
        latent = {"samples": torch.zeros(count, 4, 8, 8), "batch_index": list(range(count))}
        assert traced(_noise_object(mods, "GAUSSIAN", True, 0.5), latent, True) == ["sonar_philox_rows_f32"]
        assert traced(_noise_object(mods, "UNIFORM", True, 1.0), latent, True) == ["sonar_philox_rows_f32"]
        assert traced(_noise_object(mods, "GAUSSIAN", False, 0.5, factor=0.7), latent, True) == [
            "sonar_philox_rows_f32", "sonar_scale_noise_f32", "sonar_scale_noise_f32"]
        assert len(traced(_noise_object(mods, "GAUSSIAN", True, 0.5), latent, False)) >= count
