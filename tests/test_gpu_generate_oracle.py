"""Generate mode (device draws, cpu=False) against its stream contract (-m gpu): every kernel value compared with
oracle/device_streams.py, the numpy restatement of INTEGRATION.md 3b -- at the sizes, element offsets, seeds and stream ids where a
lane, tile, stream word or conversion could be wrong.  A mapping error shows as an O(1) difference; the bounds below only absorb the
hardware transcendentals (v_log / v_sqrt / v_sin / v_cos, fp32) against fp64.

Measured on an MI355X, max |kernel - fp64| / (1 + |z|) over every case of the file (SONAR_ORACLE_ERRORS=<file> writes them out):
  Box-Muller normals: fill 1.96e-7, normalised 1.87e-7, look-ahead 1.28e-7, accumulating 2.29e-7 ... bound NORMAL_TOL = 1e-6
  unit complex normals (spectrum draws) 1.42e-7 ..................................................... bound SPECTRUM_TOL = 1e-6
  Brownian z, per 1 + sum_k |c_k z_k|: burst family 1.71e-7, Philox family 1.67e-7 ................... bound BROWNIAN_TOL = 1e-6
  generated planes, of the peak: 2.1e-7 (normalised 2.5e-7) .......................................... bound PLANE_TOL = 2e-5
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-6     # per (1 + |z|); measured maxima in the module docstring
SPECTRUM_TOL = 1e-6
BROWNIAN_TOL = 1e-6
PLANE_TOL = 2e-5      # generated planes: of the peak |value| (the FFT's fp32 sums; fuzz_spectral.py uses 3e-5)

SEEDS = (0, 2**32 + 5, 2**64 - 1)
STREAMS = (0, 2**32 + 3, 2**47 + 1)
OFFSETS = (0, 1, 3, 4093, 7 * 4096 + 2)
SIZES = (1, 3, 4095, 4096, 4097, 3 * 4096 + 5)
CASES = [(n, OFFSETS[i % len(OFFSETS)], SEEDS[i % len(SEEDS)], STREAMS[(i // len(SEEDS)) % len(STREAMS)])
         for i, n in enumerate(SIZES * 2)] + [(512 * 4 * 128 * 128, 0, 2**32 + 5, 2**47 + 1)]


@pytest.fixture(scope="module")
def hl(pkg):
    lib = pkg.hip_lib
    lib.load()
    return lib


MEASURED: dict = {}  # family -> max error seen (written out when SONAR_ORACLE_ERRORS names a file: how the bounds were set)


@pytest.fixture(scope="module", autouse=True)
def _report_measured():
    yield
    import json
    import os

    path = os.environ.get("SONAR_ORACLE_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1)


def _seen(family, err):
    MEASURED[family] = max(MEASURED.get(family, 0.0), float(err))
    return err


def _st():
    return torch.cuda.current_stream().cuda_stream


def _view(n, misaligned):
    """A contiguous float32 device tensor of n elements, 16-byte aligned or at a 4-byte storage offset."""
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    return buf[1:n + 1] if misaligned else buf[:n]


def _rel_err(got, want):
    got = got.detach().cpu().double().numpy().reshape(-1) if isinstance(got, torch.Tensor) else np.asarray(got).reshape(-1)
    want = np.asarray(want).reshape(-1)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if want.size else 0.0


def test_stream_version_matches_the_oracle(hl):
    """Who changes generate-mode values bumps sonar_noise_stream_version() and restates the streams in oracle/device_streams.py."""
    assert hl.load().sonar_noise_stream_version() == ds.STREAM_VERSION


# ------------------------------------------------------------------------------------------------ flat fills
@pytest.mark.parametrize("n, off, seed, stream", CASES)
def test_uniform_fill_is_bit_exact(hl, n, off, seed, stream):
    out = _view(n, misaligned=n % 2 == 1)
    hl.philox_uniform(out.shape, "cuda", seed, stream, off, out=out)
    want = ds.uniform_fill(seed, stream, n, off)
    assert np.array_equal(out.cpu().numpy(), want)
    if n < 10**6:
        aff = (0.5, 2.0, 0.25)
        hl.philox_uniform(out.shape, "cuda", seed, stream, off, sub=aff[0], mul=aff[1], add=aff[2], out=out)
        want = ds.uniform_fill(seed, stream, n, off, *aff)
        ulp = np.spacing(np.abs(want).astype(np.float32))
        assert np.all(np.abs(out.cpu().numpy() - want) <= ulp)  # hipcc may contract (u - sub) * mul + add into an FMA


@pytest.mark.parametrize("n, off, seed, stream", CASES)
def test_normal_fill_against_fp64_box_muller(hl, n, off, seed, stream):
    out = _view(n, misaligned=n % 2 == 0)
    hl.philox_normal(out.shape, "cuda", seed, stream, off, out=out)
    assert _seen("normal", _rel_err(out, ds.normal_fill(seed, stream, n, off))) < NORMAL_TOL


@pytest.mark.parametrize("n, off, seed, stream, factor", [(4097, 3, 2**64 - 1, 2**32 + 3, 0.75), (3 * 4096 + 5, 4093, 0, 2**47 + 1, 1.0),
                                                         (4 * 64 * 64, 0, 2**32 + 5, 0, 1.3), (5, 1, 5, 7, 1.0)])
def test_normalised_fill_against_fp64(hl, n, off, seed, stream, factor):
    """sonar_philox_noise_f32 (draw + scale_noise, the tensor written once) against the oracle's scale_noise of the fp64 draws; with a
    mean shift the decision is forced (uniform draws)."""
    got = hl.philox_noise(False, (n,), "cuda", seed, stream, off, factor)
    want = orc.scale_noise(torch.from_numpy(ds.normal_fill(seed, stream, n, off)), factor, normalized=True).numpy()
    assert _seen("normalised", _rel_err(got, want)) < NORMAL_TOL * 2 * max(1.0, factor)
    got = hl.philox_noise(True, (n,), "cuda", seed, stream, off, factor, sub=0.25, mul=2.0, add=0.5)
    u = torch.from_numpy(ds.uniform_fill(seed, stream, n, off, 0.25, 2.0, 0.5).astype(np.float64))
    want = orc.scale_noise(u, factor, normalized=True).numpy()
    assert _seen("normalised_uniform", _rel_err(got, want)) < NORMAL_TOL * max(1.0, factor)


@pytest.mark.parametrize("uniform", [False, True])
def test_noise_ahead_against_fp64(hl, uniform):
    """sonar_philox_noise_ahead_f32: this call's values, and the statistics it leaves for the call that draws with the next stream id."""
    n, off, seed, stream, nxt, factor = 3 * 4096 + 5, 4093, 2**32 + 5, 2**32 + 3, 2**47 + 1, 0.8
    out = torch.empty(n, device="cuda")
    part, part_next = hl.new_partials("cuda"), hl.new_partials("cuda")
    aff = (0.25, 2.0, 0.5) if uniform else (0.0, 1.0, 0.0)
    rc = hl.load().sonar_philox_noise_ahead_f32(int(uniform), out.data_ptr(), n, seed, stream, off, *aff, factor, 2.5, part.data_ptr(), 0,
                                                nxt, part_next.data_ptr(), _st())
    assert rc == 0

    def draws(s):
        return ds.uniform_fill(seed, s, n, off, *aff).astype(np.float64) if uniform else ds.normal_fill(seed, s, n, off)

    want = orc.scale_noise(torch.from_numpy(draws(stream)), factor, normalized=True).numpy()
    assert _seen("ahead", _rel_err(out, want)) < NORMAL_TOL * 2
    tot = hl.stats_finalize(part_next, n).cpu().double().numpy()
    nx = draws(nxt)
    assert abs(tot[0] - nx.sum()) < 1e-5 * np.abs(nx).sum() and abs(tot[1] - (nx * nx).sum()) < 1e-5 * (nx * nx).sum()


def test_normal_acc_against_fp64(hl):
    n, off, seed, stream = 4 * 4096 + 3, 1, 2**64 - 1, 2**47 + 1
    y0 = torch.randn(n, generator=torch.Generator().manual_seed(3))
    y = y0.cuda()
    hl.philox_normal_acc_(y, 0.5, -1.5, seed, stream, off)
    want = y0.double().numpy() * 0.5 + ds.normal_fill(seed, stream, n, off) * -1.5
    assert _seen("normal_acc", _rel_err(y, want)) < NORMAL_TOL * 2


# ------------------------------------------------------------------------------------------------ spectrum draws and generated planes
SPECTRUM_CASES = [((8, H, W), 0) for H, W in ds.FIXED_PLANES] + [
    ((2, 4, 128, 128), 4), ((2, 4, 64, 64), 20), ((3, 3, 32, 32), 1), ((1, 3, 64, 128), 5), ((2, 3, 16, 16), 0),
    ((1, 4, 104, 152), 0), ((2, 3, 104, 152), 5), ((1, 3, 96, 168), 1), ((1, 4, 256, 256), 0), ((1, 3, 256, 256), 1)]


@pytest.mark.parametrize("shape, plane_offset", SPECTRUM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_spectrum_draws_against_the_oracle(hl, shape, plane_offset):
    H, W = shape[-2:]
    seed, stream = 2**64 - 1, 2**32 + 3
    group = hl.rng_group_for(shape)
    planes = int(np.prod(shape[:-2]))
    z = hl.power_spectrum(shape, "cuda", seed=seed, stream_id=stream, plane_offset=plane_offset).cpu().numpy().reshape(planes, H, W // 2 + 1)
    want = ds.spectrum_draws(seed, stream, planes, H, W, plane_offset, group, hl.power_plane_kind(H, W))
    err = np.abs(z.astype(np.complex128) - want) / (1.0 + np.abs(want))
    assert _seen("spectrum", err.max()) < SPECTRUM_TOL


def _irfft2_ortho(zf, H, W):
    return np.fft.irfft2(zf, s=(H, W), norm="ortho")  # (drops the imaginary parts of the DC and Nyquist columns, like the kernels)


@pytest.mark.parametrize("shape, pipeline", [((2, 4, 128, 128), 1), ((2, 4, 128, 128), 0), ((1, 4, 64, 64), 1), ((1, 4, 104, 152), 1),
                                             ((1, 3, 256, 256), 1)])
def test_generated_planes_against_fp64_irfft2(hl, shape, pipeline):
    """power_irfft2(None, filt) (the headline kernel at 128 x 128) and power_noise (normalised, factor 0.7) against an fp64 irfft2 of the
    oracle spectrum times the filter."""
    H, W = shape[-2:]
    seed, stream, plane_offset = 2**32 + 5, 2**47 + 1, 4 if shape[1] % 4 == 0 else 1
    planes = int(np.prod(shape[:-2]))
    g = torch.Generator().manual_seed(H * W)
    filt = torch.rand(H, W // 2 + 1, generator=g) * 2.0 - 0.5  # any sign
    lib = hl.load()
    before = lib.sonar_power_pipeline(pipeline)
    try:
        got = hl.power_irfft2(None, filt.cuda(), shape, seed=seed, stream_id=stream, plane_offset=plane_offset).cpu().double().numpy()
        got_n = hl.power_noise(filt.cuda(), shape, seed=seed, stream_id=stream, plane_offset=plane_offset, factor=0.7).cpu().double().numpy()
    finally:
        lib.sonar_power_pipeline(before)
    zf = ds.spectrum_draws(seed, stream, planes, H, W, plane_offset, hl.rng_group_for(shape), hl.power_plane_kind(H, W)) * filt.double().numpy()
    want = _irfft2_ortho(zf, H, W).reshape(shape)
    assert _seen("plane", np.max(np.abs(got - want)) / np.max(np.abs(want))) < PLANE_TOL
    want_n = orc.scale_noise(torch.from_numpy(want.copy()), 0.7, normalized=True).numpy()
    assert _seen("plane_normalised", np.max(np.abs(got_n - want_n)) / np.max(np.abs(want_n))) < PLANE_TOL


# ------------------------------------------------------------------------------------------------ Brownian z(node, e), both families
BROWNIAN_CASES = [
    # (latent shape, batch, elem_offset in latents, nodes, coefs, latent seeds)
    ((4, 64, 64), 2, 0, [0], [1.0], None),
    ((4, 64, 64), 2, 1, [5], [-0.5], None),                                            # the NEG path, a shard
    ((4, 64, 64), 3, 2, [0, 1, 2**40 + 7, 6, 13], [0.7, -0.2, 0.05, -1.1, 0.4], None),  # >= 4 nodes: the 512-thread block
    ((4, 30, 30), 2, 0, [0], [1.0], None),
    ((4, 30, 30), 3, 1, [3, 9, 2**40 + 1, 4], [0.5, -0.25, 1.5, -0.8], None),
    ((4, 64, 64), 2, 0, [0, 3], [0.6, -0.9], [11, 2**64 - 1]),                          # per-latent seeds: the Philox family
]


def _brownian_want(seed, shape, batch, off_latents, nodes, coefs, latent_seeds):
    latent = int(np.prod(shape))
    n, off = batch * latent, off_latents * latent
    z = ds.brownian_z(seed, nodes, n, off, latent, latent_seeds)
    return np.asarray(coefs) @ z, (np.abs(np.asarray(coefs)[:, None] * z)).sum(axis=0), n, off, latent


@pytest.mark.parametrize("case", BROWNIAN_CASES, ids=range(len(BROWNIAN_CASES)))
def test_brownian_against_the_oracle(hl, case):
    shape, batch, off_l, nodes, coefs, lseeds = case
    seed = 2**32 + 5
    want, mag, n, off, latent = _brownian_want(seed, shape, batch, off_l, nodes, coefs, lseeds)
    ls = None if lseeds is None else torch.tensor([s - 2**64 if s >= 2**63 else s for s in lseeds], dtype=torch.int64, device="cuda")
    got = hl.brownian((batch, *shape), "cuda", nodes, coefs, seed, off, latent_seeds=ls).cpu().double().numpy().reshape(-1)
    assert _seen("brownian_" + ds.brownian_family(n, off, latent, lseeds), np.max(np.abs(got - want) / (1.0 + mag))) < BROWNIAN_TOL
    assert ds.brownian_family(n, off, latent, lseeds) == ("burst" if lseeds is None and latent % 4096 == 0 else "philox")


@pytest.mark.parametrize("shape", [(4, 64, 64), (4, 30, 30)])
def test_brownian_point_with_misaligned_buffers_keeps_its_family(hl, shape):
    """sonar_brownian_point_f32 with out / w_out / prev at a 4-byte storage offset: the values of the aligned call (the family is a function
    of the shape and seed kind), never the other family's."""
    batch, seed, nodes, coefs = 2, 7, [0, 1, 2, 3], [0.9, -0.4, 0.3, -0.6]
    latent = int(np.prod(shape))
    n = batch * latent
    want, mag, *_ = _brownian_want(seed, shape, batch, 0, nodes, coefs, None)
    prev0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    lib, st = hl.load(), _st()
    ids = (C.c_uint64 * 4)(*nodes)
    cf = (C.c_float * 4)(*coefs)
    res = {}
    for mis in (False, True):
        out, w, prev = _view(n, mis), _view(n, mis), _view(n, mis)
        prev.copy_(prev0)
        rc = lib.sonar_brownian_point_f32(out.data_ptr(), w.data_ptr(), prev.data_ptr(), 1.5, n, 0, ids, cf, 4, seed, None, latent, st)
        assert rc == 0
        res[mis] = (out.cpu(), w.cpu())
        assert np.max(np.abs(w.cpu().double().numpy() - want) / (1.0 + mag)) < BROWNIAN_TOL, f"misaligned={mis}: not the {ds.brownian_family(n, 0, latent)} family"
        assert np.max(np.abs(out.cpu().double().numpy() - 1.5 * (want - prev0.double().numpy())) / (1.0 + mag)) < 3 * BROWNIAN_TOL
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])
