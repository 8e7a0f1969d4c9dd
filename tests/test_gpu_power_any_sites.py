"""Every call site of the general-size power-noise plane kernel against an fp64 DFT (-m gpu).

tests/power_any_sites.SWEEP holds a plane size for every (family, axis, pass, codelet length | direct | absent) site, every form of
the inverse rows' first pass and both workgroup sizes, as the library plans them (tests/test_power_any_sites_cpu.py holds the list to
that).  At each size every mode of the kernel -- replay of a supplied spectrum, forward + filter + inverse, generate, generate +
normalise, each with and without statistics -- is compared with numpy in float64 on the exact fp32 inputs.  The filter has no symmetry
in ky and its kx = 0 and kx = W/2 columns are scaled apart, so every bin matters and no mirrored index can hide; a wrong twiddle or
row-batch split at one site is an O(1) difference at the sizes routed there.

Bounds (the project's): PLANE_TOL = 2e-5 of the reference's peak for planes, GEN_VS_REPLAY_ATOL = 2e-6 for generated planes against the
device replay of their own dumped spectrum, SPECTRUM_TOL = 1e-6 per 1 + |z| for the dump against oracle/device_streams.py.

Measured on an MI355X over SWEEP (SONAR_ORACLE_ERRORS=<file> writes the maxima out per check, family and pass kinds), the largest
|kernel - fp64| of the peak over replay, forward + inverse, unit filter, generate and generate + normalise; nothing came near the bound:
  by family                 small 5.0e-7 (4 x 618)       all 4.1e-7 (14 x 354)        buckets 2.8e-7 (80 x 192)
  by an axis' pass kinds    codelet/codelet 4.0e-7 (18 x 1010)   codelet/direct 5.0e-7 (4 x 618)   direct/direct 3.7e-7 (14 x 828)
                            single codelet pass 5.0e-7 (4 x 618) single direct pass 1.7e-7 (228 x 2)
  generate against the device replay of its dump, absolute: 1.67e-6 (10 x 902; 1.43e-6 at 132 x 264), buckets 9.5e-7 ... bound 2e-6
  dumped spectrum against the stream contract, per 1 + |z|: 1.25e-7 (18 x 1010)
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc
from tests import power_any_sites as S

pytestmark = pytest.mark.gpu

PLANE_TOL = 2e-5            # of the reference's peak |value| (tests/test_gpu_generate_oracle.py; FFT_ATOL of tests/test_gpu_kernels.py)
GEN_VS_REPLAY_ATOL = 2e-6   # tests/test_gpu_kernels.py: two roundings' difference per spectrum value
SPECTRUM_TOL = 1e-6         # tests/test_gpu_generate_oracle.py
SEED, STREAM, FACTOR = 2**32 + 5, 2**47 + 1, 0.6

IDS = [f"{h}x{w}" for h, w in S.SWEEP]


@pytest.fixture(scope="module")
def hl(pkg):
    lib = pkg.hip_lib
    lib.load()
    return lib


MEASURED: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report_measured():
    yield
    path = os.environ.get("SONAR_ORACLE_ERRORS")
    if path:
        seen = {}
        if os.path.exists(path):  # (tests/test_gpu_generate_oracle.py writes the same file)
            with open(path) as f:
                seen = json.load(f)
        seen.update(MEASURED)
        with open(path, "w") as f:
            json.dump(seen, f, indent=1)


def _plan(hl, hw):
    p = S.plan(hl.load(), *hw)
    assert p is not None and hl.load().sonar_power_plane_kind(*hw) == 2
    return p


def _seen(hl, hw, what, err):
    p = _plan(hl, hw)
    key = f"power_any {what} | {S.FAMILY_NAMES[p['family']]} | {S.pass_kinds(p)}"
    if float(err) > MEASURED.get(key, (-1.0,))[0]:
        MEASURED[key] = (float(err), f"{hw[0]}x{hw[1]}")
    return float(err)


def _inputs(hw):
    """(rng, filter [H, S] fp32): rand + 0.5 with the kx = 0 and kx = M columns scaled apart."""
    h, w = hw
    rng = np.random.default_rng(1000 * h + w)
    filt = (rng.random((h, w // 2 + 1)) + 0.5).astype(np.float32)
    filt[:, 0] *= np.float32(1.25)
    filt[:, -1] *= np.float32(0.75)
    return rng, filt


def _irfft2(zf, hw):
    return np.fft.irfft2(zf, s=hw, norm="ortho")  # (drops the imaginary parts of the kx = 0 and kx = M columns, like the kernels)


def _peak_err(got, want):
    return float(np.max(np.abs(got.detach().cpu().double().numpy() - want)) / np.max(np.abs(want)))


def _check_partials(hl, part, out):
    """The statistics a launch leaves against fp64 sums of what it wrote: the bound of test_power_irfft2_general_size_planes, for the
    sum in the same form (1e-5 of the sum of magnitudes -- a thread adds at most a few hundred fp32 values before it hands them to fp64)."""
    tot = hl.stats_finalize(part, out.numel()).cpu()
    o = out.detach().cpu().double()
    assert abs(tot[1].item() - (o * o).sum().item()) < 1e-5 * tot[1].item() + 1e-9
    assert abs(tot[0].item() - o.sum().item()) < 1e-5 * o.abs().sum().item() + 1e-9


@pytest.mark.parametrize("hw", S.SWEEP, ids=IDS)
def test_replay_against_fp64(hl, hw):
    h, w = hw
    rng, filt = _inputs(hw)
    shape = (3, 2, h, w)
    z = (rng.standard_normal((3, 2, h, w // 2 + 1)) + 1j * rng.standard_normal((3, 2, h, w // 2 + 1))).astype(np.complex64)
    want = _irfft2(z.astype(np.complex128) * filt.astype(np.float64), hw)
    zd, fd = torch.from_numpy(z).cuda(), torch.from_numpy(filt).cuda()
    part = hl.new_partials("cuda")
    got = hl.power_irfft2(zd, fd, shape)
    got_p = hl.power_irfft2(zd, fd, shape, partials=part)
    err = _seen(hl, hw, "replay", _peak_err(got, want))
    print(f"{h}x{w} replay {err:.3e} {_plan(hl, hw)}")
    assert err < PLANE_TOL
    assert torch.equal(got, got_p)
    _check_partials(hl, part, got_p)


@pytest.mark.parametrize("hw", S.SWEEP, ids=IDS)
def test_forward_filter_inverse_against_fp64(hl, hw):
    """sonar_spectral_filter_f32: the forward instantiation of every site, then the filter and the inverse."""
    h, w = hw
    rng, filt = _inputs(hw)
    x = rng.standard_normal((3, 2, h, w)).astype(np.float32)
    want = np.fft.irfft2(np.fft.rfft2(x.astype(np.float64)) * filt.astype(np.float64), s=hw)
    xd, fd = torch.from_numpy(x).cuda(), torch.from_numpy(filt).cuda()
    part = hl.new_partials("cuda")
    got = hl.spectral_filter(xd, fd)
    got_p = hl.spectral_filter(xd, fd, part)
    err = _seen(hl, hw, "forward+inverse", _peak_err(got, want))
    unit = _seen(hl, hw, "unit filter", _peak_err(hl.spectral_filter(xd, torch.ones_like(fd)), x.astype(np.float64)))
    print(f"{h}x{w} forward+inverse {err:.3e} unit filter {unit:.3e} {_plan(hl, hw)}")
    assert err < PLANE_TOL
    assert unit < PLANE_TOL
    assert torch.equal(got, got_p)
    _check_partials(hl, part, got_p)


@pytest.mark.parametrize("hw", S.SWEEP, ids=IDS)
def test_generate_against_fp64(hl, hw):
    """Generate mode: the fp64 inverse of the dumped spectrum times the filter; fused with the normalisation: that plane through the
    oracle's scale_noise (mean and std in float64, factor 0.6)."""
    h, w = hw
    _, filt = _inputs(hw)
    shape = (2, 4, h, w)
    fd = torch.from_numpy(filt).cuda()
    kw = dict(seed=SEED, stream_id=STREAM, plane_offset=8)
    z = hl.power_spectrum(shape, "cuda", **kw)
    want = _irfft2(z.cpu().numpy().astype(np.complex128) * filt.astype(np.float64), hw)
    part = hl.new_partials("cuda")
    got = hl.power_irfft2(None, fd, shape, **kw)
    got_p = hl.power_irfft2(None, fd, shape, partials=part, **kw)
    err = _seen(hl, hw, "generate", _peak_err(got, want))
    rep = _seen(hl, hw, "generate - replay", (got - hl.power_irfft2(z, fd, shape)).abs().max().item())
    want_n = orc.scale_noise(torch.from_numpy(want.copy()), FACTOR, normalized=True).numpy()
    norm = _seen(hl, hw, "generate normalised", _peak_err(hl.power_noise(fd, shape, factor=FACTOR, **kw), want_n))
    print(f"{h}x{w} generate {err:.3e} vs replay {rep:.3e} normalised {norm:.3e} {_plan(hl, hw)}")
    assert err < PLANE_TOL
    assert rep < GEN_VS_REPLAY_ATOL
    assert norm < PLANE_TOL
    assert torch.equal(got, got_p)
    _check_partials(hl, part, got_p)


def _walk_edges():
    """Sizes where draw_plane_dyn's (ky, kx) walk is at an edge: one and two interior columns, the longest row, two rows, 512 rows."""
    by_w = lambda w: min((hw for hw in S.SWEEP if hw[1] == w), key=lambda hw: hw[0])
    sizes = [by_w(2), by_w(4), max(S.SWEEP, key=lambda hw: hw[1]), max((hw for hw in S.SWEEP if hw[0] == 2), key=lambda hw: hw[1])]
    tall = [hw for hw in S.SWEEP if hw[0] == 512]
    sizes.append(min(tall, key=lambda hw: hw[1]) if tall else (512, 2))  # (512, 2): the smallest accepted plane of 512 rows
    return list(dict.fromkeys(sizes))


WALK_EDGES = _walk_edges()


@pytest.mark.parametrize("hw", WALK_EDGES, ids=[f"{h}x{w}" for h, w in WALK_EDGES])
def test_generate_units_and_groups_at_the_walk_edges(hl, hw):
    """Three channels (RNG group 1), 300 latents (more single-plane units than workgroups) and 530 latents (whole groups for the full
    rounds, single planes for the rest): the planes a small launch at the same offsets draws, bit for bit; the dumped spectrum is the
    stream contract's (oracle/device_streams.py)."""
    h, w = hw
    assert hl.load().sonar_power_plane_kind(h, w) == 2
    _, filt = _inputs(hw)
    fd = torch.from_numpy(filt).cuda()
    kw = dict(seed=SEED, stream_id=STREAM)
    three = hl.power_irfft2(None, fd, (3, 3, h, w), plane_offset=3, **kw)
    for latent in range(3):
        assert torch.equal(hl.power_irfft2(None, fd, (1, 3, h, w), plane_offset=3 + 3 * latent, **kw), three[latent:latent + 1]), latent
    for latents in (300, 530):
        big = hl.power_irfft2(None, fd, (latents, 4, h, w), **kw)
        for first, count in ((0, 2), (255, 2), (latents - 19, 2), (latents - 1, 1)):
            small = hl.power_irfft2(None, fd, (count, 4, h, w), plane_offset=4 * first, **kw)
            assert torch.equal(small, big[first:first + count]), (latents, first)
        del big
    for shape, off in (((2, 4, h, w), 8), ((2, 3, h, w), 5)):
        z = hl.power_spectrum(shape, "cuda", plane_offset=off, **kw).cpu().numpy().reshape(-1, h, w // 2 + 1)
        want = ds.spectrum_draws(SEED, STREAM, z.shape[0], h, w, off, hl.rng_group_for(shape), 2)
        err = np.abs(z.astype(np.complex128) - want) / (1.0 + np.abs(want))
        assert _seen(hl, hw, "spectrum", err.max()) < SPECTRUM_TOL
