"""Generate-mode Perlin noise against its stream contract (-m gpu): the lattice kernel, the four launch routes of perlin_generate_kernel
(aligned-fast, fast, vector, scalar) in their three modes, both word-to-value converters, the four normalisation instantiations, the
three geometries of the look-ahead kernel, the accumulating and chained forms and the Perlin item hosted by the pair, Brownian and
pyramid kernels -- every value compared with oracle/device_streams.py (perlin_lattice, perlin_values) in fp64.  Every case restates the
launcher's own conditions and asserts the route or geometry it is meant to reach before it compares values.

Bounds.  Raw values with a power-of-two divisor are the bits of float32_steps (Divider's promise).  Any other divisor: |kernel - fp64| <=
(1 + 0.5 max(tables, 1)) spacing32(M), M the largest of |u / d| and the running sums (one ulp for the division, half an ulp per add);
the build divides correctly rounded (DIVIDES_CORRECTLY_ROUNDED: observed on an MI355X), so those values too are float32_steps' bits.
Normalised values: NORMAL_TOL * 2 * max(1, factor) per (1 + |z|), as the normalised fills; folds: 2 * NORMAL_TOL per (1 + |want|);
statistics: 1e-5 of sum |x| and of sum x^2 (the fast route sums a tile's 64 values per lane in fp32: 64 * 2^-24 of them at most).

The lattice bound is the one measured number: the hardware v_sin / v_cos (revolutions) against fp64.  Measured on an MI355X, the largest
|kernel - perlin_lattice| / max(iters, 1) over every lattice case of this file (SONAR_ORACLE_ERRORS=<file> writes it out as
"perlin_lattice_per_iter"): 2.16e-7 (LATTICE_MEASURED: 4 x 64 x 64, subtract_b, one iteration; lerp 9.2e-8, inject 2.0e-7; nine iterations 1.12e-6 in all at most); the bound is four times that per iteration, below the 3e-6 per iteration
tests/test_gpu_kernels.py::test_perlin_lattice_kernel_against_a_host_replay_of_its_draws allows.
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc
from tests import pyramid_refs as R
from tests.test_gpu_generate_oracle import BROWNIAN_TOL, NORMAL_TOL, SEEDS, STREAMS
from tests.test_gpu_pyramid_oracle import FAMILY as PYRAMID_FAMILY, TOL as PYRAMID_TOL

pytestmark = pytest.mark.gpu

LATTICE_MEASURED = 2.16e-7                  # max |kernel - fp64| per iteration, MI355X (module docstring)
LATTICE_TOL = 4.0 * LATTICE_MEASURED        # per iteration
assert LATTICE_TOL <= 3e-6
DIVIDES_CORRECTLY_ROUNDED = True            # u01 / d for a divisor that is no power of two: IEEE division in this build
STATS_RTOL = 1e-5
TILE = ds.TILE_ELEMS
POW2 = (2.0, 0.5, 1.0, -4.0)
OTHER = (1.5, 3.0, -1.7)


@pytest.fixture(scope="module")
def hl(pkg):
    lib = pkg.hip_lib
    lib.load()
    _LIB.append(lib)
    return lib


_LIB: list = []  # the library of the `hl` fixture, for the cached helpers below


@pytest.fixture(scope="module")
def api(pkg, hl):
    import types

    mods = {m: importlib.import_module(f"comfyui_sonar_amd.py.{m}") for m in ("noise_generation", "noise")}
    return types.SimpleNamespace(**mods, hl=hl)


MEASURED: dict = {}  # family -> max error seen (merged into the file SONAR_ORACLE_ERRORS names: how the lattice bound was set)


@pytest.fixture(scope="module", autouse=True)
def _report_measured():
    yield
    import json
    import os

    path = os.environ.get("SONAR_ORACLE_ERRORS")
    if path:
        seen = json.load(open(path)) if os.path.exists(path) else {}
        seen.update(MEASURED)
        with open(path, "w") as f:
            json.dump(seen, f, indent=1)


def _seen(family, err):
    MEASURED[family] = max(MEASURED.get(family, 0.0), float(err))
    return err


def _st():
    return torch.cuda.current_stream().cuda_stream


def _keys(i):
    return SEEDS[i % len(SEEDS)], STREAMS[(i // len(SEEDS)) % len(STREAMS)]


def _np(t):
    return t.detach().cpu().double().numpy().reshape(-1)


def _view(shape, misaligned=False, fill=float("nan")):
    """A contiguous float32 device tensor, 16-byte aligned or at a 4-byte storage offset."""
    n = math.prod(shape)
    buf = torch.full((n + 4,), fill, device="cuda")
    v = (buf[1:n + 1] if misaligned else buf[:n]).view(shape)
    assert (v.data_ptr() % 16 != 0) == bool(misaligned)
    return v


# ------------------------------------------------------------------------------------------------ the launchers' conditions, restated
def _route(chw, tables, elem_offset, *tensors):
    """launch_perlin_generate: which perlin_generate_kernel a call gets (tensors: out, the term table when there is one, the running sum)."""
    vec = chw % 4 == 0 and elem_offset % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in tensors)
    fast = vec and tables == 1 and chw >= 256
    aligned = fast and chw % TILE == 0 and elem_offset % TILE == 0
    return "aligned" if aligned else "fast" if fast else "vector" if vec else "scalar"


def _tile_grid(hl, n, elem_offset):
    tiles = (elem_offset + n - 1) // TILE - elem_offset // TILE + 1
    return max(1, min(hl.NPART, (tiles + 3) // 4))


def _scale(values, factor, decisions=None):
    return orc.scale_noise(torch.from_numpy(np.array(values, dtype=np.float64)), factor, normalized=True, decisions=decisions).numpy()


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want))))


def _check_stats(hl, part, want):
    tot = hl.stats_finalize(part, want.size).cpu().double().numpy()
    assert abs(tot[0] - want.sum()) <= STATS_RTOL * np.abs(want).sum() and abs(tot[1] - (want * want).sum()) <= STATS_RTOL * (want * want).sum()


@functools.lru_cache(maxsize=None)
def _device_lattice(c, h, w, seed, stream, iters=2, blend="lerp"):
    """The device lattice [1, C, H, W] of a case (drawn once, shared, never written to)."""
    return _LIB[-1].perlin_lattice(iters, c, h, w, "cuda", blend, seed, stream)


def _terms_np(terms):
    return terms.detach().cpu().numpy().reshape(terms.shape[0], terms[0].numel() if terms.shape[0] else terms.shape[-1])


# ------------------------------------------------------------------------------------------------ the lattice
LATTICE_ITERS = (0, 1, 3, 4, 5, 9)
LATTICE_SHAPES = ((1, 1, 1), (2, 5, 7), (4, 64, 64))
LATTICE_CASES = [(iters, blend, shape, i) for i, (iters, blend, shape) in enumerate(
    (iters, blend, shape) for shape in LATTICE_SHAPES for blend in ds.PERLIN_BLENDS for iters in LATTICE_ITERS)]


@pytest.mark.parametrize("iters, blend, shape, i", LATTICE_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{b}-{it}" for it, b, s, _ in LATTICE_CASES])
def test_lattice_kernel_against_the_oracle(hl, iters, blend, shape, i):
    """sonar_perlin_lattice_f32 at the `iters % 4` edges of its word index and counter word, no iterations at all, all three blends; where
    the look-ahead entry point takes the shape (whole tiles per latent), its lattice blocks give the lattice kernel's bits."""
    C, H, W = shape
    seed, stream = _keys(i)
    got = hl.perlin_lattice(iters, C, H, W, "cuda", blend, seed, stream)
    want = ds.perlin_lattice(seed, stream, iters, C, H, W, blend)
    err = float(np.max(np.abs(_np(got) - want.reshape(-1))))
    print(f"lattice {shape} {blend} iters={iters}: max |kernel - fp64| = {err:.3e}")
    assert _seen("perlin_lattice_per_iter", err / max(iters, 1)) <= LATTICE_TOL
    if iters == 0:
        assert not got.any()
    chw = C * H * W
    if hl.load().sonar_perlin_noise_ahead_ok(1, chw, 0):
        terms = _device_lattice(C, H, W, 5, 7)   # (any table: the lattice blocks share the call's seed, nothing else)
        out, ahead = torch.empty((1, C, H, W), device="cuda"), torch.full_like(got, float("nan"))
        part = hl.new_partials("cuda")
        rc = hl.load().sonar_perlin_noise_ahead_f32(terms.data_ptr(), out.data_ptr(), 1, chw, 2.0, seed, 6, 0, 1.0, 2.5, part.data_ptr(), 0, 0, None, None,
                                                    ahead.data_ptr(), iters, C, H, W, hl.BLEND_IDS[blend], stream, _st())
        assert rc == 0 and torch.equal(ahead, got)
    else:
        assert chw % TILE != 0


# ------------------------------------------------------------------------------------------------ raw values (MODE 0)
# (name, route, B, (C, H, W), elem_offset, tables: "lattice" | 2 random | 0, divisors, misaligned (out, terms))
RAW_CASES = [
    ("aligned_3x4096", "aligned", 3, (1, 64, 64), 0, "lattice", (2.0, -1.7, 1.0), (0, 0)),
    ("aligned_2x16384_off", "aligned", 2, (4, 64, 64), TILE * 5, "lattice", (-4.0, 1.5, 0.5), (0, 0)),
    ("fast_5x63232_latent3", "fast", 5, (4, 104, 152), 3 * 63232, "lattice", (2.0, 1.5), (0, 0)),
    ("fast_3x256", "fast", 3, (1, 16, 16), 0, "lattice", (0.5, 3.0), (0, 0)),
    ("fast_3x260_wraps", "fast", 3, (1, 13, 20), 0, "lattice", (1.0, -1.7, 1.5), (0, 0)),
    ("fast_2x4100", "fast", 2, (1, 50, 82), 0, "lattice", (-4.0, 3.0), (0, 0)),
    ("vector_3x128", "vector", 3, (2, 8, 8), 0, "lattice", (2.0, 0.5, 1.5), (0, 0)),
    ("vector_7x4", "vector", 7, (1, 2, 2), 0, "lattice", (1.0, -4.0, 3.0), (0, 0)),
    ("vector_3x1280_two_tables", "vector", 3, (5, 16, 16), 64, 2, (3.0, -1.7, 2.0), (0, 0)),
    ("vector_3x1280_no_table", "vector", 3, (5, 16, 16), 64, 0, (1.5, 0.5), (0, 0)),
    ("scalar_3x105", "scalar", 3, (3, 5, 7), 0, "lattice", (2.0, 1.5, -4.0), (0, 0)),
    ("scalar_3x256_out_misaligned", "scalar", 3, (1, 16, 16), 0, "lattice", (2.0, -1.7), (1, 0)),
    ("scalar_3x256_offset_2", "scalar", 3, (1, 16, 16), 2, "lattice", (0.5, 3.0), (0, 0)),
    ("scalar_3x256_terms_misaligned", "scalar", 3, (1, 16, 16), 0, "lattice", (1.0, 1.5), (0, 1)),
]
assert all(any(d in c[6] for c in RAW_CASES if c[1] in ("fast", "aligned")) and any(d in c[6] for c in RAW_CASES if c[1] in ("vector", "scalar"))
           for d in POW2 + OTHER)


def _case_terms(kind, chw_shape, seed, stream, misaligned=False):
    c, h, w = chw_shape
    chw = c * h * w
    if kind == "lattice":
        t = _device_lattice(c, h, w, seed, (stream + 1) & (2**64 - 1)).view(1, chw)
    elif kind == 0:
        t = torch.empty((0, chw), device="cuda")
    else:
        t = torch.randn(kind, chw, generator=torch.Generator().manual_seed(chw)).cuda()
    if misaligned:
        m = _view(tuple(t.shape), True)
        m.copy_(t)
        t = m
    return t


def _check_raw(got, terms, seed, stream, chw, d, n, off, first=0, count=None, family="perlin_raw"):
    """Raw values of a call (or of a window of it) against the oracle: float32_steps' bits, and the derived bound against fp64."""
    tn = _terms_np(terms)
    want, steps = ds.perlin_values(seed, stream, tn, chw, d, n, off, first, count)
    got = got.detach().cpu().numpy().reshape(-1)
    assert got.shape == want.shape
    if ds.divisor_is_power_of_two(d):
        assert np.array_equal(got, steps())
        if tn.shape[0] == 1:
            assert np.array_equal(got, steps(fused=True))
    else:
        bound = ds.perlin_rounding_bound(seed, stream, tn, chw, d, n, off, first, count)
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound)
        _seen(family + "_division_mismatches", float(np.count_nonzero(got != steps())))
        if DIVIDES_CORRECTLY_ROUNDED:
            assert np.array_equal(got, steps())
    return want


@pytest.mark.parametrize("case", RAW_CASES, ids=[c[0] for c in RAW_CASES])
def test_raw_values_against_the_oracle(hl, case):
    """sonar_perlin_generate_f32 with and without statistics on each launch route, over the divisors of both converters."""
    name, route, B, shape, off, kind, divisors, (mis_out, mis_terms) = case
    chw, n = math.prod(shape), B * math.prod(shape)
    seed, stream = _keys(RAW_CASES.index(case))
    terms = _case_terms(kind, shape, seed, stream, mis_terms)
    for d in divisors:
        for stats in (False, True):
            out = _view((B, *shape), mis_out)
            assert _route(chw, terms.shape[0], off, out, terms if terms.shape[0] else None) == route
            part = hl.new_partials("cuda") if stats else None
            hl.perlin_generate((B, *shape), terms, d, seed, stream, off, partials=part, out=out)
            want = _check_raw(out, terms, seed, stream, chw, d, n, off)
            if stats:
                _check_stats(hl, part, want)


# ------------------------------------------------------------------------------------------------ normalised (MODE 1 + 2)
INV_SQRT12 = float(np.float32(1.0 / math.sqrt(12.0)))
# (instantiation (subtract, scale), table, divisor, factor); shapes: one aligned, one general (vector) route each
NORM_KINDS = {
    "subtract_scale": ((True, True), "lattice", 2.0, 0.7),
    "scale_only": ((False, True), -0.25, 2.0, 1.0),
    "subtract_only": ((True, False), 0.0, INV_SQRT12, 1.0),
    "neither": ((False, False), -math.sqrt(3.0), INV_SQRT12, 1.0),
}
NORM_SHAPES = {"aligned": (3, (1, 64, 64), 0), "vector": (24, (2, 8, 8), 0)}
NORM_KEYS = {  # (seed, stream) of a case: chosen on the host so that the oracle's decisions are clear of their thresholds (asserted below)
    ("neither", "aligned"): (5, 7), ("neither", "vector"): (5, 7),
}
NORM_CASES = [(k, r) for k in NORM_KINDS for r in NORM_SHAPES]


def _norm_case(kind, route):
    (sub, scale), table, d, factor = NORM_KINDS[kind]
    B, shape, off = NORM_SHAPES[route]
    seed, stream = NORM_KEYS.get((kind, route), _keys(NORM_CASES.index((kind, route))))
    return sub, scale, table, d, factor, B, shape, off, seed, stream


def _clear_decisions(values, factor, sub, scale):
    """The oracle's decisions are the intended ones, mean and std at least 25 % of the threshold away from it."""
    dec = {}
    want = _scale(values, factor, dec)
    thr = dec["threshold"]
    assert dec["sub"] == sub and dec["div"] == scale
    assert abs(abs(dec["mean"]) - thr) >= 0.25 * thr and abs(abs(1.0 - dec["std"]) - thr) >= 0.25 * thr, dec
    return want


@pytest.mark.parametrize("kind, route", NORM_CASES, ids=[f"{k}-{r}" for k, r in NORM_CASES])
def test_normalised_values_against_the_oracle(hl, kind, route):
    """sonar_perlin_noise_f32 (statistics pass + final pass) through each of the four with_norm_flags instantiations."""
    sub, scale, table, d, factor, B, shape, off, seed, stream = _norm_case(kind, route)
    chw, n = math.prod(shape), B * math.prod(shape)
    terms = _case_terms("lattice", shape, seed, stream) if table == "lattice" else torch.full((1, chw), float(table), device="cuda")
    assert _route(chw, 1, off, terms) == route
    raw, _ = ds.perlin_values(seed, stream, _terms_np(terms), chw, d, n, off)
    want = _clear_decisions(raw, factor, sub, scale)
    got = hl.perlin_noise((B, *shape), terms, d, seed, stream, off, factor)
    assert _seen("perlin_normalised", _rel(_np(got), want)) < NORMAL_TOL * 2 * max(1.0, factor)


# ------------------------------------------------------------------------------------------------ the look-ahead kernel
def _ahead(hl, terms, out, B, chw, d, seed, stream, off, factor, part, have, nxt, terms_next, part_next, lat_out=None, lat=(0, 0, 0, 0, 0, 0)):
    rc = hl.load().sonar_perlin_noise_ahead_f32(terms.data_ptr(), out.data_ptr(), B, chw, d, seed, stream, off, factor, 2.5, part.data_ptr(), have, nxt,
                                                None if terms_next is None else terms_next.data_ptr(),
                                                None if part_next is None else part_next.data_ptr(),
                                                None if lat_out is None else lat_out.data_ptr(), *lat, _st())
    assert rc == 0


@pytest.mark.parametrize("B, shape, d", [(1, (1, 64, 64), 2.0), (4, (4, 64, 64), 1.5)], ids=["1x4096", "4x16384"])
@pytest.mark.parametrize("with_next", [0, 1])
def test_look_ahead_against_the_oracle(hl, B, shape, d, with_next):
    """sonar_perlin_noise_ahead_f32 below the capped grid: the single block form (no next call) and the interleaved form, first without
    statistics left for it, then (second call) with the ones the first call left."""
    C, H, W = shape
    chw, n, factor = C * H * W, B * C * H * W, 0.9
    seed, s0, s1, s2 = 2**32 + 5, 2**32 + 3, 2**32 + 5, 2**32 + 7
    assert hl.load().sonar_perlin_noise_ahead_ok(B, chw, 0) == 1 and _route(chw, 1, 0) == "aligned"
    fused = bool(with_next) and _tile_grid(hl, n, 0) == hl.NPART
    assert not fused
    t0, t1 = _device_lattice(C, H, W, seed, s0 + 1).view(1, chw), _device_lattice(C, H, W, seed, s1 + 1).view(1, chw)
    out0, out1 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    p0, p1, p2 = hl.new_partials("cuda"), hl.new_partials("cuda"), hl.new_partials("cuda")
    lat_out = torch.full((C, H, W), float("nan"), device="cuda")
    _ahead(hl, t0, out0, B, chw, d, seed, s0, 0, factor, p0, 0, s1, t1 if with_next else None, p1 if with_next else None, lat_out,
           (3, C, H, W, hl.BLEND_IDS["inject"], s2 + 1))
    raw0, _ = ds.perlin_values(seed, s0, _terms_np(t0), chw, d, n)
    raw1, _ = ds.perlin_values(seed, s1, _terms_np(t1), chw, d, n)
    assert _seen("perlin_ahead", _rel(_np(out0), _scale(raw0, factor))) < NORMAL_TOL * 2
    lat_err = np.max(np.abs(_np(lat_out) - ds.perlin_lattice(seed, s2 + 1, 3, C, H, W, "inject").reshape(-1)))
    assert _seen("perlin_lattice_per_iter", lat_err / 3) <= LATTICE_TOL
    if with_next:
        _check_stats(hl, p1, raw1)
    # the call that follows: its statistics were left for it (have_stats = 1) or not
    _ahead(hl, t1, out1, B, chw, d, seed, s1, 0, factor, p1 if with_next else p2, with_next, s2, None, None)
    assert _seen("perlin_ahead", _rel(_np(out1), _scale(raw1, factor))) < NORMAL_TOL * 2


BIG_B, BIG_SHAPE, BIG_D = 4100, (1, 64, 64), 1.5
BIG_TILES = (0, 1, 1717, 2900, 4095, 4096, 4099)   # the ends, two interior ones, and the second trips of waves 0 and 3 of the capped grid


@functools.lru_cache(maxsize=None)
def _big_raw(seed, stream, terms_key):
    """fp64 raw values of the 4100-tile call for one stream (computed once, shared, never written to)."""
    terms = _BIG_TERMS[terms_key]
    raw, _ = ds.perlin_values(seed, stream, terms, TILE, BIG_D, BIG_B * TILE)
    raw.setflags(write=False)
    return raw


_BIG_TERMS: dict = {}


def _windows(t):
    return [(tile, t[tile * TILE:(tile + 1) * TILE]) for tile in BIG_TILES]


def test_capped_grid_and_the_fused_look_ahead_against_the_oracle(hl):
    """4100 latents of 4096 elements: 4100 tiles on 4096 waves -- the grid is capped at 1024 blocks, tiles 4096..4099 are the second trip of
    waves 0..3, and the look-ahead kernel runs its fused form (perlin_fast_tiles_pair).  perlin_generate, perlin_noise and the fused launch
    on windows of the oracle (a divisor that is no power of two); the fused launch's whole tensor is perlin_noise's, bit for bit; the
    statistics it leaves are the next stream's fp64 sums."""
    C, H, W = BIG_SHAPE
    B, chw, d, factor = BIG_B, TILE, BIG_D, 0.8
    n = B * chw
    seed, s0, s1 = 2**64 - 1, 2**47 + 1, 2**47 + 3
    assert _tile_grid(hl, n, 0) == hl.NPART == 1024 and (n // TILE) > 4 * hl.NPART and _route(chw, 1, 0) == "aligned"
    t0, t1 = _device_lattice(C, H, W, seed, s0 + 1).view(1, chw), _device_lattice(C, H, W, seed, s1 + 1).view(1, chw)
    _BIG_TERMS["t0"], _BIG_TERMS["t1"] = _terms_np(t0), _terms_np(t1)
    raw0, raw1 = _big_raw(seed, s0, "t0"), _big_raw(seed, s1, "t1")
    norm0, norm1 = _scale(raw0, factor), _scale(raw1, factor)
    # the generating kernel and the normalising pair at the capped grid
    part = hl.new_partials("cuda")
    gen = hl.perlin_generate((B, C, H, W), t0, d, seed, s0, 0, partials=part).view(-1)
    for tile, got in _windows(gen):
        _check_raw(got, t0, seed, s0, chw, d, n, 0, tile * TILE, TILE, family="perlin_raw_capped")
    _check_stats(hl, part, raw0)
    noise0 = hl.perlin_noise((B, C, H, W), t0, d, seed, s0, 0, factor).view(-1)
    noise1 = hl.perlin_noise((B, C, H, W), t1, d, seed, s1, 0, factor).view(-1)
    for tile, got in _windows(noise0):
        assert _seen("perlin_normalised", _rel(_np(got), norm0[tile * TILE:(tile + 1) * TILE])) < NORMAL_TOL * 2
    # the fused look-ahead launch: no statistics left for it, then the ones it left itself
    fused = _tile_grid(hl, n, 0) == hl.NPART
    assert fused
    out0, out1 = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    p0, p1, p2 = hl.new_partials("cuda"), hl.new_partials("cuda"), hl.new_partials("cuda")
    lat_out = torch.full((C, H, W), float("nan"), device="cuda")
    _ahead(hl, t0, out0, B, chw, d, seed, s0, 0, factor, p0, 0, s1, t1, p1, lat_out, (5, C, H, W, hl.BLEND_IDS["subtract_b"], 9))
    assert torch.equal(out0, noise0)
    _check_stats(hl, p1, raw1)
    lat_err = np.max(np.abs(_np(lat_out) - ds.perlin_lattice(seed, 9, 5, C, H, W, "subtract_b").reshape(-1)))
    assert _seen("perlin_lattice_per_iter", lat_err / 5) <= LATTICE_TOL
    _ahead(hl, t1, out1, B, chw, d, seed, s1, 0, factor, p1, 1, s0, t0, p2)
    assert torch.equal(out1, noise1)
    _check_stats(hl, p2, raw0)
    for tile, got in _windows(out1):
        assert _seen("perlin_ahead", _rel(_np(got), norm1[tile * TILE:(tile + 1) * TILE])) < NORMAL_TOL * 2


# ------------------------------------------------------------------------------------------------ accumulating form
ACC_CASES = [c for c in RAW_CASES if c[0] in ("aligned_2x16384_off", "fast_5x63232_latent3", "vector_3x1280_two_tables", "scalar_3x256_out_misaligned")]


@pytest.mark.parametrize("case", ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_accumulating_form_against_fp64(hl, case):
    """sonar_perlin_generate_acc_f32: y <- y a + perlin b on each route, also a = 1."""
    name, route, B, shape, off, kind, divisors, (mis_out, mis_terms) = case
    chw, n = math.prod(shape), B * math.prod(shape)
    seed, stream = _keys(RAW_CASES.index(case) + 1)
    terms = _case_terms(kind, shape, seed, stream, mis_terms)
    y0 = torch.randn(B, chw, generator=torch.Generator().manual_seed(n))
    for d, (a, b) in zip((divisors[0], divisors[1]), ((0.5, -1.5), (1.0, 0.75))):
        y = _view((B, chw), mis_out)
        y.copy_(y0)
        assert _route(chw, terms.shape[0], off, y, terms) == route
        part = hl.new_partials("cuda")
        hl.perlin_generate_acc_(y, a, b, terms, d, seed, stream, off, partials=part)
        x, _ = ds.perlin_values(seed, stream, _terms_np(terms), chw, d, n, off)
        want = y0.double().numpy().reshape(-1) * float(np.float32(a)) + x * float(np.float32(b))
        assert _seen("perlin_acc", _rel(_np(y), want)) < 2 * NORMAL_TOL
        _check_stats(hl, part, want)


# ------------------------------------------------------------------------------------------------ the pair kernel
@pytest.mark.parametrize("B, shape, first_latent", [(2, (1, 64, 64), 0), (5, (4, 104, 152), 1)], ids=["2x4096", "5x63232_latent1"])
@pytest.mark.parametrize("host, prefix", [("perlin", "perlin"), ("perlin", "normal"), ("normal", "perlin"), ("normal", "normal")])
@pytest.mark.parametrize("fresh", [0, 1])
def test_chained_items_against_fp64(hl, B, shape, first_latent, host, prefix, fresh):
    """sonar_perlin_generate_chain_f32 / sonar_philox_normal_chain_f32: the previous item's fold evaluated inside the host item's pass, host
    and prefix with divisors of different kinds, against the fp64 composition of perlin_values and normal_fill."""
    C, H, W = shape
    chw, n, off = C * H * W, B * C * H * W, first_latent * C * H * W
    (hseed, hstream), (pseed, pstream) = _keys(1), _keys(5)
    dh, dp = (1.5, -4.0) if fresh else (2.0, -1.7)
    a1, b1 = (1.0, 1.0) if fresh else (0.5, 0.3)
    a2, b2 = 1.25, 0.6
    th, tp = _device_lattice(C, H, W, hseed, hstream + 1).view(1, chw), _device_lattice(C, H, W, pseed, pstream + 1).view(1, chw)
    y0 = torch.randn(B, chw, generator=torch.Generator().manual_seed(n + fresh))
    y = torch.full((B, chw), float("nan"), device="cuda") if fresh else y0.cuda()
    if prefix == "perlin":
        pre = hl.FoldPrefix(hl.PREFIX_PERLIN, y, a1, b1, pseed, pstream, off, terms=tp, div_fac=dp, fresh=bool(fresh))
        xp, _ = ds.perlin_values(pseed, pstream, _terms_np(tp), chw, dp, n, off)
    else:
        pre = hl.FoldPrefix(hl.PREFIX_NORMAL, y, a1, b1, pseed, pstream, off, fresh=bool(fresh))
        xp = ds.normal_fill(pseed, pstream, n, off)
    assert hl._hosts_pair(y, off, pre, chw) and n % 4 == 0 and off % 4 == 0 and chw % 4 == 0   # launch_pair_fold's conditions
    part = hl.new_partials("cuda")
    if host == "perlin":
        hl.perlin_generate_acc_(y, a2, b2, th, dh, hseed, hstream, off, partials=part, pre=pre)
        xh, _ = ds.perlin_values(hseed, hstream, _terms_np(th), chw, dh, n, off)
    else:
        hl.philox_normal_acc_(y, a2, b2, hseed, hstream, off, partials=part, pre=pre)
        xh = ds.normal_fill(hseed, hstream, n, off)
    assert pre.consumed
    y1 = xp if fresh else y0.double().numpy().reshape(-1) * float(np.float32(a1)) + xp * float(np.float32(b1))
    want = y1 * float(np.float32(a2)) + xh * float(np.float32(b2))
    assert _seen("perlin_chain", _rel(_np(y), want)) < 2 * NORMAL_TOL
    _check_stats(hl, part, want)


# ------------------------------------------------------------------------------------------------ a Perlin item hosted by the Brownian and pyramid kernels
@pytest.mark.parametrize("shape", [(4, 64, 64), (4, 30, 30)], ids=["burst_4x64x64", "philox_4x30x30"])
@pytest.mark.parametrize("d, fresh", [(1.5, 0), (-4.0, 0), (1.5, 1), (-4.0, 1)])
def test_perlin_prefix_of_a_brownian_item_against_fp64(hl, shape, d, fresh):
    """brownian_bridge_acc_ with a Perlin FoldPrefix: latents of whole tiles host it in the node-burst kernel (with_divider(pdiv, ...));
    any other latent gets the Philox family and the prefix's own launch.  The fp64 composition with brownian_expansion is the reference."""
    B, first_latent, nodes, coefs = 2, 1, [3, 9, 2**40 + 1], [0.5, -0.25, 1.5]
    chw = math.prod(shape)
    n, off = B * chw, first_latent * chw
    seed, (pseed, pstream) = 2**32 + 5, _keys(4)
    a1, b1 = (1.0, 1.0) if fresh else (0.5, 0.3)
    a2, b2 = 0.6, -0.8
    tp = _device_lattice(*shape, pseed, pstream + 1).view(1, chw)
    y0 = torch.randn(B, *shape, generator=torch.Generator().manual_seed(chw + fresh))
    y = torch.full((B, *shape), float("nan"), device="cuda") if fresh else y0.cuda()
    pre = hl.FoldPrefix(hl.PREFIX_PERLIN, y, a1, b1, pseed, pstream, off, terms=tp, div_fac=d, fresh=bool(fresh))
    family = ds.brownian_family(n, off, chw)
    assert family == ("burst" if chw % TILE == 0 else "philox") and pre.hosted(y, off)
    hl.brownian_bridge_acc_(y, a2, b2, nodes, coefs, seed, off, None, want_w=False, pre=pre)
    assert pre.consumed
    xp, _ = ds.perlin_values(pseed, pstream, _terms_np(tp), chw, d, n, off)
    z = ds.brownian_z(seed, nodes, n, off, chw)
    w = np.asarray(coefs) @ z
    y0n = y0.double().numpy().reshape(-1)
    y1, mag1 = (xp, np.abs(xp)) if fresh else (y0n * float(np.float32(a1)) + xp * float(np.float32(b1)), np.abs(y0n * a1) + np.abs(xp * b1))
    want = y1 * float(np.float32(a2)) + w * float(np.float32(b2))
    mag = mag1 * abs(a2) + np.abs(np.asarray(coefs)[:, None] * z).sum(axis=0) * abs(b2)
    assert _seen("perlin_in_brownian_" + family, float(np.max(np.abs(_np(y) - want) / (1.0 + mag)))) < BROWNIAN_TOL


@pytest.mark.parametrize("d, fresh", [(1.5, 0), (-4.0, 0), (1.5, 1), (-4.0, 1)])
def test_perlin_prefix_of_a_pyramid_item_against_fp64(hl, d, fresh):
    """sonar_pyramid_generate_acc_f32 hosting a Perlin item in the plane kernel (2 x 4 x 64 x 64, drawn level grids) against the fp64
    composition with pyramid_planes; the bound is the plane kernel's own of tests/test_gpu_pyramid_oracle.py, per 1 + sum |terms|."""
    name, shape, levels, mode, route, _, _ = R.PLANE_CASES[0]
    assert shape == (2, 4, 64, 64)
    B, C, H, W = shape
    chw, first_latent = C * H * W, 1
    n, off = B * chw, first_latent * chw
    (seed, stream), (pseed, pstream) = (R.SEEDS[0], R.STREAMS[1]), _keys(2)
    a1, b1 = (1.0, 1.0) if fresh else (0.5, 0.3)
    a2, b2 = 0.9, 0.4
    tp = _device_lattice(C, H, W, pseed, pstream + 1).view(1, chw)
    y0 = torch.randn(shape, generator=torch.Generator().manual_seed(11 + fresh))
    y = torch.full(shape, float("nan"), device="cuda") if fresh else y0.cuda()
    pre = hl.FoldPrefix(hl.PREFIX_PERLIN, y, a1, b1, pseed, pstream, off, terms=tp, div_fac=d, fresh=bool(fresh))
    assert hl.pyramid_route(H, W, levels, mode, off) == route and route in (1, 2) and pre.hosted(y, off)
    assert hl.pyramid_generate_acc_(y, a2, b2, levels, mode, seed, stream, off, pre=pre) and pre.consumed
    xp, _ = ds.perlin_values(pseed, pstream, _terms_np(tp), chw, d, n, off)
    planes, pmag = ds.pyramid_planes(seed, stream, B * C, H, W, levels, mode, off, R.resize, magnitude=True)
    planes, pmag = planes.reshape(-1), pmag.reshape(-1)
    y0n = y0.double().numpy().reshape(-1)
    y1, mag1 = (xp, np.abs(xp)) if fresh else (y0n * float(np.float32(a1)) + xp * float(np.float32(b1)), np.abs(y0n * a1) + np.abs(xp * b1))
    want = y1 * float(np.float32(a2)) + planes * float(np.float32(b2))
    mag = mag1 * abs(a2) + pmag * abs(b2)
    assert _seen("perlin_in_pyramid", float(np.max(np.abs(_np(y) - want) / (1.0 + mag)))) < PYRAMID_TOL[PYRAMID_FAMILY[route]]


# ------------------------------------------------------------------------------------------------ the generator's key use
SIG = (torch.tensor(14.6), torch.tensor(10.0))


@pytest.mark.parametrize("shape", [(3, 4, 16, 16), (2, 4, 64, 64)], ids=["3x4x16x16", "2x4x64x64"])
@pytest.mark.parametrize("first_latent", [0, 1])
def test_generator_takes_two_streams_and_offsets_by_the_first_latent(api, shape, first_latent):
    """get_noise_sampler("perlin", cpu=False): PerlinOldNoiseGenerator takes device_key(2), draws the base on `stream` and the lattice
    (2 iterations, lerp, div_fac 2) on `stream + 1`, and a shard starts at its first latent's element.  Raw values: the oracle lattice in
    fp64 stands in for the device's, so the bound is the lattice's (two iterations) plus the sum's rounding; normalised values divide
    that by the tensor's std."""
    ng = api.noise_generation
    B, C, H, W = shape
    chw = C * H * W
    n, off = B * chw, first_latent * chw
    x = torch.zeros(shape, device="cuda")

    def run(normalized, factor):
        torch.manual_seed(2024 + first_latent)
        state = torch.cuda.get_rng_state()
        with ng.shard_offset(first_latent):
            got = api.noise.get_noise_sampler("perlin", x, 0.03, 14.6, seed=None, cpu=False, factor=factor, normalized=normalized)(*SIG)
        torch.cuda.set_rng_state(state)
        return got, ng.DeviceRNG.take()

    raw, (seed, stream) = run(False, 1.0)
    terms = ds.perlin_lattice(seed, stream + 1, 2, C, H, W, "lerp").reshape(1, chw)
    want, _ = ds.perlin_values(seed, stream, terms, chw, 2.0, n, off)
    bound = 2 * LATTICE_TOL + ds.perlin_rounding_bound(seed, stream, terms, chw, 2.0, n, off)
    assert tuple(raw.shape) == shape and np.all(np.abs(_np(raw) - want) <= bound)
    factor = 0.7
    normed, keys = run(True, factor)
    assert keys == (seed, stream)
    dec = {}
    want_n = _scale(want, factor, dec)
    assert dec["sub"] and dec["div"]
    err = np.abs(_np(normed) - want_n)
    assert np.all(err <= NORMAL_TOL * 2 * (1.0 + np.abs(want_n)) + 2 * LATTICE_TOL * factor / dec["std"])
