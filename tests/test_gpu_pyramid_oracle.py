"""Generate-mode pyramid noise against its stream contract (-m gpu): the plane kernel in its stretched-rows form (route 2) and its
plain form (route 1), the flat kernel (route 0), sonar_level_normal_f32 and sonar_levels_sampled_f32, every value compared with
oracle/device_streams.py (pyramid_level_grid, level_normal, pyramid_planes) through the fp64 resampler of tests/pyramid_refs.py -- at
the plane sizes, level sizes, level lists, shard offsets, seeds and stream ids where a stream id, slot, plane key, tap or row could be
wrong.  Every case asserts the kernel it gets (sonar_pyramid_route) before it compares values.  A mapping error is an O(1) difference;
the bounds only absorb fp32 against fp64: Box-Muller (~2e-7, tests/test_gpu_generate_oracle.py) plus one fp32 sum per level.

The error of a value is |kernel - fp64| / (1 + base_scale |z| + sum_l |w_l| max |grid_l|); of a normalised value and of a level value
|kernel - fp64| / (1 + |fp64|).  Measured on an MI355X, the maximum over every case of the family (SONAR_ORACLE_ERRORS=<file> writes
them out), and the bound, about four times that:
  plane kernel, stretched rows (route 2) 1.43e-7 ................. bound 6e-7
  plane kernel (route 1: bilinear, nearest-exact, area) 1.13e-7 .. bound 5e-7
  flat kernel (route 0) 9.1e-8 ................................... bound 4e-7
  normalised (pyramid_noise, factor 0.7), every route 5.28e-7 .... bound 2e-6
  sonar_level_normal_f32 1.50e-7 ................................. bound 6e-7
  sonar_levels_sampled_f32: bilinear 6.0e-8 (bound 2.5e-7), nearest-exact 6.9e-8 (3e-7), nearest 7.7e-8 (3e-7), bicubic 1.26e-7
  (5e-7), area 5.2e-8 (2e-7); a single nearest tap against the oracle's chosen element: the Box-Muller bound 1e-6 per (1 + |value|)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import device_streams as ds
from oracle import sonar_oracle as orc
from tests import pyramid_refs as R

pytestmark = pytest.mark.gpu

TOL = {   # about 4 x the measured maxima of the module docstring
    "pyramid_route2": 6e-7, "pyramid_route1": 5e-7, "pyramid_flat": 4e-7, "pyramid_normalised": 2e-6, "level_normal": 6e-7,
    "levels_sampled_bilinear": 2.5e-7, "levels_sampled_nearest-exact": 3e-7, "levels_sampled_nearest": 3e-7, "levels_sampled_bicubic": 5e-7,
    "levels_sampled_area": 2e-7,
}
BOX_MULLER_TOL = 1e-6   # test_gpu_generate_oracle.NORMAL_TOL: a single tap of a nearest mode is one Box-Muller value times sd and weight
STATS_RTOL = 1e-5       # statistics against the fp64 sums: what the fill tests use
FAMILY = {0: "pyramid_flat", 1: "pyramid_route1", 2: "pyramid_route2"}


@pytest.fixture(scope="module")
def hl(pkg):
    lib = pkg.hip_lib
    lib.load()
    return lib


MEASURED: dict = {}  # family -> max error seen (merged into the file SONAR_ORACLE_ERRORS names: how the bounds were set)


@pytest.fixture(scope="module", autouse=True)
def _report_measured():
    yield
    import json
    import os

    path = os.environ.get("SONAR_ORACLE_ERRORS")
    if path:
        seen = json.load(open(path)) if os.path.exists(path) else {}   # (tests/test_gpu_generate_oracle.py writes the same file)
        seen.update(MEASURED)
        with open(path, "w") as f:
            json.dump(seen, f, indent=1)


def _seen(family, err):
    MEASURED[family] = max(MEASURED.get(family, 0.0), float(err))
    return err


def _st():
    return torch.cuda.current_stream().cuda_stream


def _keys(i):
    return R.SEEDS[i % 2], R.STREAMS[(i // 2) % 2]


def _supplied(levels, planes, tag):
    """The case's level list for the library (device tensors) and for the oracle (fp64 arrays): grids marked ``supplied`` are torch.randn
    on the host."""
    g = torch.Generator().manual_seed(1000 + tag)
    dev, host = [], []
    for grid, h, w, wt in levels:
        if grid is None:
            dev.append((None, h, w, wt))
            host.append((None, h, w, wt))
        else:
            t = torch.randn(planes, h, w, generator=g)
            dev.append((t.cuda(), h, w, wt))
            host.append((t.double().numpy(), h, w, wt))
    return dev, host


@functools.lru_cache(maxsize=None)
def _want_planes(table, index, mode, k):
    """fp64 planes and per-value magnitudes of a case (computed once; shared, never written to)."""
    if table == "plane":
        name, shape, levels, _, _, _, _ = R.PLANE_CASES[index]
        off = k * shape[-2] * shape[-1]
    else:
        name, shape, levels, off, _ = R.FLAT_CASES[index]
    planes, (H, W) = shape[0] * shape[1], shape[-2:]
    seed, stream = _keys(index)
    dev, host = _supplied(levels, planes, index)
    want, mag = ds.pyramid_planes(seed, stream, planes, H, W, host, mode, off, R.resize, magnitude=True)
    want.setflags(write=False)
    mag.setflags(write=False)
    return dev, want, mag


def _err(got, want, mag):
    got = got.detach().cpu().double().numpy().reshape(want.shape)
    assert np.isfinite(got).all()
    return float(np.max(np.abs(got - want) / (1.0 + mag)))


def _check_stats(hl, part, want):
    tot = hl.stats_finalize(part, want.size).cpu().double().numpy()
    assert abs(tot[0] - want.sum()) < STATS_RTOL * np.abs(want).sum() and abs(tot[1] - (want * want).sum()) < STATS_RTOL * (want * want).sum()


def _normalised(want, factor):
    return orc.scale_noise(torch.from_numpy(want.copy()), factor, normalized=True).numpy()


# ------------------------------------------------------------------------------------------------ the plane kernel, drawn grids
PLANE_PARAMS = [(i, k) for i, c in enumerate(R.PLANE_CASES) for k in c[6]]


@pytest.mark.parametrize("index, k", PLANE_PARAMS, ids=[f"{R.PLANE_CASES[i][0]}-shard{k}" for i, k in PLANE_PARAMS])
def test_plane_kernel_against_the_oracle(hl, index, k):
    """hl.pyramid_generate (with its statistics where the case asks) and hl.pyramid_noise (factor 0.7) with level grids drawn in the
    kernel; shard k draws the global planes k * planes .. -- the plane key and the tile walk both shift."""
    name, shape, levels, mode, route, stats, _ = R.PLANE_CASES[index]
    H, W = shape[-2:]
    off = k * H * W
    seed, stream = _keys(index)
    dev, want, mag = _want_planes("plane", index, mode, k)
    assert hl.pyramid_route(H, W, dev, mode, off) == route
    part = hl.new_partials("cuda") if stats else None
    got = hl.pyramid_generate(shape, "cuda", dev, mode, seed, stream, off, partials=part)
    assert got is not None
    assert _seen(FAMILY[route], _err(got, want, mag)) < TOL[FAMILY[route]]
    if stats:
        _check_stats(hl, part, want)
    got_n = hl.pyramid_noise(shape, "cuda", dev, mode, seed, stream, off, 0.7)
    want_n = _normalised(want, 0.7)
    assert _seen("pyramid_normalised", _err(got_n, want_n, np.abs(want_n))) < TOL["pyramid_normalised"]


def test_thirteen_levels_are_refused(hl):
    lib = hl.load()
    H, W = 104, 152
    out = torch.zeros(2, 1, H, W, device="cuda")
    n, ptrs, hs, ws, wts = hl._pyramid_args(R.THIRTEEN)
    assert lib.sonar_pyramid_generate_f32(out.data_ptr(), 2, H, W, n, ptrs, hs, ws, wts, 0, 1, 2, 0, None, _st()) == hl.ERR_UNSUPPORTED
    assert lib.sonar_pyramid_route(H, W, n, hs, ws, 0, 0) == hl.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.any()
    assert hl.pyramid_generate((2, 1, H, W), "cuda", R.THIRTEEN, "bilinear", 1, 2) is None
    assert hl.pyramid_route(H, W, R.TWELVE, "bilinear") == 2


# ------------------------------------------------------------------------------------------------ the flat kernel, supplied grids
FLAT_PARAMS = [(i, m) for i in range(len(R.FLAT_CASES)) for m in R.FLAT_MODES]


@pytest.mark.parametrize("index, mode", FLAT_PARAMS, ids=[f"{R.FLAT_CASES[i][0]}-{m}" for i, m in FLAT_PARAMS])
def test_flat_kernel_against_the_oracle(hl, index, mode):
    """Supplied grids beyond the plane kernel's LDS budget, or a shard that does not start on a plane: normal_fill plus the resampler."""
    name, shape, levels, off, routes = R.FLAT_CASES[index]
    H, W = shape[-2:]
    seed, stream = _keys(index)
    dev, want, mag = _want_planes("flat", index, mode, 0)
    route = routes[mode]
    assert hl.pyramid_route(H, W, dev, mode, off) == route
    part = hl.new_partials("cuda")
    got = hl.pyramid_generate(shape, "cuda", dev, mode, seed, stream, off, partials=part)
    assert _seen(FAMILY[route], _err(got, want, mag)) < TOL[FAMILY[route]]
    _check_stats(hl, part, want)
    got_n = hl.pyramid_noise(shape, "cuda", dev, mode, seed, stream, off, 0.7)
    want_n = _normalised(want, 0.7)
    assert _seen("pyramid_normalised", _err(got_n, want_n, np.abs(want_n))) < TOL["pyramid_normalised"]


def test_a_drawn_level_on_the_flat_route_is_refused(hl):
    for shape, levels, off in (((1, 3, 32, 36), [(None, 9, 9, 0.7)], 4 * 77), ((2, 2, 64, 64), [(None, 127, 127, 0.7), (None, 5, 7, 0.5)], 0)):
        assert hl.pyramid_route(*shape[-2:], levels, "bilinear", off) == 0
        assert hl.pyramid_generate(shape, "cuda", levels, "bilinear", 3, 4, off) is None
        assert hl.pyramid_noise(shape, "cuda", levels, "bilinear", 3, 4, off, 0.7) is None


# ------------------------------------------------------------------------------------------------ level values
@pytest.mark.parametrize("i", range(len(R.LEVEL_NORMAL_CASES)))
def test_level_normal_against_the_oracle(hl, i):
    shape, po, sd = R.LEVEL_NORMAL_CASES[i]
    seed, stream = _keys(i)
    h, w = shape[-2:]
    n = int(np.prod(shape))
    got = hl.level_normal(shape, "cuda", sd, seed, stream, po)
    want = ds.level_normal(seed, stream, po * h * w + np.arange(n, dtype=np.int64)) * float(np.float32(sd))
    assert _seen("level_normal", _err(got, want, np.abs(want))) < TOL["level_normal"]


@functools.lru_cache(maxsize=None)
def _whole_levels(shape, po, levels, seed, stream):
    """Every level of a levels_sampled call as a whole fp64 grid [planes, h, w] (std sd): level l from the stream id stream + l."""
    planes = shape[0] * shape[1]
    out = []
    for l, (h, w, _, sd) in enumerate(levels):
        e = po * h * w + np.arange(planes * h * w, dtype=np.int64)
        g = ds.level_normal(seed, stream + l, e).reshape(planes, h, w) * float(np.float32(sd))
        g.setflags(write=False)
        out.append(g)
    return out


def _sampled_want(shape, po, levels, seed, stream, mode):
    H, W = shape[-2:]
    grids = _whole_levels(shape, po, tuple(levels), seed, stream)
    want = sum(float(np.float32(lv[2])) * R.resize(g, H, W, mode) for lv, g in zip(levels, grids))
    mag = sum(abs(lv[2]) * np.abs(g).max() for lv, g in zip(levels, grids))
    return want.reshape(shape), mag


SAMPLED_SETS = [("five_levels", R.SAMPLED_SHAPE, R.SAMPLED_PLANE_OFFSET, R.SAMPLED_LEVELS),
                ("far_keys", R.SAMPLED_FAR_SHAPE, R.SAMPLED_FAR_PLANE_OFFSET, R.SAMPLED_FAR_LEVELS)]


@pytest.mark.parametrize("mode", R.SAMPLED_MODES)
@pytest.mark.parametrize("which", range(len(SAMPLED_SETS)), ids=[s[0] for s in SAMPLED_SETS])
def test_levels_sampled_against_resampled_oracle_levels(hl, which, mode):
    """The taps the kernel draws against the resampler run over whole oracle levels; then onto an existing ``out``."""
    _, shape, po, levels = SAMPLED_SETS[which]
    seed, stream = _keys(which + 1)
    want, mag = _sampled_want(shape, po, levels, seed, stream, mode)
    got = hl.levels_sampled(shape, "cuda", levels, mode, seed, stream, po)
    assert got is not None
    fam = "levels_sampled_" + mode
    assert _seen(fam, _err(got, want, mag)) < TOL[fam]
    y0 = torch.randn(shape, generator=torch.Generator().manual_seed(9))
    y = hl.levels_sampled(shape, "cuda", levels, mode, seed, stream, po, out=y0.cuda())
    assert _seen(fam, _err(y, want + y0.double().numpy(), mag + np.abs(y0.double().numpy()))) < TOL[fam]
    if mode in ("nearest-exact", "nearest"):
        # one tap per level: the oracle's chosen element to the Box-Muller bound, level by level -- a neighbouring element fails
        H, W = shape[-2:]
        index = R.nearest_exact_index if mode == "nearest-exact" else R.nearest_index
        grids = _whole_levels(shape, po, tuple(levels), seed, stream)
        for l, (lv, g) in enumerate(zip(levels, grids)):
            one = hl.levels_sampled(shape, "cuda", [lv], mode, seed, stream + l, po)
            pick = g[:, index(lv[0], H)[:, None], index(lv[1], W)[None, :]] * float(np.float32(lv[2]))
            assert _err(one, pick.reshape(shape), np.abs(pick.reshape(shape))) < BOX_MULLER_TOL * max(1.0, abs(lv[2]) * lv[3]), (l, lv)


def test_levels_sampled_area_is_keyed_by_the_output_element(hl):
    """Area over whole blocks: one normal per output element and level, std sd / sqrt(r_h r_w), keyed by the output's global index; any
    other ratio is refused."""
    shape, po, levels = R.SAMPLED_SHAPE, R.SAMPLED_PLANE_OFFSET, R.SAMPLED_AREA_LEVELS
    seed, stream = _keys(0)
    H, W = shape[-2:]
    n = int(np.prod(shape))
    e = po * H * W + np.arange(n, dtype=np.int64)
    want, mag = np.zeros(n), 0.0
    for l, (h, w, wt, sd) in enumerate(levels):
        std = float(np.float32(sd) / np.sqrt(np.float32(h // H) * np.float32(w // W), dtype=np.float32))
        z = ds.level_normal(seed, stream + l, e) * std
        want += float(np.float32(wt)) * z
        mag += abs(wt) * np.abs(z).max()
    got = hl.levels_sampled(shape, "cuda", levels, "area", seed, stream, po)
    assert _seen("levels_sampled_area", _err(got, want.reshape(shape), mag)) < TOL["levels_sampled_area"]
    assert hl.levels_sampled(shape, "cuda", R.SAMPLED_LEVELS[:3], "area", seed, stream, po) is None   # 50 x 70: the windows overlap


def test_levels_sampled_takes_sixteen_levels(hl):
    shape, levels = R.SAMPLED_SIXTEEN_SHAPE, R.SAMPLED_SIXTEEN
    seed, stream = _keys(3)
    want, mag = _sampled_want(shape, 2, levels, seed, stream, "bilinear")
    got = hl.levels_sampled(shape, "cuda", levels, "bilinear", seed, stream, 2)
    assert got is not None
    assert _seen("levels_sampled_bilinear", _err(got, want, mag)) < TOL["levels_sampled_bilinear"]
    assert hl.levels_sampled(shape, "cuda", levels + [(2, 2, 0.1, 1.0)], "bilinear", seed, stream, 2) is None
