"""CPU: the fp64 resampler of tests/pyramid_refs.py against torch.nn.functional.interpolate on float32 inputs at every (source,
destination, mode) pair tests/test_gpu_pyramid_oracle.py resamples, and its case tables against the budget arithmetic that routes a
pyramid call (restated in pyramid_refs.route; on the GPU the cases assert the library's own answer, sonar_pyramid_route)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pyramid_refs as R

PAIRS = R.resize_pairs()


@pytest.mark.parametrize("mode", R.MODES)
def test_resampler_against_interpolate(mode):
    """nearest-exact / nearest pick the very element ATen picks; bilinear, bicubic and area within 2e-6 peak + 2e-6 (the bound of
    test_scale_samples_every_mode: ATen sums in fp32).  ATen's CPU kernels round the source coordinate of bilinear / bicubic once or
    twice depending on how they were built (pyramid_refs: ``fused``): ONE of the two conventions must hold at every pair."""
    pairs = [(src, dst) for src, dst, m in PAIRS if m == mode]
    assert pairs
    worst = {}
    for fused in (False, True):
        g = torch.Generator().manual_seed(11)
        worst[fused] = -np.inf
        for (h, w), (H, W) in pairs:
            x = torch.randn(2, 3, h, w, generator=g)
            want = F.interpolate(x, size=(H, W), mode=mode).double().numpy()
            got = R.resize(x.numpy(), H, W, mode, fused=fused)
            assert got.shape == want.shape and got.dtype == np.float64
            if mode in ("nearest-exact", "nearest"):
                assert np.array_equal(got, want), ((h, w), (H, W))
            else:
                worst[fused] = max(worst[fused], np.abs(got - want).max() - (2e-6 * np.abs(want).max() + 2e-6))
        if mode in ("nearest-exact", "nearest", "area"):
            assert worst[fused] <= 0 and np.array_equal(got, R.resize(x.numpy(), H, W, mode))   # no source coordinate: no convention
    assert min(worst.values()) <= 0, worst


def test_the_two_coordinate_roundings_differ_by_an_ulp():
    """fused or not, the source coordinate is the same real number rounded once or twice: the two resamplers differ by at most an ulp of
    the coordinate (2^-18 below 64) times the largest step between neighbouring samples, per axis."""
    g = np.random.default_rng(3).standard_normal((2, 50, 70))
    step = max(np.abs(np.diff(g, axis=-1)).max(), np.abs(np.diff(g, axis=-2)).max())
    for mode, gain in (("bilinear", 1.0), ("bicubic", 2.0)):   # (the cubic kernel's slope is at most 1.5 of a step, its taps overshoot)
        d = np.abs(R.resize(g, 24, 40, mode, fused=True) - R.resize(g, 24, 40, mode, fused=False)).max()
        assert 0 < d <= 2 * gain * 2.0**-18 * step


def test_every_mode_is_exercised():
    assert {m for _, _, m in PAIRS} == set(R.MODES)
    sizes = {src for src, _, _ in PAIRS}
    assert {(1, 1), (3, 3), (5, 7), (33, 33), (21, 20), (3, 10), (63, 63), (127, 127)} <= sizes


def test_area_windows_overlap_off_whole_ratios():
    lo, hi = R.area_windows(21, 64)
    assert (hi - lo).max() == 2 and (lo[1:] < hi[:-1]).any()       # enlarging: neighbouring outputs share a sample
    lo, hi = R.area_windows(50, 40)
    assert (hi - lo).max() == 2 and (lo[1:] < hi[:-1]).any()       # shrinking by 5 / 4
    lo, hi = R.area_windows(96, 24)
    assert np.array_equal(lo, np.arange(24) * 4) and np.array_equal(hi, lo + 4)


@pytest.mark.parametrize("case", R.PLANE_CASES, ids=[c[0] for c in R.PLANE_CASES])
def test_plane_cases_land_on_their_route(case):
    name, shape, levels, mode, want, _, shards = case
    H, W = shape[-2:]
    assert shape[0] * shape[1] * H * W <= 110_000
    for k in shards:
        assert R.route(H, W, levels, mode, k * H * W) == want
    assert any(g is None and (h, w) != (H, W) for g, h, w, _ in levels)   # a drawn grid
    assert len(R.grid_sizes(H, W, levels)) <= 12


def test_route_budgets_as_stated():
    by = {c[0]: c for c in R.PLANE_CASES}
    _, shape, levels, mode, *_ = by["rows_do_not_fit"]
    assert R.budget(*shape[-2:], levels, mode) == (37920, 70688)
    _, shape, levels, mode, *_ = by["tiles_3_86"]
    assert len(levels) == 12 and R.budget(*shape[-2:], levels, mode)[1] <= R.LDS_BUDGET
    assert len(R.THIRTEEN) == 13
    # what the shapes reach: planes per tile, tiles per plane, rows per stretch round
    assert by["tile_per_plane"][1][-2] * by["tile_per_plane"][1][-1] == 4096
    assert 4 * 32 * 32 == 4096 and 40 * 36 == 1440 and 512 % 36 != 0 and 128 * 160 == 5 * 4096
    assert abs(104 * 152 / 4096 - 3.86) < 0.005
    assert by["more_planes_than_workgroups"][1][0] == 1027


@pytest.mark.parametrize("case", R.FLAT_CASES, ids=[c[0] for c in R.FLAT_CASES])
def test_flat_cases_land_on_their_route(case):
    name, shape, levels, off, routes = case
    H, W = shape[-2:]
    assert set(routes) == set(R.FLAT_MODES)
    for mode, want in routes.items():
        assert R.route(H, W, levels, mode, off) == want
    assert off % 4 == 0 and all(g is not None for g, *_ in levels)


def test_flat_case_budgets_as_stated():
    _, shape, levels, _, _ = R.FLAT_CASES[0]
    assert R.budget(*shape[-2:], levels, "nearest-exact")[0] == 64656 and R.budget(*shape[-2:], levels, "bilinear")[0] == 64656 + 4096
    assert R.FLAT_CASES[2][3] % (32 * 36) != 0


def test_sampled_cases_reach_the_far_keys():
    h, w = R.SAMPLED_FAR_LEVELS[1][:2]
    assert R.SAMPLED_FAR_PLANE_OFFSET * h * w // 4 >= 2**32
    shape, po, _ = R.LEVEL_NORMAL_CASES[2]
    assert po * shape[-2] * shape[-1] // 4 >= 2**32
    shape, po, _ = R.LEVEL_NORMAL_CASES[0]
    assert po * shape[-2] * shape[-1] == 35                      # the first Philox group is cut
    shape, po, _ = R.LEVEL_NORMAL_CASES[3]
    assert (po * 35) % 4 != 0 and ((po + shape[0]) * 35) % 4 != 0   # ... and here the last one too
    assert len(R.SAMPLED_SIXTEEN) == 16
    H, W = R.SAMPLED_SHAPE[-2:]
    assert all(h % H == 0 and w % W == 0 for h, w, *_ in R.SAMPLED_AREA_LEVELS) and 50 % H != 0


def test_the_library_routes_as_the_tables_say(pkg):
    """sonar_pyramid_route is host arithmetic: it answers without a GPU, and as pyramid_refs.route restates it."""
    hl = pkg.hip_lib
    for name, shape, levels, mode, want, _, shards in R.PLANE_CASES:
        for k in shards:
            assert hl.pyramid_route(*shape[-2:], levels, mode, k * shape[-2] * shape[-1]) == want, name
    for name, shape, levels, off, routes in R.FLAT_CASES:
        for mode, want in routes.items():
            assert hl.pyramid_route(*shape[-2:], levels, mode, off) == want, (name, mode)
    H, W = 64, 64
    for n in (60, 61, 62, 63, 64, 90, 126, 127, 128):                  # across both thresholds
        for mode in R.FLAT_MODES:
            lv = [(None, n, n, 1.0), (None, 2, 3, 0.5)]
            assert hl.pyramid_route(H, W, lv, mode) == R.route(H, W, lv, mode), (n, mode)
    assert hl.pyramid_route(8, 10, [(3, 3)], "bilinear") == 0             # W % 4
    assert hl.pyramid_route(8, 12, [(3, 3)], "bilinear", 4) == 0 and hl.pyramid_route(8, 12, [(3, 3)], "bilinear", 96) == 2
    lib = hl.load()
    n, _, hs, ws, _ = hl._pyramid_args(R.THIRTEEN)
    assert lib.sonar_pyramid_route(104, 152, n, hs, ws, 0, 0) == hl.ERR_UNSUPPORTED
    assert lib.sonar_pyramid_route(104, 152, n, None, ws, 0, 0) == hl.ERR_ARG and lib.sonar_pyramid_route(104, 152, 0, None, None, 3, 0) == hl.ERR_ARG
    assert lib.sonar_pyramid_route(104, 152, 0, None, None, 0, 0) == 2
