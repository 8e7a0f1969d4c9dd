"""-m gpu: statistics over any subset of dimensions (csrc/group_stats.hip) and NormalizeToScaleNoise through them.  The kernels against
torch in float64; the split route's determinism; argument checks; empty tensors; the affine / rescale kernels bit for bit against the row
kernels on a transposed copy; every case of tests/golden/normalize_dims.npz through the item; normalize_to_scale; plan replay.

Tolerances.  Kernel level: the sums are float64 (a product of two floats is exact there), so mean and std are the float64 values rounded
to float32 once: rtol 2^-23 of the value, and atol 1e-10 for the float64 summation error of at most 2 x 10^4 values of size <= 8
(2e4 * 8 * 1.1e-16 = 2e-11) where a mean is near zero.  Min / max are exact.  Item level: the node sweep's atol = 2e-6 * max|want| + 2e-6,
rtol = 0 (tests/test_gpu_round2.py), which the golden script shows the reference's own float32 output to meet against float64."""
import importlib
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import normalize_dims_cases as cases  # noqa: E402

SIG = (torch.tensor(cases.SIGMA[0]), torch.tensor(cases.SIGMA[1]))
SENTINEL = -7.25


@pytest.fixture(scope="module")
def api(pkg):
    pkg.hip_lib.load()
    return types.SimpleNamespace(hl=pkg.hip_lib, nz=importlib.import_module("comfyui_sonar_amd.py.noise"),
                                 utils=importlib.import_module("comfyui_sonar_amd.py.utils"))


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 1.5 + 0.4


def all_dims(shape, dims):
    return tuple(dims) if len(dims) else tuple(range(len(shape)))


# (shape, dims): what each is there for
SHAPES = [
    # kept-inner lengths 1, 3, 5, 67 (a lane per group); group counts 6, 12, 20, 201: no multiples of 64
    ((6, 7, 1), (1,)), ((4, 9, 3), (1,)), ((4, 9, 5), (1,)), ((3, 10, 67), (1,)),
    # reduced lengths 1, 2, 63, 64, 65 on the lane route (64 is the slice: 65 is split in two)
    ((1, 70), (0,)), ((2, 70), (0,)), ((63, 5), (0,)), ((64, 5), (0,)), ((65, 5), (0,)),
    # ... and on the run route: below and above a wave (64), above a wave's four loads (256), at and above the slice (1024)
    ((5, 1), (1,)), ((5, 2), (1,)), ((5, 63), (1,)), ((5, 65), (1,)), ((5, 300), (1,)), ((3, 1024), (1,)), ((3, 1030), (1,)),
    # more groups than one launch has waves (8192 items) and than one workgroup has lanes
    ((9000, 3), (1,)), ((3, 700), (0,)),
    # one to six segments, starting with either kind
    ((1, 3), (0,)), ((3,), (0,)),
    ((3, 2), (0,)), ((3, 2), (1,)),
    ((3, 2, 5), (0, 2)), ((3, 2, 5), (1,)),
    ((3, 2, 5, 2), (0, 2)), ((3, 2, 5, 2), (1, 3)),
    ((3, 2, 5, 2, 3), (0, 2, 4)), ((3, 2, 5, 2, 3), (1, 3)),
    ((3, 2, 5, 2, 3, 4), (0, 2, 4)), ((3, 2, 5, 2, 3, 4), (1, 3, 5)),
    # either side of the split rule on both routes
    ((2049, 3, 7), (0,)), ((64, 3, 7), (0,)), ((5, 3, 700), (0, 2)), ((5, 3, 200), (0, 2)),
    # everything reduced, negative dims, size-1 dimensions in between
    ((7, 11, 13), ()), ((3, 4, 6, 10), (0, -1)), ((2, 1, 3, 1, 4), (0, 4)),
]


@pytest.fixture(scope="module")
def references():
    """The float64 statistics of every shape, computed once on the CPU."""
    out = {}
    for i, (shape, dims) in enumerate(SHAPES):
        x = seeded(shape, 100 + i)
        d = all_dims(shape, dims)
        x64 = x.double()
        out[(shape, dims)] = (x, x64.mean(dim=d, keepdim=True).flatten(), x64.std(dim=d, keepdim=True).flatten(),
                              x.amin(dim=d, keepdim=True).flatten(), x.amax(dim=d, keepdim=True).flatten())
    return out


@pytest.mark.filterwarnings("ignore:std\\(\\)")
@pytest.mark.parametrize("shape,dims", SHAPES, ids=lambda v: "x".join(map(str, v)) or "all")
def test_group_stats_against_float64(api, references, shape, dims):
    x, mean64, std64, lo, hi = references[(shape, dims)]
    xd = x.cuda()
    mean, std, glo, ghi = api.hl.group_stats(xd, dims, mean_std=True, minmax=True)
    for name, got, want in (("mean", mean, mean64), ("std", std, std64)):
        print(f"{name}: max |error| {float((got.cpu().double() - want).abs().nan_to_num(0).max()):.3e}")
        torch.testing.assert_close(got.cpu().double(), want, rtol=2.0 ** -23, atol=1e-10, equal_nan=True)
    assert torch.equal(glo.cpu(), lo) and torch.equal(ghi.cpu(), hi)
    if int(np.prod(shape)) == mean.numel():  # groups of one member: torch's NaN
        assert bool(std.isnan().all())
    # a pair alone gives the bits of the pair in the combined sweep
    m2, s2 = api.hl.group_stats(xd, dims)
    l2, h2 = api.hl.group_stats(xd, dims, mean_std=False, minmax=True)
    assert torch.equal(m2, mean) and torch.equal(s2.nan_to_num(7.0), std.nan_to_num(7.0)) and torch.equal(l2, glo) and torch.equal(h2, ghi)
    assert torch.equal(xd.cpu(), x), "the input was written"


@pytest.mark.parametrize("shape,dims", [((2049, 3, 7), (0,)), ((5, 3, 700), (0, 2)), ((40, 3, 5000), (0, 2)), ((3000, 300), (0,))])
def test_the_split_route_gives_the_same_bits_twice(api, shape, dims):
    sizes, first, _groups = api.hl.group_segments(shape, dims)
    need = api.hl.load().sonar_group_stats_ws_doubles(len(sizes), first, *sizes, *([1] * (6 - len(sizes))), 1, 1)
    assert need > 0, "the shape is not split: the test would show nothing"
    x = seeded(shape, 9).cuda()
    a = api.hl.group_stats(x, dims, mean_std=True, minmax=True)
    junk = torch.randn(1 << 20, device="cuda")  # another allocation pattern between the runs
    b = api.hl.group_stats(x, dims, mean_std=True, minmax=True)
    del junk
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def _raw(api, x, nseg, first, sizes, mean, std, lo, hi, ws):
    hl = api.hl
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return hl.load().sonar_group_stats_f32(ptr(x), nseg, first, *sizes, ptr(mean), ptr(std), ptr(lo), ptr(hi), ptr(ws), hl._stream())


def test_argument_checks_return_err_arg_and_launch_nothing(api):
    hl = api.hl
    lib = hl.load()
    x = seeded((2049, 21), 3).cuda()
    outs = [torch.full((21,), SENTINEL, device="cuda") for _ in range(4)]
    ws = torch.full((33 * 21 * 4,), SENTINEL, dtype=torch.float64, device="cuda")
    ok = (2, 1, (2049, 21, 1, 1, 1, 1))
    bad = [
        _raw(api, x, 0, 1, ok[2], *outs, ws), _raw(api, x, 7, 1, (2, 2, 2, 2, 2, 2), *outs, ws),  # segment count
        _raw(api, x, 2, 1, (-2049, 21, 1, 1, 1, 1), *outs, ws),                                   # a negative size
        _raw(api, None, *ok[:2], ok[2], *outs, ws),                                               # no input
        _raw(api, x, *ok[:2], ok[2], None, None, None, None, ws),                                 # nothing asked for
        _raw(api, x, *ok[:2], ok[2], outs[0], None, None, None, ws),                              # half a pair
        _raw(api, x, *ok[:2], ok[2], outs[0], outs[1], None, outs[3], ws),
        _raw(api, x, *ok[:2], ok[2], x, outs[1], None, None, ws),                                 # a result over x
        _raw(api, x, *ok[:2], ok[2], *outs, None),                                                # a split shape without its workspace
    ]
    a = torch.full((21,), SENTINEL, device="cuda")
    out = torch.full_like(x, SENTINEL)
    seg = (2, 1, 2049, 21, 1, 1, 1, 1)
    bad += [
        lib.sonar_group_affine_f32(2, x.data_ptr(), *seg, a.data_ptr(), a.data_ptr(), out.data_ptr(), hl._stream()),   # op
        lib.sonar_group_affine_f32(0, x.data_ptr(), *seg, None, None, out.data_ptr(), hl._stream()),                   # no operand
        lib.sonar_group_affine_f32(0, x.data_ptr(), *seg, a.data_ptr(), None, None, hl._stream()),                     # no output
        lib.sonar_group_affine_f32(0, None, *seg, a.data_ptr(), None, out.data_ptr(), hl._stream()),
        lib.sonar_group_affine_f32(0, x.data_ptr(), 9, 1, 2049, 21, 1, 1, 1, 1, a.data_ptr(), None, out.data_ptr(), hl._stream()),
        lib.sonar_group_affine_f32(0, x.data_ptr(), *seg, out.data_ptr(), None, out.data_ptr(), hl._stream()),         # out over a table
        lib.sonar_group_minmax_rescale_f32(x.data_ptr(), *seg, None, a.data_ptr(), 1e-7, 0.0, 1.0, out.data_ptr(), hl._stream()),
        lib.sonar_group_minmax_rescale_f32(x.data_ptr(), *seg, a.data_ptr(), a.data_ptr(), 1e-7, 0.0, 1.0, None, hl._stream()),
        lib.sonar_group_minmax_rescale_f32(x.data_ptr(), 0, 1, 2049, 21, 1, 1, 1, 1, a.data_ptr(), a.data_ptr(), 1e-7, 0.0, 1.0, out.data_ptr(), hl._stream()),
        lib.sonar_group_adjust_f32(3, a.data_ptr(), 21, 0.5, out.data_ptr(), hl._stream()),
        lib.sonar_group_adjust_f32(0, None, 21, 0.5, out.data_ptr(), hl._stream()),
        lib.sonar_group_adjust_f32(0, a.data_ptr(), -1, 0.5, out.data_ptr(), hl._stream()),
    ]
    assert bad == [hl.ERR_ARG] * len(bad), bad
    torch.cuda.synchronize()
    for t in (*outs, ws, a, out):
        assert bool((t == SENTINEL).all()), "a refused call wrote something"
    # the same call, accepted
    assert _raw(api, x, *ok[:2], ok[2], *outs, ws) == 0
    assert not bool((outs[0] == SENTINEL).any())


def test_empty_tensors_launch_nothing(api):
    hl = api.hl
    outs = [torch.full((4,), SENTINEL, device="cuda") for _ in range(4)]
    x = torch.empty((0, 4), device="cuda")
    assert _raw(api, x, 2, 1, (0, 4, 1, 1, 1, 1), *outs, None) == 0    # four groups without members
    assert _raw(api, None, 2, 0, (0, 4, 1, 1, 1, 1), *outs, None) == 0  # no groups (an empty tensor has no buffer)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs)
    assert hl.group_affine(0, x, (0,), outs[0], None).shape == x.shape
    assert hl.group_minmax_rescale(x, (0,), outs[0], outs[1], 1e-7, 0.0, 1.0).shape == x.shape
    assert hl.group_adjust(1, torch.empty(0, device="cuda"), 0.5).numel() == 0
    assert all(t.numel() == 4 for t in hl.group_stats(x, (0,)))


LAYOUTS = [((3, 4, 6, 10), (0,)), ((3, 4, 6, 10), (1,)), ((3, 4, 6, 10), (0, 2, 3)), ((3, 4, 6, 10), (-2,)), ((3, 4, 6, 10), (0, -1)),
           ((2, 3, 5, 6, 7), (1, 3, 4)), ((2, 3, 5, 6, 7), (0, 2)), ((3, 2, 5, 2, 3, 4), (0, 2, 4)), ((3, 2, 5, 2, 3, 4), (1, 3, 5)),
           ((70, 67), (0,)), ((300, 3, 129), (1,))]


@pytest.mark.parametrize("shape,dims", LAYOUTS, ids=lambda v: "x".join(map(str, v)))
def test_affine_and_rescale_are_the_row_kernels_on_a_transposed_copy(api, shape, dims):
    hl, utils = api.hl, api.utils
    x = seeded(shape, 21).cuda()
    xt, inverse = utils.dims_last(x, dims)
    assert inverse is not None
    groups = hl.group_segments(shape, dims)[2]
    inner = x.numel() // groups
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(groups, generator=g).cuda(), (torch.rand(groups, generator=g) + 0.5).cuda()
    for op in (0, 1):
        want = utils.dims_restore(hl.row_affine(op, xt, groups, inner, a, b), inverse)
        assert torch.equal(hl.group_affine(op, x, dims, a, b), want)
    # a missing operand is the identity one
    assert torch.equal(hl.group_affine(0, x, dims, a, None), hl.group_affine(0, x, dims, a, torch.ones_like(a)))
    assert torch.equal(hl.group_affine(0, x, dims, None, b), hl.group_affine(0, x, dims, torch.zeros_like(b), b))
    lo, hi = hl.group_stats(x, dims, mean_std=False, minmax=True)
    rlo, rhi = hl.minmax_rows(xt, groups, inner)
    assert torch.equal(lo, rlo) and torch.equal(hi, rhi)
    for tmin, tmax in ((-3.5, 4.0), (0.1, 0.3)):
        want = utils.dims_restore(hl.minmax_rescale(xt, groups, inner, rlo, rhi, 1e-7, tmin, tmax), inverse)
        assert torch.equal(hl.group_minmax_rescale(x, dims, lo, hi, 1e-7, tmin, tmax), want)
    # in place
    y = x.clone()
    hl._check(hl.load().sonar_group_affine_f32(0, y.data_ptr(), *hl._segment_args(shape, dims)[0], a.data_ptr(), b.data_ptr(), y.data_ptr(),
                                               hl._stream()), "sonar_group_affine_f32")
    assert torch.equal(y, hl.group_affine(0, x, dims, a, b))


def test_group_adjust(api):
    v = torch.tensor([0.0, 1.0, 3.0, float("nan"), -1.0, 0.75], device="cuda")
    assert torch.equal(api.hl.group_adjust(0, v, -0.25).nan_to_num(9.0), (v * -0.25).nan_to_num(9.0))
    for k in (1.0, 0.5, -0.25, 1.0 / 3.0):
        t = (v - 1.0) * k + 1.0
        want = torch.where(t == 0, torch.full_like(t, 1e-07), t)
        got = api.hl.group_adjust(1, v, k)
        assert torch.equal(got.isnan(), want.isnan()) and bool(got[3].isnan()) and torch.equal(got.nan_to_num(9.0), want.nan_to_num(9.0))
    assert float(api.hl.group_adjust(1, v, 1.0)[0]) == float(torch.tensor(1e-07, dtype=torch.float32))  # std 0, multiplier 1: the 1e-07


@pytest.mark.parametrize("shape,dims", LAYOUTS, ids=lambda v: "x".join(map(str, v)))
def test_normalize_to_scale_is_the_transposed_route_bit_for_bit(api, shape, dims):
    hl, utils = api.hl, api.utils
    x = seeded(shape, 33).cuda()
    xt, inverse = utils.dims_last(x, dims)
    groups = hl.group_segments(shape, dims)[2]
    inner = x.numel() // groups
    lo, hi = hl.minmax_rows(xt, groups, inner)
    want = utils.dims_restore(hl.minmax_rescale(xt, groups, inner, lo, hi, 1e-07, -3.5, 4.0), inverse)
    assert torch.equal(utils.normalize_to_scale(x, -3.5, 4.0, dim=dims), want)


# ------------------------------------------------------------------------------------------------ the item against the reference
@pytest.fixture(scope="module")
def golden():
    from tests.conftest import GOLDEN

    g = np.load(f"{GOLDEN}/normalize_dims.npz", allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def planted_item(nz, stored):
    class PlantedNoise(nz.CustomNoiseItemBase):
        """Hands back the stored tensor in the dtype and on the device of the latent it was built for."""

        def make_noise_sampler(self, x, *args, **kwargs):
            planes = self.planes

            def noise_sampler(_s, _sn):
                return planes.to(device=x.device, dtype=x.dtype, copy=True)

            return noise_sampler

    return PlantedNoise(1.0, planes=stored)


def build_item(api, case, stored):
    chain = api.nz.CustomNoiseChain()
    chain.add(planted_item(api.nz, stored))
    return api.nz.NormalizeToScaleNoise(case["factor"], noise=chain, **cases.item_kwargs(case)).clone()


def parent_route(api, case, noise):
    """The route of the parent commit for trailing mean_dims / std_dims, composed here from rowstats + row_affine."""
    hl, utils = api.hl, api.utils

    def rows_inner(dims):
        n = len(dims) if len(dims) else noise.ndim
        inner = int(np.prod(noise.shape[noise.ndim - n:]))
        return noise.numel() // inner, inner

    if case["mode"] == "simple":
        noise = utils.normalize_to_scale(noise, cases.RANGE["min_negative_value"], cases.RANGE["max_positive_value"], dim=case["dims"])
    else:
        rows = noise.shape[0] if case["dims"] else 1
        noise = hl.signed_rescale(noise, rows, noise.numel() // rows, cases.RANGE["min_negative_value"], cases.RANGE["max_negative_value"],
                                  cases.RANGE["min_positive_value"], cases.RANGE["max_positive_value"])
    if case["mean_multiplier"] != 0:
        rows, inner = rows_inner(case["mean_dims"])
        mean, _ = hl.rowstats(noise, rows, inner)
        noise = hl.row_affine(0, noise, rows, inner, mean * case["mean_multiplier"], torch.ones_like(mean))
    if case["std_multiplier"] != 0:
        rows, inner = rows_inner(case["std_dims"])
        _, std = hl.rowstats(noise, rows, inner)
        adj = (std - 1.0) * case["std_multiplier"] + 1.0
        adj = torch.where(adj == 0, torch.full_like(adj, 1e-07), adj)
        noise = hl.row_affine(0, noise, rows, inner, torch.zeros_like(adj), adj)
    return utils.scale_noise(noise, case["factor"], normalized=bool(case["normalize"]))


def _is_trailing(dims, ndim):
    want = sorted(d % ndim for d in dims) if len(dims) else list(range(ndim))
    return want == list(range(ndim - len(want), ndim))


@pytest.mark.filterwarnings("ignore:std\\(\\)")
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_item_against_the_reference(api, golden, name):
    """Every case of the golden file through make_noise_sampler on the device.  Refusals by exception type; the batch-1 case all NaN as in
    the reference; cases whose two reductions are both trailing also bit for bit against the parent commit's route."""
    g, meta = golden
    case, m = cases.CASES[name], meta[name]
    assert all(m[k] == (list(v) if isinstance(v, tuple) else v) for k, v in case.items()), "the golden file is older than the case table"
    stored = torch.from_numpy(g[f"planes_{case['latent']}"])
    x = torch.zeros(cases.LATENTS[case["latent"]], device="cuda")
    if case["error"]:
        with pytest.raises({"RuntimeError": RuntimeError, "IndexError": IndexError}[case["error"]]) as caught:
            build_item(api, case, stored).make_noise_sampler(x, 0.03, 14.6, seed=0, cpu=True, normalized=True)(*SIG)
        assert type(caught.value).__name__ == m["reference_error"]["type"]
        return
    got = build_item(api, case, stored).make_noise_sampler(x, 0.03, 14.6, seed=0, cpu=True, normalized=True)(*SIG)
    want = torch.from_numpy(g[f"out_{name}"])
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    if case["all_nan"]:
        assert bool(want.isnan().all()) and bool(got.isnan().all())
        torch.testing.assert_close(got.cpu(), want, rtol=0, atol=0, equal_nan=True)
        return
    print(f"{name}: max |error| {float((got.cpu() - want).abs().max()):.3e} of {2e-6 * float(want.abs().max()) + 2e-6:.3e}")
    torch.testing.assert_close(got.cpu(), want, rtol=0, atol=2e-6 * float(want.abs().max()) + 2e-6)
    if _is_trailing(case["mean_dims"], x.ndim) and _is_trailing(case["std_dims"], x.ndim):
        assert torch.equal(got, parent_route(api, case, stored.cuda()))


def test_the_table_has_trailing_cases_for_the_parent_route():
    both = [n for n, c in cases.CASES.items() if not c["error"] and _is_trailing(c["mean_dims"], 4) and _is_trailing(c["std_dims"], 4)]
    assert "a_l4_m3_m2_m1" in both and "a_l4_all" in both


# ------------------------------------------------------------------------------------------------ plan replay
def _planned_chain(api, x, **kw):
    nz = api.nz
    inner = nz.CustomNoiseChain()
    inner.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    case = dict(cases.CASES["c_simple_0_2_3"], **kw)
    outer = nz.CustomNoiseChain()
    outer.add(nz.NormalizeToScaleNoise(case["factor"], noise=inner, **cases.item_kwargs(case)))
    return outer.make_noise_sampler(x, 0.03, 14.6, seed=None, cpu=False, normalized=True)


def _calls(api, ns, n, plans):
    hl = api.hl
    old, hl.PLANS_ENABLED = hl.PLANS_ENABLED, plans
    try:
        torch.manual_seed(4321)
        return [ns(*SIG).clone() for _ in range(n)]
    finally:
        hl.PLANS_ENABLED = old


@pytest.mark.parametrize("kw", [dict(), dict(dims=cases.TRAILING, mean_dims=(0,), std_dims=(1, 3), normalize=True, factor=0.7),
                                dict(mean_multiplier=0.0, std_multiplier=-0.25)], ids=["node_form", "own_dims_normalised", "std_only"])
def test_a_replayed_step_with_non_trailing_dims_is_the_plain_call(api, kw):
    """Nine calls with plans (two ordinary, one traced, six replayed) == nine ordinary calls from the same RNG position, bit for bit: the
    simple mode with non-trailing reductions issues nothing but replayable entry points."""
    x = torch.zeros(3, 4, 16, 24, device="cuda")
    a, b = _planned_chain(api, x, **kw), _planned_chain(api, x, **kw)
    with_plans, plain = _calls(api, a, 9, True), _calls(api, b, 9, False)
    assert all(torch.equal(p, q) for p, q in zip(with_plans, plain))
    assert not torch.equal(plain[0], plain[1])
    assert isinstance(a, api.hl.Planned) and a.plan is not None, getattr(a, "reason", "no Planned wrapper")
    assert a.plan.runs == 6


def test_trailing_dims_and_the_advanced_mode_are_not_offered_to_the_planner(api):
    """Their steps hold torch operations (the trailing route's per-row operands) or an entry point outside the replayable set."""
    x = torch.zeros(3, 4, 16, 24, device="cuda")
    for kw in (dict(mean_dims=cases.TRAILING, std_dims=cases.TRAILING), dict(mode="advanced", dims=cases.TRAILING)):
        ns = _planned_chain(api, x, **kw)
        assert not isinstance(ns, api.hl.Planned)
        assert ns(*SIG).shape == x.shape
