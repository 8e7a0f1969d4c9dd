"""-m gpu: reductions over any dims on the tensor as it lies (csrc/group_stats.hip) behind PowerLawNoiseGenerator's ``div_max_dims`` and
scale_noise's ``normalize_dims``, against tests/golden/reduce_dims.npz (the reference's outputs; tests/golden/reduce_dims_cases.py).

Tolerances.
  power law   The value before the division is held to the existing power-law golden test's bound for ``hip_lib.powerlaw_`` (rtol 2e-5,
              atol 5e-6: tests/test_gpu_rows_next.py).  The division is exact: the output equals the test's own copy of the pre-division
              tensor divided by its amax in torch, bit for bit, and it equals the reference's output bit for bit wherever the kernel's
              pre-division value and the group's peak are the reference's (both stored in the fixture: torch's CPU pow is not the same on
              every machine, so the test does not recompute it).
  scale_noise atol = 2e-6 * max|want| + 2e-6, rtol 0: what tests/test_gpu_group_stats.py gives the row kernels against the normalize_dims
              golden (the golden script shows the reference's own float32 output to meet it against float64).  And bit for bit the parent
              commit's route, built here from dims_last + scale_noise_rows_ + dims_restore.  scale_noise keeps that route for one family of
              layouts (hip_lib.group_scale_noise_slow), so every case also runs the strided kernels directly."""
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
import reduce_dims_cases as cases  # noqa: E402

SIG = (torch.tensor(cases.SIGMA[0]), torch.tensor(cases.SIGMA[1]))


@pytest.fixture(scope="module")
def api(pkg):
    pkg.hip_lib.load()
    mods = {m: importlib.import_module(f"comfyui_sonar_amd.py.{m}") for m in ("utils", "noise_generation", "noise")}
    return types.SimpleNamespace(hl=pkg.hip_lib, registry=importlib.import_module("comfyui_sonar_amd.py.nodes.registry"), **mods)


@pytest.fixture(scope="module")
def fixture_file():
    from tests.conftest import GOLDEN

    g = np.load(f"{GOLDEN}/reduce_dims.npz", allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def dims_of(case):
    return cases.DIMS[case["latent"]][case["dims"]]


def powerlaw_sampler(api, case, x, **kw):
    torch.manual_seed(cases.SEED)
    return api.noise.get_noise_sampler("grey", x, 0.03, 14.6, seed=cases.SEED, cpu=True, factor=1.0, normalized=False, alpha=case["alpha"],
                                       div_max_dims=dims_of(case), use_sign=case["use_sign"], use_div_max_abs=case["use_div_max_abs"], **kw)


def peak_of(pre, case):
    return torch.amax(pre.abs() if case["use_div_max_abs"] else pre, dim=tuple(dims_of(case)), keepdim=True)


# ------------------------------------------------------------------------------------------------ power law
@pytest.mark.parametrize("name", sorted(cases.POWERLAW))
def test_powerlaw_over_any_dims_against_the_reference(api, fixture_file, name):
    g, _meta = fixture_file
    case = cases.POWERLAW[name]
    draw, want = torch.from_numpy(g[f"draw_{case['latent']}"]), torch.from_numpy(g[f"pl_{name}"])
    got = powerlaw_sampler(api, case, torch.zeros(draw.shape, device="cuda"))(*SIG)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    got = got.cpu()
    # before the division: the kernel of the existing golden test, at its tolerance
    pre = api.hl.powerlaw_(draw.cuda(), case["alpha"], case["use_sign"]).cpu()
    ref_pre = torch.from_numpy(g[cases.pre_key(case)])  # the reference's own float32 pow, as the machine that wrote the fixture computed it
    print(f"{name}: pre-division max |error| {float((pre - ref_pre).abs().max()):.3e}")
    torch.testing.assert_close(pre, ref_pre, rtol=2e-5, atol=5e-6)
    # the division itself: exact
    peak = peak_of(pre, case)
    torch.testing.assert_close(got, pre / peak, rtol=0, atol=0)
    # ... and so the reference's bits wherever its pow and the kernel's agree (for the element and for its group's peak)
    agree = (pre == ref_pre) & (peak == peak_of(ref_pre, case))
    print(f"{name}: pow agrees on {float(agree.float().mean()):.4f} of the elements")
    assert bool(agree.any())
    torch.testing.assert_close(got[agree], want[agree], rtol=0, atol=0)
    assert bool(got.isfinite().all())


def test_a_nan_member_reaches_its_own_group_only(api):
    """torch.amax propagates a NaN; both sweeps (a lane per group, a wave per group) and the split route do."""
    for shape, dims, at in (((3, 5, 6, 7), (0, 2), (1, 2, 3, 4)), ((3, 5, 6, 7), (1, 3), (2, 1, 4, 6)), ((2049, 3, 7), (0,), (2000, 1, 5)),
                            ((2, 3, 3000), (0, 2), (1, 2, 2999))):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(3))
        x[at] = float("nan")
        for use_abs in (False, True):
            got = api.hl.group_peak(x.cuda(), dims, use_abs).cpu()
            want = torch.amax(x.abs() if use_abs else x, dim=dims, keepdim=True).flatten()
            assert int(got.isnan().sum()) == 1 and torch.equal(got.isnan(), want.isnan())
            assert torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))


def test_a_zero_peak_gives_what_torch_gives(api):
    x = torch.randn(3, 5, 6, 7, generator=torch.Generator().manual_seed(4))
    x[:, 1, :, 2] = 0.0  # one whole group of dims (0, 2)
    d = api.hl.group_peak(x.cuda(), (0, 2), True)
    got = api.hl.group_div_(x.cuda(), (0, 2), d).cpu()
    want = x / x.abs().amax(dim=(0, 2), keepdim=True)
    assert bool(got[:, 1, :, 2].isnan().all()) and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))


@pytest.mark.parametrize("name", ["s4_02_a2", "s4_13_a05_sign", "s5_024_a05_sign", "big_13_a05_sign"])
def test_the_advanced_item_and_the_yaml_node_take_the_same_route(api, fixture_file, name):
    """SonarAdvancedPowerLawNoise's socket only names adjacent choices; its item takes any tuple, and SonarCustomNoiseAdv takes a yaml list."""
    case = cases.POWERLAW[name]
    assert case["use_div_max_abs"]  # (the item does not forward use_div_max_abs: the generator's default)
    shape = cases.SHAPES[case["latent"]]
    x = torch.zeros(shape, device="cuda")
    want = powerlaw_sampler(api, case, x)(*SIG)
    item = api.noise.AdvancedPowerLawNoise(1.0, alpha=case["alpha"], div_max_dims=tuple(dims_of(case)), use_sign=case["use_sign"],
                                           use_div_max_abs=True)
    torch.manual_seed(cases.SEED)
    assert torch.equal(item.make_noise_sampler(x, 0.03, 14.6, seed=cases.SEED, cpu=True, normalized=False)(*SIG), want)
    node = api.registry.NODE_CLASS_MAPPINGS["SonarCustomNoiseAdv"]()
    text = f"alpha: {case['alpha']}\ndiv_max_dims: {list(dims_of(case))}\nuse_sign: {str(case['use_sign']).lower()}\n"
    (chain,) = node.go(factor=1.0, rescale=0.0, noise_type="grey", yaml_parameters=text)
    torch.manual_seed(cases.SEED)
    got = chain.make_noise_sampler(x, 0.03, 14.6, seed=cases.SEED, cpu=True, normalized=False)(*SIG)
    api.utils.pop_stats(got)
    assert torch.equal(got, want)


def test_adjacent_dims_keep_amax_mid_and_div_mid(api, golden, monkeypatch):
    """One adjacent case of the existing golden (div_max_dims = 1): the parent commit's two kernels, its bits, and not the strided pair."""
    hl = api.hl
    g = golden("powerlaw")
    draw = g["draw"]
    calls = []
    real_amax, real_div = hl.amax_mid, hl.div_mid_
    monkeypatch.setattr(hl, "amax_mid", lambda *a: calls.append("amax_mid") or real_amax(*a))
    monkeypatch.setattr(hl, "div_mid_", lambda *a: calls.append("div_mid_") or real_div(*a))
    monkeypatch.setattr(hl, "group_peak", lambda *a: pytest.fail("adjacent dims went to the strided route"))
    torch.manual_seed(33)
    item = api.noise.AdvancedPowerLawNoise(1.0, alpha=1.2, div_max_dims=1, use_sign=True, use_div_max_abs=True)
    got = item.make_noise_sampler(torch.zeros(tuple(draw.shape), device="cuda"), 0.03, 14.6, seed=33, cpu=True, normalized=False)(*SIG)
    assert calls == ["amax_mid", "div_mid_"]
    b, c, h, w = draw.shape
    parent = hl.powerlaw_(draw.cuda(), 1.2, True)
    parent = real_div(parent, b, c, h * w, real_amax(parent, b, c, h * w, True))
    assert torch.equal(got, parent)
    torch.testing.assert_close(got.cpu(), g["adv_a12_channel"], rtol=2e-5, atol=5e-6)


def test_a_device_mode_step_with_non_adjacent_dims_is_replayable(api):
    ng = api.noise_generation
    x = torch.zeros(3, 4, 16, 24, device="cuda")
    ns = api.noise.get_noise_sampler("grey", x, 0.03, 14.6, seed=11, cpu=False, factor=1.0, normalized=False, alpha=2.0, div_max_dims=(0, 2))
    out, plan = api.hl.trace_plan(ns, SIG, take=ng.DeviceRNG.take, rewind=ng.DeviceRNG.rewind, guards=())
    assert plan is not None, api.hl.trace_plan.last_reason
    assert out.shape == x.shape and torch.equal(out.abs().amax(dim=(0, 2)).cpu(), torch.ones(4, 24))


# ------------------------------------------------------------------------------------------------ scale_noise
def scale_input(g, case):
    x = torch.from_numpy(g[f"draw_{case['latent']}"])
    return x + cases.offsets(torch, case["latent"], case["dims"]) if case["offset"] else x


def parent_route(api, x, dims, factor):
    """scale_noise(normalize_dims=dims) of the parent commit: the row kernel on a transposed copy."""
    rows_last, inverse = api.utils.dims_last(x, dims)
    assert inverse is not None
    inner = int(np.prod(rows_last.shape[x.ndim - len(dims):]))
    return api.utils.dims_restore(api.hl.scale_noise_rows_(rows_last, x.numel() // inner, inner, factor), inverse)


@pytest.mark.filterwarnings("ignore:std\\(\\)")
@pytest.mark.parametrize("name", sorted(cases.SCALE))
def test_scale_noise_over_any_dims_against_the_reference_and_the_parent_route(api, fixture_file, name):
    g, meta = fixture_file
    case, m = cases.SCALE[name], meta[f"sn_{name}"]
    want = torch.from_numpy(g[f"sn_{name}"])
    x = scale_input(g, case).cuda()
    parent = parent_route(api, x.clone(), dims_of(case), case["factor"])
    public = api.utils.scale_noise(x.clone(), case["factor"], normalized=True, normalize_dims=dims_of(case))
    got = api.hl.group_scale_noise_(x, dims_of(case), case["factor"])  # the strided kernels, whichever route scale_noise picks for the layout
    assert got.data_ptr() == x.data_ptr() and got.shape == want.shape  # in place
    if m["all_nan"]:
        assert bool(got.isnan().all()) and bool(parent.isnan().all()) and bool(public.isnan().all())
        return
    assert torch.equal(public, got)
    bound = 2e-6 * float(want.abs().max()) + 2e-6
    print(f"{name}: max |error| {float((got.cpu() - want).abs().max()):.3e} of {bound:.3e}")
    torch.testing.assert_close(got.cpu(), want, rtol=0, atol=bound)
    torch.testing.assert_close(got, parent, rtol=0, atol=0)
    if case["offset"]:  # groups on both sides of the mean threshold are there, and both kinds come out centred (the reference skips neither)
        flags = torch.from_numpy(g[f"flags_{name}"]).bool()
        assert bool(flags.any()) and not bool(flags.all())
        centred = got.cpu().double().mean(dim=tuple(dims_of(case)), keepdim=True).flatten().abs()
        assert float(centred[flags].max()) < 1e-6 and float(centred[~flags].max()) < 1e-6


@pytest.mark.parametrize("shape,dims", [((2049, 3, 7), (0,)), ((5, 3, 700), (0, 2)), ((40, 3, 5000), (0, 2)), ((3, 4, 6, 10), (0, -1))])
def test_scale_noise_on_the_split_route_is_the_parent_route(api, shape, dims):
    """Shapes whose reductions are cut into slices (few groups of many members), either kind innermost."""
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(8)) * 1.5 + 0.4).cuda()
    parent = parent_route(api, x.clone(), dims, 0.35)
    assert torch.equal(api.hl.group_scale_noise_(x.clone(), dims, 0.35), parent)
    assert torch.equal(api.utils.scale_noise(x, 0.35, normalized=True, normalize_dims=dims), parent)


def test_the_route_scale_noise_picks(api, monkeypatch):
    """The strided route, except where it was measured slower than the transposed copies: the innermost segment kept
    and fewer than 1024 groups."""
    hl = api.hl
    assert hl.group_scale_noise_slow((512, 4, 128, 128), (0, 2)) and not hl.group_scale_noise_slow((512, 4, 128, 128), (1, 3))
    assert not hl.group_scale_noise_slow((512, 4, 128, 128), (0,)) and not hl.group_scale_noise_slow((512, 4, 128, 128), (0, 2, 3))
    calls = []
    real = hl.group_scale_noise_
    monkeypatch.setattr(hl, "group_scale_noise_", lambda *a: calls.append(a[1]) or real(*a))
    for shape, dims, strided in (((3, 5, 6, 7), (1, 3), True), ((3, 5, 6, 7), (0, 2), False), ((2, 3, 8, 400), (0, 2), True)):
        x = torch.randn(shape, generator=torch.Generator().manual_seed(12)).cuda()
        del calls[:]
        api.utils.scale_noise(x, 1.0, normalized=True, normalize_dims=dims)
        assert bool(calls) == strided, (shape, dims)


def test_trailing_dims_keep_the_row_kernel(api, monkeypatch):
    hl = api.hl
    x = torch.randn(3, 5, 6, 7, generator=torch.Generator().manual_seed(9)).cuda()
    want = hl.scale_noise_rows_(x.clone(), 15, 42, 0.35)
    monkeypatch.setattr(hl, "group_scale_noise_", lambda *a: pytest.fail("trailing dims went to the strided route"))
    got = api.utils.scale_noise(x, 0.35, normalized=True, normalize_dims=(-2, -1))
    assert got.data_ptr() == x.data_ptr() and torch.equal(got, want)


def test_the_call_is_in_place_and_holds_no_torch_copy(api):
    """The trace recorder refuses a step that runs a torch kernel on a device tensor: the parent's route is refused for its transposed copies,
    the strided route is not."""
    hl, ng = api.hl, api.noise_generation
    x = torch.randn(3, 5, 6, 7, generator=torch.Generator().manual_seed(10)).cuda()
    ptr = x.data_ptr()
    _out, plan = hl.trace_plan(lambda _s, _sn: parent_route(api, x, (1, 3), 0.35), SIG, take=ng.DeviceRNG.take, rewind=ng.DeviceRNG.rewind, guards=())
    assert plan is None and "torch operation aten." in hl.trace_plan.last_reason
    out, plan = hl.trace_plan(lambda _s, _sn: api.utils.scale_noise(x, 0.35, normalized=True, normalize_dims=(1, 3)), SIG,
                              take=ng.DeviceRNG.take, rewind=ng.DeviceRNG.rewind, guards=())
    assert "torch operation" not in (hl.trace_plan.last_reason or "")
    assert out is x and out.data_ptr() == ptr and out.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
