"""GPU: utils.pattern_break and PatternBreakNoise (csrc/pattern_break.hip).

Every output is held to the fp64 statement of the filter (tests/pattern_break_refs.py) on the reference's own inputs, all elements, within
MARGIN x E x the case's output range, E being the fp32 statement's measured distance from the fp64 one (1.05e-7: the bound is 8.4e-7 of
the range).  The front half of the filter is chaotic -- a last-place error anywhere before erfinv moves outputs by more than 0.1 at many
elements -- so there is nothing between "within the bound" and "far outside".  The two routes are compared with torch.equal.  The item over
a gaussian base in replay mode goes through scale_noise; with normalized=True the chain tolerance of the node sweep is added (rtol = 4e-5,
atol = 4e-5 * max(1, peak))."""
import importlib

import numpy as np
import pytest
import torch

from tests import pattern_break_refs as R

cases = R.cases
pytestmark = pytest.mark.gpu
DEV = "cuda"
FUNCTION_CASES = cases.function_cases()
SIG = (torch.tensor(10.0), torch.tensor(5.0))


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def st():
    return R.statements()


def _kw(nz, p, d, r, m):
    return dict(percentage=p, detail_level=d, restore_scale=r, blend_function=nz.utils.BLENDING_MODES[m])


def _within(got, s64, scale, E, what):
    worst = float(np.abs(got.astype(np.float64) - s64).max())
    print(f"{what}: {worst / scale:.3e} of the range (bound {R.MARGIN * E:.3e})")
    assert np.isfinite(got).all() and worst <= R.MARGIN * E * scale, (what, worst, R.MARGIN * E * scale)


# ------------------------------------------------------------------------------------------------ 1. the function against the reference
@pytest.mark.parametrize("case", FUNCTION_CASES, ids=lambda c: c[0])
def test_function_goldens_within_the_bound(nz, st, case):
    name, inp, p, d, r, m = case
    want, _s32, s64, scale = st["table"][name]
    x = torch.from_numpy(st["g"][f"in_{inp}"]).to(DEV)
    before = x.clone()
    out = nz.utils.pattern_break(x, **_kw(nz, p, d, r, m))
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape and out.data_ptr() != x.data_ptr() and torch.equal(x, before)
    got = out.cpu().numpy()
    _within(got, s64, scale, st["E"], name)
    _within(got, want.astype(np.float64), scale, st["E"], name + " against the reference's output")


def test_both_routes_give_the_same_bits(nz, st):
    for name, inp, p, d, r, m in FUNCTION_CASES:
        x = torch.from_numpy(st["g"][f"in_{inp}"]).to(DEV)
        one, three = (nz.utils.pattern_break(x, route=route, **_kw(nz, p, d, r, m)) for route in ("one", "three"))
        assert torch.equal(one, three), name
        assert torch.equal(nz.utils.pattern_break(x, **_kw(nz, p, d, r, m)), one), name


def test_route_threshold_grid_stride_and_alignment(pkg, nz, st):
    """Sizes on both sides of the one-launch threshold (the default route is the forced one's bits), a tensor of more values than one sweep
    of the three-launch grid covers (512 workgroups x 2048), and views that start off a 16-byte boundary: together with `out` (a scalar
    head, 16-byte groups, a scalar tail) and against it (every element through the scalar loop)."""
    hl = pkg.hip_lib
    lib = hl.load()
    limit = next(n for n in (1 << k for k in range(8, 26)) if lib.sonar_pattern_break_route(n + 1) == 2)
    assert lib.sonar_pattern_break_route(limit) == 1
    g = torch.Generator().manual_seed(9)
    for n in (limit, limit + 1, 512 * 2048 * 2 + 5):
        x = torch.randn(n, generator=g)
        s64 = R.pattern_break(x.numpy(), dtype=np.float64)
        xd = x.to(DEV)
        one, three, auto = (nz.utils.pattern_break(xd, route=route) for route in ("one", "three", None))
        assert torch.equal(one, three) and torch.equal(auto, one)
        _within(three.cpu().numpy(), s64, R.out_range(s64), st["E"], f"n = {n}")
    n = 4488
    base = torch.from_numpy(st["g"]["in_g4488"]).flatten().to(DEV)
    want = nz.utils.pattern_break(base)
    for shift in (1, 2, 3):
        buf = torch.zeros(n + 8, device=DEV)
        buf[shift:shift + n] = base
        x = buf[shift:shift + n]
        assert x.data_ptr() % 16 == 4 * shift
        for route in ("one", "three"):
            assert torch.equal(nz.utils.pattern_break(x, route=route), want)            # a fresh, aligned `out`: no 16-byte groups in common
            obuf = torch.full((n + 8,), -7.0, device=DEV)
            out, _ = hl.pattern_break(x, 1.0, 0.5, "lerp", True, route=route, out=obuf[shift:shift + n])
            assert torch.equal(out, want) and bool((obuf[:shift] == -7).all()) and bool((obuf[shift + n:] == -7).all())


def test_nan_stays_where_it_is_and_never_wins_the_extremes(nz, st):
    x = st["g"]["in_g4488"].copy()
    x.ravel()[[5, 4000]] = np.nan
    s64 = R.pattern_break(x, dtype=np.float64)
    for route in ("one", "three"):
        got = nz.utils.pattern_break(torch.from_numpy(x).to(DEV), route=route).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(x))
        ok = ~np.isnan(x)
        _within(got[ok], s64[ok], R.out_range(s64), st["E"], f"NaN input, route {route}")


# ------------------------------------------------------------------------------------------------ 2. the item, replay mode
@pytest.mark.parametrize("name", list(cases.ITEMS))
def test_item_goldens(nz, st, name):
    factor, normalized, kw = cases.ITEMS[name]
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.PatternBreakNoise(factor, noise=chain, **kw).clone()
    torch.manual_seed(cases.ITEM_GLOBAL_SEED)
    ns = item.make_noise_sampler(torch.zeros(cases.ITEM_LATENT, device=DEV), cases.SIGMA_MIN, cases.SIGMA_MAX, seed=cases.ITEM_SEED, cpu=True,
                                 normalized=normalized)
    want = torch.from_numpy(st["g"][f"item_{name}"])
    for i, (s, sn) in enumerate(cases.ITEM_SIGMAS):
        got = ns(torch.tensor(s), torch.tensor(sn))
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == cases.ITEM_LATENT
        w = want[i]
        bound = R.MARGIN * st["E"] * R.out_range(w.numpy())
        worst = float((got.cpu() - w).abs().max())
        print(f"{name} call {i}: {worst:.3e} (filter bound {bound:.3e})")
        if normalized:
            torch.testing.assert_close(got.cpu(), w, rtol=4e-5, atol=4e-5 * max(1.0, float(w.abs().max())) + bound)
        else:
            assert worst <= bound, (name, i, worst, bound)


# ------------------------------------------------------------------------------------------------ 3. dtypes and layouts
def test_half_precision_and_channels_last_agree_with_float32(nz, st):
    x = torch.from_numpy(st["g"]["in_g4488"]).to(DEV)
    for dtype in (torch.float16, torch.bfloat16):
        xh = x.to(dtype)
        out = nz.utils.pattern_break(xh, percentage=0.25, detail_level=3.5)
        assert out.dtype == dtype and out.shape == x.shape
        assert torch.equal(out, nz.utils.pattern_break(xh.float(), percentage=0.25, detail_level=3.5).to(dtype))  # one rounding of the fp32 result
    cl = x.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    out = nz.utils.pattern_break(cl, restore_scale=False)
    assert out.shape == x.shape and torch.equal(out, nz.utils.pattern_break(x, restore_scale=False))
    assert out.is_contiguous(memory_format=torch.channels_last)  # the input's layout
    t = x.transpose(2, 3)
    assert torch.equal(nz.utils.pattern_break(t), nz.utils.pattern_break(t.contiguous()))


# ------------------------------------------------------------------------------------------------ 4. statistics hand-off, no host read
def test_the_output_carries_its_statistics_for_scale_noise(pkg, nz, st, monkeypatch):
    hl, utils = pkg.hip_lib, nz.utils
    x = torch.from_numpy(st["g"]["in_g64k"]).to(DEV)
    sweeps = []
    real = hl.stats
    monkeypatch.setattr(hl, "stats", lambda *a, **k: (sweeps.append(1), real(*a, **k))[1])
    for route in ("one", "three"):
        out = utils.pattern_break(x, route=route)
        assert getattr(out, hl.STATS_ATTR, None) is not None
        partials = getattr(out, hl.STATS_ATTR)[0]
        o64 = out.double()
        torch.testing.assert_close(partials.view(-1, 2).sum(0), torch.stack((o64.sum(), (o64 * o64).sum())), rtol=1e-12, atol=1e-9)
        plain = out.clone()                       # a copy carries no tag: the statistics kernel runs
        del sweeps[:]
        a = utils.scale_noise(out, 0.7, normalized=True)
        assert not sweeps and a.data_ptr() == out.data_ptr()
        b = utils.scale_noise(plain, 0.7, normalized=True)
        assert len(sweeps) == 1
        torch.testing.assert_close(a, b, rtol=2e-6, atol=2e-6)  # the two summation orders: fp64 sums, a few fp32 roundings of mean and std
    # a float32 input in another layout: the result is a copy into that layout, the statistics do not depend on the order and stay with it
    cl = torch.from_numpy(st["g"]["in_g4488"]).to(DEV).contiguous(memory_format=torch.channels_last)
    out = utils.pattern_break(cl)
    tag = getattr(out, hl.STATS_ATTR, None)
    assert tag is not None
    o64 = out.double()
    torch.testing.assert_close(tag[0].view(-1, 2).sum(0), torch.stack((o64.sum(), (o64 * o64).sum())), rtol=1e-12, atol=1e-9)
    # other dtypes are rounded after the statistics were taken: no tag
    assert getattr(utils.pattern_break(cl.half()), hl.STATS_ATTR, None) is None


def test_no_host_synchronisation_inside_the_call(nz, st):
    x = torch.from_numpy(st["g"]["in_g4488"]).to(DEV)
    nz.utils.pattern_break(x)  # the library is loaded, the allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [nz.utils.pattern_break(x, route=route, **_kw(nz, 0.5, 3.5, r, "inject")) for route in ("one", "three") for r in (True, False)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    torch.cuda.set_sync_debug_mode("error")  # the idiom does see a read-back: the reference's own first step
    try:
        with pytest.raises(RuntimeError):
            x.min().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ------------------------------------------------------------------------------------------------ 5. refusals, before any launch
def test_refusals_leave_the_output_untouched(pkg, nz):
    hl = pkg.hip_lib
    lib = hl.load()
    x = torch.randn(1000, device=DEV)
    out = torch.full_like(x, -1.0)
    ws = torch.zeros(hl.PATTERN_BREAK_WS, device=DEV)
    stats = hl.new_partials(DEV)
    st_ = hl._stream()
    px, po, pw, ps = x.data_ptr(), out.data_ptr(), ws.data_ptr(), stats.data_ptr()
    fn = lib.sonar_pattern_break_f32
    W = hl.PATTERN_BREAK_WS

    def refused(*args):
        with pytest.raises(hl.SonarHipError):
            hl._check(fn(*args), "pattern_break")

    refused(None, po, 1000, 1.0, 0.5, 0, 1, 0, pw, W, ps, st_)
    refused(px, None, 1000, 1.0, 0.5, 0, 1, 0, pw, W, ps, st_)
    refused(px, po, 1000, 1.0, 0.5, 0, 1, 0, None, W, ps, st_)
    refused(px, px, 1000, 1.0, 0.5, 0, 1, 0, pw, W, ps, st_)
    refused(px, po + 2, 996, 1.0, 0.5, 0, 1, 0, pw, W, ps, st_)
    for n in (0, -1):
        refused(px, po, n, 1.0, 0.5, 0, 1, 0, pw, W, ps, st_)
    for mode in (-1, 3):
        refused(px, po, 1000, 1.0, 0.5, mode, 1, 0, pw, W, ps, st_)
    for route in (-1, 3):
        refused(px, po, 1000, 1.0, 0.5, 0, 1, route, pw, W, ps, st_)
    refused(px, po, 1000, 1.0, 0.5, 0, 1, 0, pw, W - 1, ps, st_)
    with pytest.raises(hl.SonarHipError):
        hl.pattern_break(x, 1.0, 0.5, "lerp", True, out=x)
    with pytest.raises(hl.SonarHipError):
        hl.pattern_break(x, 1.0, 0.5, "lerp", True, route="both", out=out)
    with pytest.raises(NotImplementedError):
        nz.utils.pattern_break(x, blend_function=torch.lerp)
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    with ng.shard_offset(1), pytest.raises(NotImplementedError, match="sharded batch"):
        nz.utils.pattern_break(x)
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    # without a statistics buffer the call runs and leaves no tag behind
    got, partials = hl.pattern_break(x, 1.0, 0.5, "lerp", True, want_stats=False)
    assert partials is None and torch.equal(got, nz.utils.pattern_break(x))
