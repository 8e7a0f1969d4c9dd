"""-m gpu: csrc/bislerp.hip (``sonar_bislerp_acc_f32``), ``utils.bislerp``, the ``scale_samples`` switch and the four bislerp presets
against the fp64 statement of the definition (tests/bislerp_refs.py).

**Parity unpinned.**  The reference reaches bislerp through ComfyUI's ``common_upscale``; ComfyUI is neither vendored by the reference nor
installed where these tests run, so there are no goldens: the statement is what is built and what is tested.

Tolerance (worked out, not picked): the statement in fp32 (torch CPU, same formulae) against the statement in fp64 over the kernel cases
below differs by at most 1.2e-05 relative to the summed norms of the four source vectors a pixel reads (the worst pixels are the nearly
opposite pairs, where sin(om) is small); the kernel's bound is four times the figure the run measures (4.9e-05) -- the margin covers the
device's sin / acos / division and another summation order over the channels.  Measured on an MI355X: the kernel's largest error is
4.4e-05 (40x24 -> 64x72 at C = 3, one nearly opposite pair: 89 % of the bound); every other case stays below 3.3e-06, the known-value
inputs below 2.8e-08.  The negative control (a statement that takes the linear mix where slerp belongs, 2x3 -> 7x5 at C = 4) is 0.15
away from the kernel, three thousand bounds.

The definition jumps where a dot crosses 1 - 1e-5 or 1e-5 - 1.  A pixel for which any of the statement's three fp64 dots lies within 2e-6
of a threshold is left out of a comparison, at most 0.5 % of a case's pixels; the kernel cases' seeds leave out none
(tests/test_bislerp_cpu.py asserts that)."""
import importlib
import types

import pytest
import torch

from tests import bislerp_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIG = (torch.tensor(14.6), torch.tensor(10.0))
GUARD = 64
PRESETS = ("pyramid_bislerp", "highres_pyramid_bislerp", "pyramid_old_bislerp", "pyramid_mix_bislerp")
LATENTS = ((2, 4, 12, 20), (1, 4, 2, 12, 8))


@pytest.fixture(scope="module")
def api(pkg):
    pkg.hip_lib.load()
    mods = {m: importlib.import_module(f"comfyui_sonar_amd.py.{m}") for m in ("utils", "noise_generation", "noise")}
    return types.SimpleNamespace(**mods, hl=pkg.hip_lib)


@pytest.fixture(scope="module")
def bound():
    b = R.kernel_bound()
    print(f"fp32 statement error {R.fp32_statement_error():.3e}, kernel bound {b:.3e}")
    return b


def run_kernel(hl, src, H, W, scale, base=None, partials=None):
    """``bislerp_acc_`` into a tensor that sits between NaN guards; accumulate onto ``base`` when given, else over a NaN-prefilled dst."""
    N, C = src.shape[:2]
    n = N * C * H * W
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    dst = buf[GUARD:GUARD + n].view(N, C, H, W)
    if base is not None:
        dst.copy_(base)
    hl.bislerp_acc_(dst, src.to(DEV), scale, base is not None, partials)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "the kernel wrote outside dst"
    return dst


def check(got, src, H, W, bound, scale=1.0, base=None, mutated=False):
    """The largest error of ``got`` against the statement, relative to the source norms (times |scale|), over the pixels that are compared."""
    want, dots = R.bislerp(src, W, H, mutated=mutated)
    want = want * scale + (0.0 if base is None else base.detach().cpu().double())
    out = R.near_threshold(dots)
    assert float(out.double().mean()) <= R.LEFT_OUT_CAP
    assert bool(torch.isfinite(got).all())
    return R.rel_error(got, want, R.source_scale(src, W, H) * abs(scale), ~out)


def check_partials(hl, part, dst):
    tot = part.view(hl.NPART, 2).sum(0).cpu()  # every pair: the slots no workgroup owns are zeroed by the kernel
    d = dst.double()
    assert abs(float(tot[0]) - float(d.sum())) < 1e-7 * d.numel() and abs(float(tot[1]) - float((d * d).sum())) < 1e-7 * d.numel()


# ------------------------------------------------------------------------------------------------ the kernel against the statement
@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("index", range(len(R.SIZES)), ids=[f"{h}x{w}-{H}x{W}" for (h, w), (H, W) in R.SIZES])
def test_kernel_against_the_statement(api, bound, index, C):
    hl = api.hl
    src, base, (H, W) = R.case_input(index, C)
    worst = 0.0
    for with_partials in (False, True):
        for accumulate in (True, False):
            part = torch.full((hl.NPART * 2,), float("nan"), dtype=torch.float64, device=DEV) if with_partials else None
            got = run_kernel(hl, src, H, W, R.ACC_SCALE if accumulate else 1.0, base if accumulate else None, part)
            err = check(got, src, H, W, bound, R.ACC_SCALE if accumulate else 1.0, base if accumulate else None)
            worst = max(worst, err)
            if with_partials:
                check_partials(hl, part, got)
    print(f"case {index} C={C}: kernel error {worst:.3e} of bound {bound:.3e}")
    assert worst <= bound


@pytest.mark.parametrize("name", sorted(R.known_inputs()))
def test_known_value_inputs_on_the_device(api, bound, name):
    src, W, H = R.known_inputs()[name]
    got = run_kernel(api.hl, src, H, W, 1.0)
    err = check(got, src, H, W, bound)
    print(f"{name}: kernel error {err:.3e} of bound {bound:.3e}")
    assert err <= bound
    if name == "identical":  # the dot > 1 - 1e-5 branch copies b1
        assert torch.equal(got.cpu(), src[0, :, 0, 0].reshape(1, -1, 1, 1).expand_as(got))


def test_the_table_cache_holds_one_entry_per_axis_and_device(api):
    hl = api.hl
    a = hl.bislerp_tables(7, 13, DEV)
    assert hl.bislerp_tables(7, 13, torch.device("cuda", torch.cuda.current_device())) is a
    want = R.axis_tables(7, 13)
    assert a[0].dtype == a[1].dtype == torch.int32 and all(t.is_cuda for t in a)
    assert torch.equal(a[0].cpu().long(), want[0]) and torch.equal(a[1].cpu().long(), want[1]) and torch.equal(a[2].cpu(), want[2])


# ------------------------------------------------------------------------------------------------ utils.bislerp / scale_samples
@pytest.mark.parametrize("kind", ["float16", "bfloat16", "channels_last", "strided"])
def test_utils_bislerp_dtypes_and_layouts(api, bound, kind):
    g = torch.Generator().manual_seed(7300)
    src = torch.randn(2, 4, 9, 7, generator=g)
    if kind in ("float16", "bfloat16"):
        x = src.to(getattr(torch, kind))
    elif kind == "channels_last":
        x = src.contiguous(memory_format=torch.channels_last)
    else:
        x = torch.randn(2, 4, 9, 14, generator=g)[..., ::2]
    wide = x.float()  # the statement runs on the widened input
    got = api.utils.bislerp(x.to(DEV), 12, 15)
    assert got.dtype == x.dtype and tuple(got.shape) == (2, 4, 15, 12) and got.is_cuda
    want, dots = R.bislerp(wide, 12, 15)
    keep = ~R.near_threshold(dots)
    assert float((~keep).double().mean()) <= R.LEFT_OUT_CAP
    scale = R.source_scale(wide, 12, 15)
    if x.dtype == torch.float32:
        assert R.rel_error(got, want, scale, keep) <= bound
    else:  # rounded once: the fp32 result (within the bound of the statement) cast to the input's dtype
        eps = torch.finfo(x.dtype).eps
        err = (got.cpu().double() - want).abs().amax(dim=1)
        allowed = bound * scale + 0.5 * eps * want.abs().amax(dim=1) * (1 + 1e-3) + float(torch.finfo(x.dtype).tiny)
        assert bool((err <= allowed)[keep].all())


def test_scale_samples_takes_bislerp_only_with_the_switch(api):
    utils = api.utils
    x = torch.randn(2, 4, 6, 5, generator=torch.Generator().manual_seed(7301)).to(DEV)
    before = utils.BISLERP_IN_SCALE_SAMPLES
    try:
        utils.BISLERP_IN_SCALE_SAMPLES = False
        with pytest.raises(NotImplementedError):
            utils.scale_samples(x, 9, 8, mode="bislerp")
        utils.BISLERP_IN_SCALE_SAMPLES = True
        assert torch.equal(utils.scale_samples(x, 9, 8, mode="bislerp"), utils.bislerp(x, 9, 8))
    finally:
        utils.BISLERP_IN_SCALE_SAMPLES = before


# ------------------------------------------------------------------------------------------------ the presets end to end
def samplers(api):
    """name -> factory(x, seed, cpu, normalized) for the four presets and the advanced node's item"""
    nz = api.noise
    out = {name: (lambda x, seed, cpu, normalized, name=name: nz.get_noise_sampler(name, x, 0.03, 14.6, seed=seed, cpu=cpu, factor=1.0,
                                                                                   normalized=normalized)) for name in PRESETS}
    out["advanced_pyramid"] = lambda x, seed, cpu, normalized: nz.AdvancedPyramidNoise(
        1.0, variant="pyramid", discount=0.6, iterations=4, upscale_mode="bislerp").make_noise_sampler(x, 0.03, 14.6, seed=seed, cpu=cpu,
                                                                                                        normalized=normalized)
    return out


NAMES = PRESETS + ("advanced_pyramid",)


@pytest.mark.parametrize("shape", LATENTS, ids=["4d", "5d"])
@pytest.mark.parametrize("name", NAMES)
def test_presets_replay_against_the_statement(api, bound, monkeypatch, name, shape):
    """Replay mode: every level a preset resamples goes through ``bislerp_acc_``; each call is held to the statement on the very draws it
    was handed (captured at the call: what dst held, the level, the weight), and for the generators that only sum levels the result is
    the last call's dst -- the statement composed with the same host draws."""
    hl = api.hl
    calls = []
    real = hl.bislerp_acc_

    def spy(dst, src, scale, accumulate=True, partials=None):
        before = dst.detach().clone()
        out = real(dst, src, scale, accumulate, partials)
        calls.append((before.cpu(), src.detach().cpu().clone(), float(scale), bool(accumulate), dst.detach().cpu().clone()))
        return out

    monkeypatch.setattr(hl, "bislerp_acc_", spy)
    x = torch.zeros(shape, device=DEV)
    torch.manual_seed(71)
    got = samplers(api)[name](x, 71, True, False)(*SIG)
    assert got.is_cuda and tuple(got.shape) == tuple(shape) and bool(torch.isfinite(got).all())
    channels = shape[1] * (shape[2] if len(shape) == 5 else 1)  # frames fold into the channels: the slerp runs over all of them
    assert len(calls) >= 2
    for before, src, scale, accumulate, after in calls:
        assert tuple(src.shape[:2]) == (shape[0], channels) and accumulate
        H, W = after.shape[-2:]
        assert check(after, src, H, W, bound, scale, before) <= bound
    if name in ("pyramid_bislerp", "pyramid_old_bislerp", "highres_pyramid_bislerp", "advanced_pyramid"):
        assert torch.equal(got.cpu().reshape(calls[-1][4].shape), calls[-1][4])


@pytest.mark.parametrize("shape", LATENTS, ids=["4d", "5d"])
@pytest.mark.parametrize("name", NAMES)
def test_presets_generate_mode_is_finite_and_repeatable(api, name, shape):
    x = torch.zeros(shape, device=DEV)

    def gen(normalized):
        torch.manual_seed(9)
        return samplers(api)[name](x, None, False, normalized)(*SIG)

    a, b = gen(False), gen(False)
    assert a.is_cuda and tuple(a.shape) == tuple(shape) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    n = gen(True)
    assert bool(torch.isfinite(n).all()) and torch.equal(n, gen(True))
    assert abs(float(n.std()) - 1.0) < 0.1  # the sampler's normalisation (it leaves alone what is within 2.5 / sqrt(n) already)


@pytest.mark.parametrize("name", ["pyramid_bislerp", "pyramid_old_bislerp", "advanced_pyramid"])
def test_batch_shards_equal_the_unsharded_call(api, name):
    """Device draws are keyed by the global latent: two shards under ``shard_offset`` are the whole call's halves, bit for bit (the other
    two presets normalise parts per call tensor -- shards differ by design, as for their bilinear forms)."""
    ng = api.noise_generation

    def gen(b0, b):
        torch.manual_seed(9)
        with ng.shard_offset(b0):
            x = torch.zeros((b, 4, 12, 20), device=DEV)
            return samplers(api)[name](x, None, False, False)(*SIG)

    whole = gen(0, 4)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(torch.cat([gen(0, 2), gen(2, 2)]), whole)


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_a_prepared_plan_replays_the_ordinary_bits_or_declines(api, name, normalized):
    hl = api.hl
    x = torch.zeros((2, 4, 12, 20), device=DEV)

    def run(plans):
        ns = samplers(api)[name](x, 5, False, normalized)
        old = hl.PLANS_ENABLED
        hl.PLANS_ENABLED = plans
        try:
            torch.manual_seed(4321)
            return [ns(*SIG).clone() for _ in range(6)], ns
        finally:
            hl.PLANS_ENABLED = old

    (with_plans, ns), (without, _) = run(True), run(False)
    for p, q in zip(with_plans, without):
        assert torch.equal(p, q)
    planned = ns if isinstance(ns, hl.Planned) else getattr(ns, "_planned", None)
    if planned is not None and planned.plan is None and planned.attempts:
        assert planned.reason  # declined, and says why
