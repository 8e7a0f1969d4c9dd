"""-m gpu: SonarCustomNoiseParameters.  The two tail kernels (csrc/noise_params.hip) against a float64 restatement of the reference's
fix / crop / scale_noise written here; the item through ``make_noise_sampler`` on the device in replay mode against the reference's own
outputs (tests/golden/noise_params.npz); the generate-mode RNG contract; prepared plans; the tail's launch count.

Tolerances.  Kernel level, float32 output: rtol 1e-5, atol 1e-6, the bound of the scale_noise parity test of tests/test_gpu_kernels.py
(the same arithmetic: float64 statistics, then subtract / divide / multiply in float32).  Half-precision outputs: the float64 reference
rounded to the dtype, within one ulp of it.  The cancellation case (2^20 + 3 values, mean 300, std 1) is held to the same bound: the
statistics are float64 and the mean is subtracted as two floats, so the float32 ulp of a value near 300 does not reach the result.
Item level: the node sweep's rtol = 4e-5, atol = 4e-5 * max(1, |want|max)."""
import importlib
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import noise_params_cases as cases  # noqa: E402

SIG = (torch.tensor(9.0), torch.tensor(6.0))
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def api(pkg):
    pkg.hip_lib.load()
    return types.SimpleNamespace(hl=pkg.hip_lib, nz=importlib.import_module("comfyui_sonar_amd.py.noise"),
                                 sonar=importlib.import_module("comfyui_sonar_amd.py.sonar"),
                                 reg=importlib.import_module("comfyui_sonar_amd.py.nodes.registry"))


# ------------------------------------------------------------------------------------------------ the float64 restatement (points 3-5)
def ref_tail(src: torch.Tensor, plane_out: int, fix: bool, normalized: bool, factor: float, margins=None) -> torch.Tensor:
    """src: [planes, plane_in] (any float dtype, on the CPU) -> float64 [planes, plane_out]."""
    t = src.double().clone()
    if fix:
        zeroed = t.nan_to_num(0.0, posinf=0.0, neginf=0.0)
        t = t.nan_to_num(0.0, posinf=float(zeroed.max()), neginf=float(zeroed.min()))
    t = t[:, :plane_out].contiguous()
    if normalized and t.numel():
        mean, std = float(t.mean()), float(t.std())
        thr = 2.5 / math.sqrt(t.numel())
        if margins is not None:
            margins.append((abs(abs(mean) - thr) / thr, abs(abs(1.0 - std) - thr) / thr))
        if abs(mean) > thr:
            t = t - mean
        if abs(1.0 - std) > thr:
            t = t / std
    return t * factor if factor != 1 else t


def ordered_bits(t: torch.Tensor) -> torch.Tensor:
    """16-bit floats as integers in value order (-0 and +0 coincide): neighbours differ by one."""
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, 0x8000 - b, b)


def check(got: torch.Tensor, want64: torch.Tensor, rtol=1e-5, atol=1e-6):
    got = got.cpu()
    assert tuple(got.shape) == tuple(want64.shape)
    if got.dtype == torch.float32:
        torch.testing.assert_close(got.double(), want64, rtol=rtol, atol=atol, equal_nan=True)
    else:
        want = want64.to(got.dtype)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        ok = ~torch.isnan(want)
        worst = int((ordered_bits(got)[ok] - ordered_bits(want)[ok]).abs().max()) if bool(ok.any()) else 0
        assert worst <= 1, f"{worst} ulp of {got.dtype}"


def seeded(planes, plane_in, seed, shift=0.8, scale=1.7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(planes, plane_in, generator=g) * scale + shift


def sprinkle(src, seed):
    """A few NaN / +inf / -inf anywhere (kept part and padding alike)."""
    g = torch.Generator().manual_seed(seed)
    flat = src.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[: max(3, flat.numel() // 97)]
    flat[idx[0::3]] = float("nan")
    flat[idx[1::3]] = float("inf")
    flat[idx[2::3]] = float("-inf")
    return src


def run_tail(api, src, plane_out, *, fix, normalized, factor, out_dtype=torch.float32):
    planes, plane_in = src.shape
    return api.hl.noise_params_tail(src.cuda().contiguous(), (planes, plane_out), out_dtype, planes, plane_in, plane_out, fix_invalid=fix,
                                    normalized=normalized, factor=factor)


GEOMETRIES = [(144, 140), (81, 77), (64, 60), (4096, 4096), (4100, 4099)]


@pytest.mark.parametrize("planes", [1, 8, 37])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: f"{g[0]}to{g[1]}")
def test_tail_kernels_against_float64(api, planes, geometry):
    """An unaligned crop (144 -> 140: vectors, a guarded last tile), an odd crop (81 -> 77: one value per lane), a plane shorter than a
    tile (64 -> 60), whole tiles on the vector route (4096), and the one-value route with a tail tile (4100 -> 4099)."""
    plane_in, plane_out = geometry
    src = sprinkle(seeded(planes, plane_in, 1000 + planes * 7 + plane_in), 5 + planes)
    margins = []
    want = ref_tail(src, plane_out, True, True, 0.6, margins)
    assert min(margins[0]) >= 0.2, f"the test's own input sits near a threshold: {margins}"
    check(run_tail(api, src, plane_out, fix=True, normalized=True, factor=0.6), want)


@pytest.mark.parametrize("fix,normalized,factor", [(False, True, 1.0), (True, False, 1.0), (False, False, -0.3), (False, False, 1.0), (True, True, 1.0)])
@pytest.mark.parametrize("geometry", [(144, 140), (81, 77), (4096, 4096)], ids=lambda g: f"{g[0]}to{g[1]}")
def test_tail_flag_combinations(api, fix, normalized, factor, geometry):
    plane_in, plane_out = geometry
    src = seeded(8, plane_in, 77 + plane_in)
    if fix:
        sprinkle(src, 3)
    check(run_tail(api, src, plane_out, fix=fix, normalized=normalized, factor=factor), ref_tail(src, plane_out, fix, normalized, factor))


def test_without_fix_non_finite_values_reach_the_statistics(api):
    """fix_invalid off: scale_noise sees the values as they are -- one NaN makes mean and std NaN, both comparisons false, nothing changes
    but the factor; one +inf makes the mean +inf and the subtraction turns everything into -inf / NaN, as torch's does."""
    for bad in (float("nan"), float("inf")):
        src = seeded(8, 144, 9)
        src[3, 20] = bad
        t = src[:, :140].double()
        mean, std = float(t.mean()), float(t.std())
        thr = 2.5 / math.sqrt(t.numel())
        if abs(mean) > thr:
            t = t - mean
        if abs(1.0 - std) > thr:
            t = t / std
        check(run_tail(api, src, 140, fix=False, normalized=True, factor=0.6), t * 0.6)


@pytest.mark.parametrize("dst", sorted(DTYPES))
@pytest.mark.parametrize("srct", sorted(DTYPES))
@pytest.mark.parametrize("geometry", [(144, 140), (81, 77)], ids=lambda g: f"{g[0]}to{g[1]}")
def test_tail_every_dtype_pair(api, srct, dst, geometry):
    plane_in, plane_out = geometry
    src = sprinkle(seeded(37, plane_in, 4242), 8).to(DTYPES[srct])  # the reference starts from the rounded source values
    want = ref_tail(src, plane_out, True, True, 0.6)
    check(run_tail(api, src, plane_out, fix=True, normalized=True, factor=0.6, out_dtype=DTYPES[dst]), want)


@pytest.mark.parametrize("pattern", ["nan", "inf_positive_part", "inf_negative_part", "padding_only", "padding_extremes", "all_nan"])
@pytest.mark.parametrize("normalized", [True, False])
def test_tail_planted_patterns(api, pattern, normalized):
    """The planted planes of the golden file's group d, as 16 planes of 144 of which 140 are kept.  All-NaN with normalisation is 0 / 0."""
    src = cases.planted(torch, pattern, (2, 4, 12, 12)).reshape(16, 144)
    want = ref_tail(src, 140, True, normalized, 0.6)
    if pattern == "inf_positive_part":
        assert float(want.min()) == 0.0 or normalized  # -inf became 0, not the smallest finite value
    check(run_tail(api, src, 140, fix=True, normalized=normalized, factor=0.6), want)


def test_tail_cancellation_mean_300(api):
    """2^20 + 3 values with mean 300 and std 1: sum of squares 9.4e10 against a centred sum of 1e6.  The kernel meets the standard bound
    here too: its statistics are float64 and it subtracts the mean as two floats (measured: 2.8e-7 from the float64 result).  torch's own
    float32 scale_noise on the CPU, whose subtracted mean is one float32 near 300 (ulp 3.1e-5), is printed for comparison (8.97e-6)."""
    n = (1 << 20) + 3
    g = torch.Generator().manual_seed(300)
    src = (torch.randn(n, generator=g) + 300.0).reshape(1, n)
    margins = []
    want = ref_tail(src, n, True, True, 0.6, margins)
    assert min(margins[0]) >= 0.2, margins
    t = src.clone()  # py/utils.py:100-106 in float32 on the CPU
    mean, std = t.mean().item(), t.std().item()
    thr = 2.5 / math.sqrt(n)
    if abs(mean) > thr:
        t -= mean
    if abs(1.0 - std) > thr:
        t /= std
    t.mul_(0.6)
    got = run_tail(api, src, n, fix=True, normalized=True, factor=0.6)
    err = float((got.cpu().double() - want).abs().max())
    print(f"cancellation case: torch float32 on the CPU is {float((t.double() - want).abs().max()):.3e} from float64, the kernel {err:.3e}")
    check(got, want)
    assert float(got.std()) == pytest.approx(0.6 * float(src.double().std()), rel=1e-6)  # std was judged to be 1: no division


def test_tail_refuses_bad_arguments(api):
    hl = api.hl
    src = torch.zeros(4, 16, device="cuda")
    with pytest.raises(hl.SonarHipError):
        hl.noise_params_tail(src, (4, 17), torch.float32, 4, 16, 17, fix_invalid=True, normalized=True, factor=1.0)  # keeps more than there is
    with pytest.raises(hl.SonarHipError):
        hl.noise_params_tail(src, (4, 16), torch.float64, 4, 16, 16, fix_invalid=True, normalized=True, factor=1.0)
    with pytest.raises(hl.SonarHipError):
        hl.noise_params_tail(src, (3, 16), torch.float32, 3, 16, 16, fix_invalid=False, normalized=False, factor=1.0)  # planes do not cover src


# ------------------------------------------------------------------------------------------------ item and node against the reference
def _golden():
    from tests.conftest import GOLDEN

    g = np.load(f"{GOLDEN}/noise_params.npz", allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def planted_item(nz, planes):
    class PlantedNoise(nz.CustomNoiseItemBase):
        """Hands back the stored planes, one per call, in the dtype and on the device of the latent it was built for."""

        def make_noise_sampler(self, x, *args, **kwargs):
            stored, state = self.planes, {"i": 0}

            def noise_sampler(_s, _sn):
                out = stored[state["i"] % stored.shape[0]].to(device=x.device, dtype=x.dtype, copy=True)
                state["i"] += 1
                assert out.shape == x.shape, (out.shape, x.shape)
                return out

            return noise_sampler

    return PlantedNoise(1.0, planes=planes)


def build_item(api, m, planes=None, **override):
    nz = api.nz
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian") if m["base"] == "gaussian" else planted_item(nz, planes))
    kw = dict(m["kw"]) | override
    return nz.CustomNoiseParametersNoise(kw.pop("factor", m["factor"]), noise=chain, **kw).clone()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_item_against_the_reference(api, name):
    """Every case of the golden file through make_noise_sampler on the device in replay mode; group g also compares the caller's next
    host draws after each call bit for bit.  The two normalised bfloat16-latent cases compare within one bfloat16 ulp of the reference's
    scale_noise run in float64 on the same bfloat16 values (the case table says why).  b_square_3d_77: the reference's own item fails there (its crop flattens one dimension of
    the squared plane; recorded as reference_error) and the expectation is put together from the reference's parts in the item's order."""
    g, meta = _golden()
    m = meta[name]
    assert m["kw"] == cases.CASES[name]["kw"] and m["seed"] == cases.CASES[name]["seed"], "the golden file is older than the case table"
    planes = torch.from_numpy(g[f"planes_{name}"]) if f"planes_{name}" in g else None
    item = build_item(api, m, planes)
    x = torch.zeros(m["shape"], dtype=DTYPES[m["dtype"]], device="cuda")
    torch.manual_seed(m["seed"])
    ns = item.make_noise_sampler(x, 0.03, 14.6, seed=m["seed"], cpu=True, normalized=True)
    want = torch.from_numpy(g[f"out_{name}"])
    for i, (s, sn) in enumerate(cases.SIGMAS):
        got = ns(torch.tensor(s), torch.tensor(sn))
        after = torch.randn(4)
        assert got.is_cuda and got.dtype == x.dtype and tuple(got.shape) == tuple(m["shape"])
        w = want[i]
        if m.get("compare") == "float64_rounded":  # the reference's scale_noise run in float64, rounded to the latent's dtype: one ulp
            worst = int((ordered_bits(got.cpu()) - ordered_bits(w.to(x.dtype))).abs().max())
            assert worst <= 1, f"{worst} ulp of {x.dtype}"
            continue
        torch.testing.assert_close(got.float().cpu(), w, rtol=4e-5, atol=4e-5 * max(1.0, float(w.abs().max())))
        if name.startswith("g_"):
            assert torch.equal(after, torch.from_numpy(g[f"after_{name}"])[i]), "the caller's host generator was left somewhere else"


def test_node_with_reference_sockets(api):
    """The node's own route to the item (dtype names, the tristate, device names: "cpu" = replay mode) on the case that sets most of them."""
    g, meta = _golden()
    m = meta["f_bf16_on_f32"]
    node = api.reg.NODE_CLASS_MAPPINGS["SonarCustomNoiseParameters"]()
    inner = api.nz.CustomNoiseChain()
    inner.add(planted_item(api.nz, torch.from_numpy(g["planes_f_bf16_on_f32"])))
    kw = dict(m["kw"]) | {"override_dtype": "bfloat16", "override_device": "cpu", "normalize": "default"}
    item = node.go(factor=m["factor"], custom_noise=inner, **kw)[0].items[0]
    x = torch.zeros(m["shape"], device="cuda")
    ns = item.make_noise_sampler(x, 0.03, 14.6, seed=m["seed"], cpu=False, normalized=True)
    want = torch.from_numpy(g["out_f_bf16_on_f32"])
    for i, (s, sn) in enumerate(cases.SIGMAS):
        got = ns(torch.tensor(s), torch.tensor(sn))
        torch.testing.assert_close(got.cpu(), want[i], rtol=4e-5, atol=4e-5 * max(1.0, float(want[i].abs().max())))
    gpu = node.go(factor=1.0, custom_noise=inner, **(dict(m["kw"]) | {"override_dtype": "default", "override_device": "gpu", "normalize": "disabled"}))[0]
    assert torch.device(gpu.items[0].override_device).type == "cuda" and gpu.items[0].normalize is False


# ------------------------------------------------------------------------------------------------ generate mode: the RNG contract
def _gen_item(api, **kw):
    m = {"base": "gaussian", "factor": 1.0, "kw": cases.DEFAULTS | kw}
    return build_item(api, m)


def _device_position():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset()


@pytest.mark.parametrize("rng_mode", ["fork", "separate"])
@pytest.mark.parametrize("cpu", [False, True])
def test_fork_and_separate_leave_the_device_generator_where_it_was(api, rng_mode, cpu):
    x = torch.zeros(2, 4, 10, 14, device="cuda")
    torch.manual_seed(5)
    torch.randn(8, device="cuda")  # the generator is somewhere past its start
    ns = _gen_item(api, rng_mode=rng_mode, rng_offset_mode="override", rng_state_offset=31).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=cpu,
                                                                                                                normalized=True)
    before = _device_position()
    host = torch.get_rng_state()
    out = ns(*SIG)
    assert _device_position() == before and torch.equal(torch.get_rng_state(), host)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())
    plain = _gen_item(api).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=cpu, normalized=True)
    plain(*SIG)  # "default" does move the generator it draws from
    assert (not torch.equal(torch.get_rng_state(), host)) if cpu else (_device_position() != before)


def test_separate_is_a_function_of_its_seed(api):
    x = torch.zeros(2, 4, 10, 14, device="cuda")

    def two(seed_kw, prepare, **kw):
        prepare()
        ns = _gen_item(api, rng_mode="separate", **kw).make_noise_sampler(x, 0.03, 14.6, cpu=False, normalized=True, **seed_kw)
        torch.randn(3, device="cuda")  # the caller draws in between: not the item's business
        first = ns(*SIG).clone()
        torch.randn(5, device="cuda")
        return first, ns(*SIG).clone()

    def state_a():
        torch.manual_seed(1)

    def state_b():
        torch.manual_seed(2)
        torch.randn(1000, device="cuda")

    a = two({"seed": 9}, state_a, rng_offset_mode="override", rng_state_offset=1234)
    b = two({"seed": 10}, state_b, rng_offset_mode="override", rng_state_offset=1234)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], a[1])
    c = two({"seed": 9}, state_a, rng_offset_mode="override", rng_state_offset=1235)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # "add" with offset k is "override" with seed + k
    d = two({"seed": 1200}, state_b, rng_offset_mode="add", rng_state_offset=34)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])


# ------------------------------------------------------------------------------------------------ prepared plans, launch count
def _param_chain(api, **kw):
    chain = api.nz.CustomNoiseChain()
    chain.add(_gen_item(api, **kw))
    return chain


def _fake_model(x, sigma, **_kw):
    s = sigma.reshape(-1, *([1] * (x.ndim - 1)))
    return x * 0.5 + torch.tanh(x) * (0.1 * s / (1.0 + s))


def test_a_sampler_step_with_this_item_is_traced_and_replays_the_same_bits(api):
    """Sonar Euler ancestral steps over a chain holding the item (fix_invalid and the square option: both tail launches): with plans the
    chain's step is traced and replayed, and every step's x equals the ordinary path's bit for bit."""
    hl = api.hl
    x0 = (torch.randn(2, 4, 10, 14, generator=torch.Generator().manual_seed(3)) * 14.6).cuda()
    sigmas = torch.cat((torch.linspace(14.6, 0.03, 10), torch.zeros(1)))

    def run(plans):
        old, hl.PLANS_ENABLED = hl.PLANS_ENABLED, plans
        try:
            torch.manual_seed(77)
            ns = _param_chain(api, fix_invalid=True, ensure_square_aspect_ratio=True).make_noise_sampler(x0, 0.03, 14.6, seed=77, cpu=False, normalized=True)
            trace = []
            api.sonar.SonarEulerAncestral.sampler(_fake_model, x0.clone(), sigmas, {"seed": 77}, lambda d: trace.append(d["x"].clone()), True, None, {},
                                                  0.8, 1.1, ns)
            return ns, trace
        finally:
            hl.PLANS_ENABLED = old

    (a, ta), (b, tb) = run(True), run(False)
    assert len(ta) == len(tb) >= 10 and all(torch.equal(p, q) for p, q in zip(ta, tb))
    planned = [p for p in (a, getattr(a, "deferred", None)) if isinstance(p, hl.Planned)]
    assert planned, "the chain holding the item was not offered to the planner"
    assert any(p.plan is not None and p.plan.runs >= 1 for p in planned), [p.reason for p in planned]


def test_separate_rng_declines_the_trace_and_takes_the_ordinary_path(api):
    """rng_mode "separate" / "fork" move generator state around the draw on the host: such a sampler is not offered to the planner."""
    x = torch.zeros(2, 4, 10, 14, device="cuda")
    ns = _param_chain(api, rng_mode="fork").make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=False, normalized=True)
    assert not isinstance(ns, api.hl.Planned) and not getattr(ns, "plan_static", False)
    torch.manual_seed(4)
    outs = [ns(*SIG).clone() for _ in range(5)]
    assert all(torch.equal(outs[0], o) for o in outs[1:])  # a fork draws from the same position every time


def _traced_length(api, fn):
    """Records of the plan ``hip_lib.trace_plan`` makes of one call of ``fn``: its recorder notes every entry point the call issues and
    refuses the trace when a torch kernel touches a device tensor in between."""
    hl, rng = api.hl, api.nz.DeviceRNG
    out, plan = hl.trace_plan(fn, SIG, take=rng.take, rewind=rng.rewind, guards=())
    assert plan is not None, hl.trace_plan.last_reason
    return out, hl.load().sonar_plan_length(plan.handle)


def test_the_tail_is_at_most_two_launches_and_no_torch_kernel(api, monkeypatch):
    """One call of the item's sampler traced by ``hip_lib.trace_plan``: the trace is accepted (nothing but this library's entry points
    touches a device tensor), and it holds the inner chain's own records plus two for fix + crop + normalisation, plus one for a crop
    alone, plus none of the new ones when there is nothing to fix, crop or convert."""
    x = torch.zeros(2, 4, 10, 14, device="cuda")
    inner = api.nz.CustomNoiseChain()
    inner.add(api.nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    bare = inner.make_noise_sampler(torch.zeros(2, 4, 12, 12, device="cuda"), 0.03, 14.6, seed=1, cpu=False, normalized=False)
    bare(*SIG)
    _out, base = _traced_length(api, bare)
    calls = []
    real = api.hl.noise_params_tail
    monkeypatch.setattr(api.hl, "noise_params_tail", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    for kw, extra in ((dict(fix_invalid=True, ensure_square_aspect_ratio=True), 2), (dict(ensure_square_aspect_ratio=True, normalize=False), 1)):
        ns = _gen_item(api, **kw).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=False, normalized=True)
        ns(*SIG)
        del calls[:]
        out, length = _traced_length(api, ns)
        assert length == base + extra and len(calls) == 1 and out.shape == x.shape
    # nothing to fix, crop or convert: the existing scale_noise, none of the new entry points
    ns = _gen_item(api).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=False, normalized=True)
    ns(*SIG)
    del calls[:]
    _traced_length(api, ns)
    assert not calls


def test_empty_latent_comes_back_in_its_own_shape(api):
    x = torch.zeros(0, 4, 10, 14, device="cuda")
    item = _gen_item(api, fix_invalid=True, override_device="cpu")
    ns = item.make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True, normalized=True)
    assert ns(*SIG).shape == x.shape
    # frames folded, plane squared, another generation dtype: still the latent's shape and dtype
    x = torch.zeros(0, 4, 3, 6, 10, device="cuda")
    item = _gen_item(api, fix_invalid=True, frames_to_channels=True, ensure_square_aspect_ratio=True, override_dtype="float16")
    out = item.make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True, normalized=True)(*SIG)
    assert out.shape == x.shape and out.dtype == x.dtype
