"""-m gpu: FreeUExtremeConfig.apply on the device (csrc/freeu.hip) against the fp64 statement (tests/freeu_refs.py) and the reference's
recorded outputs (tests/golden/freeu_extreme.npz).

Tolerances (derived as the pattern-break change's): E = the largest distance between the reference's fp32 output and the statement over
the golden cases, as a fraction of the output's range (1.7e-7 here).  The fp32 kernel is held to 8 E at every element, against the statement
and against the reference alike; half dtypes to the statement of the upcast input within 8 E of the range plus one rounding of the output
dtype (2^-11 / 2^-8 of the value), and to being no farther from the statement than the reference's own half outputs.  Measured distances:
profiles/freeu_extreme_refs.txt."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import freeu_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def fx(pkg):
    pkg.hip_lib.load()
    return importlib.import_module("comfyui_sonar_amd.py.nodes.freeu_extreme")


@pytest.fixture(scope="module")
def PF(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.powernoise").PowerFilter


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "freeu_extreme.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def E(g):
    return R.reference_error(g)


def config(fx, PF, kw, fname):
    return fx.FreeUExtremeConfig(target="both", stage_1=True, sonar_power_filter_opt=None if fname is None else PF(**R.FILTERS[fname]), **kw)


def check(got, x_in, filt, kw, dname, E, ref_out=None, what=""):
    """got: the device result (any dtype) as float64; x_in: the input as the kernel saw it (upcast)."""
    st = R.apply_ref(x_in, filt, **kw)
    got = got.float().cpu().numpy().astype(np.float64)
    err = np.abs(got - st)
    bound = 8 * E * R.spread(st) + (R.HALF_EPS[dname] * np.abs(st) if dname != "float32" else 0.0)
    print(f"{what} {dname}: max |got - statement| / range = {err.max() / R.spread(st):.3e}" +
          ("" if ref_out is None else f", reference: {R.distance(ref_out, st):.3e}"))
    assert (err <= bound).all(), (what, dname, float((err - bound).max()))
    if ref_out is not None:
        if dname == "float32":
            assert (np.abs(got - np.asarray(ref_out, dtype=np.float64)) <= 8 * E * R.spread(st)).all(), (what, "vs reference")
        else:
            assert err.max() <= np.abs(np.asarray(ref_out, dtype=np.float64) - st).max(), (what, dname, "farther than the reference")
    return st


@pytest.mark.parametrize("dname", R.DTYPES)
@pytest.mark.parametrize("tag", list(R.CASES))
def test_cases(fx, PF, g, E, tag, dname):
    shape, kw, fname = R.CASES[tag]
    x = torch.from_numpy(g[f"{tag}_x"]).to(DT[dname]).cuda()
    x0 = x.clone()
    cache = {}
    out = config(fx, PF, kw, fname).apply(0, x, cache, cpu_fft=True)
    assert out is x
    filt = g.get(f"{tag}_filter") if fname else None
    if fname:
        assert set(cache) == {(0, torch.Size(shape[-2:]))}
        assert torch.allclose(cache[(0, torch.Size(shape[-2:]))].reshape(-1).cpu(), torch.from_numpy(filt).reshape(-1), rtol=1e-5, atol=1e-6)
    check(x, x0.float().cpu().numpy(), filt, kw, dname, E, g[f"{tag}_out_{dname}"], tag)
    sl = R.slice_of(shape[1], kw.get("slice", 1.0), kw.get("slice_offset", 0.0))
    keep = [c for c in range(shape[1]) if c not in range(shape[1])[sl]]
    assert torch.equal(x[:, keep], x0[:, keep])  # channels outside the slice: bit-identical


@pytest.mark.parametrize("dname", R.DTYPES)
@pytest.mark.parametrize("tag", ["a", "b", "d", "g"])
def test_layouts(fx, PF, g, E, tag, dname):
    """Channels-last (dense copy and back) and a view with a storage offset inside a larger tensor: same values, same object, and the
    storage around the view untouched."""
    shape, kw, fname = R.CASES[tag]
    x = torch.from_numpy(g[f"{tag}_x"]).to(DT[dname]).cuda()
    filt = g.get(f"{tag}_filter") if fname else None
    cl = x.clone().contiguous(memory_format=torch.channels_last)
    ptr = cl.data_ptr()
    assert config(fx, PF, kw, fname).apply(0, cl, {}) is cl and cl.data_ptr() == ptr and cl.is_contiguous(memory_format=torch.channels_last)
    check(cl, x.float().cpu().numpy(), filt, kw, dname, E, g[f"{tag}_out_{dname}"], tag + " channels-last")
    big = torch.full((shape[0] + 1, shape[1] + 3, shape[2], shape[3]), 7.0, dtype=DT[dname], device="cuda")
    view = big[1:, 1:1 + shape[1]]
    view.copy_(x)
    assert config(fx, PF, kw, fname).apply(0, view, {}) is view
    check(view, x.float().cpu().numpy(), filt, kw, dname, E, g[f"{tag}_out_{dname}"], tag + " view")
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:, 1:1 + shape[1]] = False
    assert (big[mask] == 7.0).all()
    odd = torch.zeros(x.numel() + 1, dtype=DT[dname], device="cuda")  # a plane start that is aligned to one element only
    v1 = odd[1:].view(shape)
    v1.copy_(x)
    config(fx, PF, kw, fname).apply(0, v1, {})
    check(v1, x.float().cpu().numpy(), filt, kw, dname, E, g[f"{tag}_out_{dname}"], tag + " odd offset")


def test_cache_hit_and_stack(fx, PF, g, E):
    shape, kw, f_cfg, _f_cached = R.CACHE_HIT
    x = torch.from_numpy(g["hit_x"]).cuda()
    held = torch.from_numpy(g["hit_filter"]).cuda()
    cache = {(7, torch.Size(shape[-2:])): held}
    config(fx, PF, kw, f_cfg).apply(7, x, cache)
    assert cache[(7, torch.Size(shape[-2:]))] is held
    check(x, g["hit_x"], g["hit_filter"], kw, "float32", E, g["hit_out"], "cache hit")
    with pytest.raises(UnboundLocalError):
        config(fx, PF, kw, f_cfg).apply(None, x, cache)
    shape, (kw1, f1), (kw2, f2) = R.STACK
    y = torch.from_numpy(g["stack_x"]).cuda()
    cache = {}
    for idx, (kw_, fname) in enumerate(((kw1, f1), (kw2, f2))):
        assert config(fx, PF, kw_, fname).apply(idx, y, cache) is y
    # the statement of the second application starts from the statement of the first: the bound is the single application's, per element,
    # against the statement and against the reference's recorded output alike
    st = R.apply_ref(R.apply_ref(g["stack_x"], g["stack_filter"], **kw1), None, **kw2)
    got = y.cpu().numpy().astype(np.float64)
    print(f"stack: {np.abs(got - st).max() / R.spread(st):.3e}, reference {R.distance(g['stack_out'], st):.3e}")
    assert (np.abs(got - st) <= 8 * E * R.spread(st)).all()
    assert (np.abs(got - g["stack_out"].astype(np.float64)) <= 8 * E * R.spread(st)).all()


# shapes at which the fused kernel's loops take more than one trip (the golden shapes never do): 128-long lines (eight item trips, the
# direct-sum second factor), more planes than resident workgroups (the plane loop and its barrier; the hidden mean's channel groups), and
# a plane above half the LDS (the 1024-thread instantiation).  No recorded reference at these sizes: the fp64 statement alone, same bound.
BIG = {
    "lines128": ((1, 8, 128, 128), dict(scale=1.3, hidden_mean=True, blend=0.7, blend_mode="lerp", filter_norm=1.0), "A"),
    "planes640": ((2, 320, 16, 16), dict(scale=1.2, hidden_mean=True, filter_norm=1.0), "A"),
    "threads1024": ((1, 4, 192, 192), dict(scale=0.8, hidden_mean=True, slice=0.5, blend=0.7, blend_mode="inject", filter_norm=1.0), "B"),
}


@pytest.mark.parametrize("dname", ["float32", "float16"])
@pytest.mark.parametrize("tag", list(BIG))
def test_more_than_one_trip(fx, PF, pkg, E, tag, dname, monkeypatch):
    shape, kw, fname = BIG[tag]
    assert pkg.hip_lib.power_plane_kind(*shape[-2:]) in (1, 2)
    x0 = torch.from_numpy(R.make_input(shape, 500)).to(DT[dname]).cuda()
    ref_in = x0.float().cpu().numpy()
    for route in ("fused", "as routed"):  # 128 x 128 is routed to the pre-filtered path (PREFILTERED_PLANES): the fused kernel is run all the same
        if route == "fused":
            monkeypatch.setattr(fx, "PREFILTERED_PLANES", frozenset())
        else:
            monkeypatch.undo()
            if tuple(shape[-2:]) not in fx.PREFILTERED_PLANES:
                continue
        x, cache = x0.clone(), {}
        assert config(fx, PF, kw, fname).apply(3, x, cache) is x
        (filt,) = cache.values()
        check(x, ref_in, filt.cpu().numpy(), kw, dname, E, None, f"{tag} {route}")


def test_zero_input_gives_the_reference_nans(fx, PF, g):
    z = torch.zeros(1, 4, 8, 8, device="cuda")
    out = config(fx, PF, dict(scale=1.3, hidden_mean=True), None).apply(0, z, {})
    assert np.array_equal(np.isnan(out.cpu().numpy()), np.isnan(g["zero_out"]))
    half = torch.zeros(1, 4, 8, 8, device="cuda", dtype=torch.bfloat16)
    assert config(fx, PF, dict(scale=1.3, hidden_mean=True, slice=0.5), None).apply(0, half, {})[:, :2].isnan().all() and (half[:, 2:] == 0).all()


def test_get_scale_and_refusals(fx, PF, g, pkg):
    x = torch.from_numpy(g["a_x"]).cuda()
    s = config(fx, PF, dict(scale=1.3), None).get_scale(x).cpu().numpy().astype(np.float64)
    m = g["a_x"].astype(np.float64).mean(1, keepdims=True)
    lo, hi = m.min((2, 3), keepdims=True), m.max((2, 3), keepdims=True)
    assert np.abs(s - (1 + 0.3 * (m - lo) / (hi - lo))).max() < 1e-6
    nan = x.clone()
    nan[1, 3, 2, 2] = float("nan")
    _mean, ext = pkg.hip_lib.freeu_hidden_mean(nan)
    assert ext[1].isnan().all() and ext[0].isfinite().all()
    with pytest.raises(NotImplementedError):
        config(fx, PF, {}, None).apply(0, x.double(), {})
    with pytest.raises(pkg.hip_lib.SonarHipError):
        config(fx, PF, {}, "A").apply(0, torch.zeros(1, 1, 2, 4096, device="cuda"), {})
    with pytest.raises(KeyError):
        config(fx, PF, dict(blend=0.5, blend_mode="nope"), None).apply(0, x, {})


def test_block_patches_end_to_end(fx, PF, g, E):
    """Stage 2 (2 m channels) through in_patch with a stub timestep; an unmapped channel count comes back untouched."""
    _shape, kw, fname = R.CASES["a"]
    cfg = fx.FreeUExtremeConfig(target="both", stage_2=True, start=0.2, end=0.6, sonar_power_filter_opt=PF(**R.FILTERS[fname]), **kw)
    inp, mid, outp = fx.make_block_patches(model_channels=4, timestep=lambda s: s * 999.0, input_config=cfg, output_config=cfg)
    assert mid is None
    x = torch.from_numpy(g["a_x"]).cuda()
    top = {"sigmas": torch.tensor([0.3, 0.6], device="cuda")}  # pct = 0.4
    assert inp(x, top) is x
    check(x, g["a_x"], g["a_filter"], kw, "float32", E, g["a_out_float32"], "in_patch")
    late = torch.from_numpy(g["a_x"]).cuda()
    assert torch.equal(inp(late, {"sigmas": torch.tensor([0.9], device="cuda")}), torch.from_numpy(g["a_x"]).cuda())  # pct = 0.1 < start
    other = torch.ones(1, 6, 8, 8, device="cuda")
    assert torch.equal(inp(other, top), torch.ones(1, 6, 8, 8, device="cuda"))
    h, hsp = torch.from_numpy(g["a_x"]).cuda(), torch.from_numpy(g["a_x"]).cuda()[:, :5].contiguous()
    a, b = outp(h, hsp, top)
    assert a is h and b is hsp
    check(h, g["a_x"], g["a_filter"], kw, "float32", E, g["a_out_float32"], "out_patch h")
    check(hsp, g["a_x"][:, :5], g["a_filter"], kw, "float32", E, None, "out_patch hsp")  # 5 channels: the stage came from h
