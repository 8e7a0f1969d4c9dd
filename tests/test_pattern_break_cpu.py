"""CPU: utils.pattern_break / PatternBreakNoise -- the host statements of the filter (tests/pattern_break_refs.py) against the reference's
stored outputs and against torch, the exact-remainder form the kernel uses, the entry points of csrc/pattern_break.hip declared, bound and
exported, their refusals without a device, the Python refusals, the unchanged registry and the percentage == 0 pass-through.

The tolerance is measured, not chosen: E = the largest |fp32 statement - fp64 statement| over the golden cases, each divided by its case's
output range (pattern_break_refs.out_range), and the bound of a case is MARGIN x E x its range.  profiles/pattern_break_refs.txt holds the
figures (E = 1.05e-7; the reference's own outputs lie within 1.6e-7 of the fp64 statement).  No element is excluded anywhere."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import pattern_break_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
cases = R.cases

ENTRY_POINTS = ("sonar_pattern_break_route", "sonar_pattern_break_f32")
FUNCTION_CASES = cases.function_cases()


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


load_goldens, statements = R.load_goldens, R.statements


def test_the_case_table_covers_the_issue_and_matches_the_files():
    g = load_goldens()
    assert 36 <= len(FUNCTION_CASES) <= 48 and len({c[0] for c in FUNCTION_CASES}) == len(FUNCTION_CASES)
    for col, values in ((2, cases.PERCENTAGES), (3, cases.DETAIL_LEVELS), (4, (True, False)), (5, cases.MODES)):
        assert {c[col] for c in FUNCTION_CASES} == set(values)
    assert {c[1] for c in FUNCTION_CASES} == set(cases.INPUTS)
    for name, (shape, _kind) in cases.INPUTS.items():
        assert g[f"in_{name}"].shape == shape and g[f"in_{name}"].dtype == np.float32
    for name, inp, *_ in FUNCTION_CASES:
        assert g[f"out_{name}"].shape == cases.INPUTS[inp][0]
    ext = g["in_extremes"].ravel()
    assert (ext == ext.min()).sum() >= 3 and (ext == ext.max()).sum() >= 3 and np.signbit(ext[18]) and ext[17] == 0 and not np.signbit(ext[17])
    assert np.ptp(g["in_const"]) == 0 and g["in_single"].size == 1 and g["in_g5d"].ndim == 5
    assert abs(float(np.abs(g["in_scaled"]).max())) > 50
    for name in cases.ITEMS:
        assert g[f"item_{name}"].shape == (len(cases.ITEM_SIGMAS), *cases.ITEM_LATENT)


def test_the_goldens_lie_within_the_bound_of_both_statements():
    st = statements()
    E = st["E"]
    assert 2e-8 < E < 1e-6, E  # a chain of a few fp32 roundings on values of the order of the range
    lines = []
    for name, (want, s32, s64, scale) in st["table"].items():
        bound = R.MARGIN * E * scale
        d64, d32 = float(np.abs(want - s64).max()), float(np.abs(want.astype(np.float64) - s32).max())
        lines.append(f"{name}: range {scale:.4g}  fp32 statement {float(np.abs(s32 - s64).max()) / scale:.3e}  reference {d64 / scale:.3e}  "
                     f"bound {R.MARGIN * E:.3e} (x range)")
        assert np.isfinite(want).all() and d64 <= bound and d32 <= bound, (name, d64, d32, bound)
    print(f"E = {E:.4e}\n" + "\n".join(lines))


@pytest.mark.parametrize("shape", [(1, 4, 8, 8), (2, 4, 33, 17), (4, 16, 128, 128)])
def test_the_front_half_equals_torch_bit_for_bit(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    lo, hi = x.min(), x.max()  # py/utils.py:587-590 up to erfinv's argument, in torch fp32 on the CPU
    v = (((x - lo) / ((hi - lo) + 1e-7)) * 2 + (-1)).clamp(-1, 1)
    a = 2 * (torch.remainder(torch.abs(v) * 1000000, 11) / 11) - 1
    mine, mlo, mhi = R.front(x.numpy())
    assert mine.dtype == np.float32 and np.array_equal(mine, a.numpy()) and mlo == lo.item() and mhi == hi.item()
    # r == 0 becomes exactly -1 and happens: the infinity of erfinv(-1) is part of the filter
    if x.numel() > 4000:
        assert (mine == -1).any()


def test_one_ulp_in_the_input_moves_outputs_by_more_than_the_bound():
    """Why the front half is stated bit-exactly: the map is chaotic."""
    x = statements()["g"]["in_g4488"]
    y = x.copy()
    y.ravel()[np.argmin(x)] = np.nextafter(x.min(), np.float32(-np.inf))
    a, b = (R.pattern_break(t, percentage=1.0, restore_scale=False) for t in (x, y))
    assert float(np.abs(a - b).max()) > 0.1


def test_the_exact_remainder_form_equals_fmod_in_every_binade():
    rng = np.random.default_rng(5)
    parts = [np.array([0.0, 10.999999, 11.0, 11.000001, 21.999998, 22.0, 1e6, 999999.94, 1.0, 11 * 90909.0], dtype=np.float32)]
    for e in range(-30, 20):  # every binade up to 2^20 > 1e6, random mantissas, and the multiples of 11 with their neighbours
        parts.append(np.ldexp(1 + rng.random(2000), e).astype(np.float32))
    k = (np.arange(0, 90910, 7, dtype=np.float64) * 11).astype(np.float32)
    parts += [k, np.nextafter(k, np.float32(np.inf)), np.nextafter(k, np.float32(-1))]
    m = np.concatenate(parts)
    m = m[(m >= 0) & (m <= 1e6)]
    assert m.size > 90000 and len(set(np.frexp(m[m > 0])[1])) >= 45
    want = np.fmod(m.astype(np.float64), 11.0)
    got = R.remainder11_exact_form(m)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(np.fmod(m, np.float32(11)), got)


def test_the_newton_erfinv_inverts_erf():
    """The fp64 statement's erfinv where scipy is not installed: erf(erfinv(a)) == a to fp64 rounding, and the one in use agrees."""
    import math

    a = np.concatenate((np.linspace(-0.999999, 0.999999, 2001), [0.0, 1e-12, -1e-300, 1 - 2.0**-24, -1 + 2.0**-24]))
    z = R.newton_erfinv(a)
    back = np.array([math.erf(v) for v in z])
    assert np.abs(back - a).max() < 4e-16 and np.array_equal(np.sign(z), np.sign(a))
    # a few fp64 roundings of erf's value, through erfinv's slope sqrt(pi) / 2 exp(z^2)
    assert (np.abs(R._erfinv(a) - z) <= 4e-16 * math.sqrt(math.pi) / 2 * np.exp(z * z) + 1e-15).all()
    for fn in (R.newton_erfinv, R._erfinv):
        assert fn(np.array([-1.0]))[0] == -np.inf and fn(np.array([1.0]))[0] == np.inf
        assert fn(np.array([-1, 0.5], dtype=np.float32)).dtype == np.float32


def test_entry_points_are_declared_bound_and_exported(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64}
    lib = hl.load()
    for name in ENTRY_POINTS:
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert restype is hl.C.c_int and len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), (name, p)
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    define = lambda n: int(re.search(rf"#define {n} (\d+)", text).group(1))  # noqa: E731
    assert define("SONAR_PATTERN_BREAK_NPART") * 4 == hl.PATTERN_BREAK_WS and define("SONAR_PATTERN_BREAK_NPART") <= hl.NPART
    assert hl.PATTERN_BREAK_ROUTES == {None: define("SONAR_PATTERN_BREAK_AUTO"), "one": define("SONAR_PATTERN_BREAK_ONE"),
                                       "three": define("SONAR_PATTERN_BREAK_THREE")}
    limit = define("SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX")
    assert lib.sonar_pattern_break_route(1) == 1 and lib.sonar_pattern_break_route(limit) == 1 and lib.sonar_pattern_break_route(limit + 1) == 2
    assert os.path.exists(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "pattern_break.hip"))
    assert os.path.exists(os.path.join(ROOT, "tools", "pattern_break_validate.cpp"))


def test_bad_arguments_come_back_as_error_codes_without_a_device(pkg):
    """The checks run before anything touches the HIP runtime: the pointers below are never dereferenced."""
    hl = pkg.hip_lib
    lib = hl.load()
    fn = lib.sonar_pattern_break_f32
    x, out, ws, st = 0x1000, 0x2000, 0x3000, 0x4000
    ok = dict(x=x, out=out, n=100, detail=1.0, p=0.5, mode=0, restore=1, route=0, ws=ws, wsn=hl.PATTERN_BREAK_WS, stats=st)

    def call(**kw):
        a = ok | kw
        return fn(a["x"], a["out"], a["n"], a["detail"], a["p"], a["mode"], a["restore"], a["route"], a["ws"], a["wsn"], a["stats"], None)

    for bad in (dict(x=None), dict(out=None), dict(ws=None), dict(x=x + 2), dict(out=out + 1), dict(ws=ws + 2), dict(stats=st + 4),
                dict(out=x), dict(ws=x), dict(ws=out), dict(n=0), dict(n=-5), dict(mode=3), dict(mode=-1), dict(route=3), dict(route=-1),
                dict(wsn=hl.PATTERN_BREAK_WS - 1), dict(wsn=0)):
        assert call(**bad) == hl.ERR_ARG, bad
    assert call(wsn=7) == hl.ERR_ARG and b"SONAR_PATTERN_BREAK_WS" in lib.sonar_last_error()
    assert call(mode=7) == hl.ERR_ARG and b"blend mode 7" in lib.sonar_last_error()


def test_python_refusals(nz, monkeypatch):
    utils = nz.utils
    params = inspect.signature(utils.pattern_break).parameters
    assert list(params) == ["noise", "percentage", "detail_level", "restore_scale", "blend_function", "route"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in params.items() if name != "noise")
    assert (params["percentage"].default, params["detail_level"].default, params["restore_scale"].default) == (0.5, 0.0, True)
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="blend_function"):  # before the device check: a foreign callable never runs
        utils.pattern_break(x, blend_function=torch.lerp)
    with pytest.raises(NotImplementedError, match="blend_function"):
        utils.pattern_break(x, blend_function=lambda a, b, t: a)
    for fn in utils.BLENDING_MODES.values():  # the three built-in ones pass that check and reach the device check
        with pytest.raises(nz.hip_lib.SonarHipError, match="only runs on a ROCm device"):
            utils.pattern_break(x, blend_function=fn)
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    monkeypatch.setattr(utils, "_require_device", lambda t, what: None)
    with ng.shard_offset(1), pytest.raises(NotImplementedError, match="reduces across the samples of the batch, which a sharded batch"):
        utils.pattern_break(x)
    with pytest.raises(RuntimeError, match="numel\\(\\) == 0"):
        utils.pattern_break(torch.zeros(0, 4))
    with pytest.raises(nz.hip_lib.SonarHipError, match="route"):
        nz.hip_lib.pattern_break(x, 1.0, 0.5, "lerp", True, route="two")
    with pytest.raises(nz.hip_lib.SonarHipError, match="blend mode"):
        nz.hip_lib.pattern_break(x, 1.0, 0.5, "slerp", True)


def test_the_registry_is_unchanged(reg):
    assert len(reg.NODE_CLASS_MAPPINGS) == 54 and len(reg.IMPLEMENTED_KEYS) == 42
    off = sorted(k for k, cls in reg.NODE_CLASS_MAPPINGS.items() if cls.__name__.startswith("OffPath_"))
    assert len(off) == 12 and not set(off) & set(reg.IMPLEMENTED_KEYS)
    assert "SonarPatternBreakNoise" in off and "SonarPatternBreakNoise" not in reg.IMPLEMENTED_KEYS


class _Inner:
    """A chain stand-in whose sampler is one known object; remembers how it was asked."""

    def __init__(self):
        self.sampler = lambda s, sn: None
        self.asked = []

    def clone(self):
        return self

    def make_noise_sampler(self, *a, **k):
        self.asked.append(k)
        return self.sampler


def test_the_item_and_its_pass_through(nz):
    assert issubclass(nz.PatternBreakNoise, nz.CustomNoiseItemBase)
    params = inspect.signature(nz.PatternBreakNoise.__init__).parameters
    assert list(params) == ["self", "factor", "noise", "detail_level", "percentage", "restore_scale", "blend_mode", "blend_function"]
    assert params["blend_mode"].default == "lerp" and params["blend_function"].default is None
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.PatternBreakNoise(0.7, noise=chain, detail_level=3.5, percentage=0.25, restore_scale=False, blend_mode="inject")
    clone = item.clone()
    assert clone.keys == {"noise", "detail_level", "percentage", "restore_scale", "blend_function"} and clone.noise is not item.noise
    assert (clone.factor, clone.detail_level, clone.percentage, clone.restore_scale) == (0.7, 3.5, 0.25, False)
    assert clone.blend_function is nz.utils.BLENDING_MODES["inject"]
    with pytest.raises(KeyError):
        nz.PatternBreakNoise(1.0, noise=chain, detail_level=0.0, percentage=0.5, restore_scale=True, blend_mode="slerp")
    # percentage == 0: the inner sampler object itself, asked with the caller's `normalized`
    for normalized in (True, False):
        inner = _Inner()
        ns = nz.PatternBreakNoise(0.7, noise=inner, detail_level=0.0, percentage=0, restore_scale=True).make_noise_sampler(
            torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=normalized)
        assert ns is inner.sampler and inner.asked[-1]["normalized"] is normalized
        assert inner.asked[-1]["sigma_min"] == 0.03 and inner.asked[-1]["sigma_max"] == 14.6
    # otherwise the inner chain is asked for un-normalised noise and the result is a new sampler
    inner = _Inner()
    ns = nz.PatternBreakNoise(0.7, noise=inner, detail_level=0.0, percentage=0.5, restore_scale=True).make_noise_sampler(
        torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)
    assert ns is not inner.sampler and inner.asked[-1]["normalized"] is False
    # a launchable call on a CPU latent: no host fallback
    with pytest.raises(nz.hip_lib.SonarHipError):
        item.make_noise_sampler(torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)(torch.tensor(10.0), torch.tensor(5.0))
