"""CPU: VoronoiNoiseGenerator / AdvancedVoronoiNoise -- the numpy statement (tests/voronoi_refs.py) against the reference's own outputs
(tests/golden/voronoi.npz), the mode parser's errors and refusals, the entry point declared, bound and exported with its argument
checks, the unchanged registry and the item class.  tests/test_gpu_voronoi.py holds the kernel to the same statement and the same file.

The bound is not a fixed tolerance: per case the fp32 statement's distance to the fp64 statement is measured over the elements that are
not ambiguous, and the reference's golden must lie within 8 x that of the fp64 statement (floor 1e-6 of the case's output range); 8 x
because the reference's operation order differs from the statement's by a few roundings.  The measured figures are in
profiles/voronoi_refs.txt."""
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import voronoi_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import voronoi_cases as cases  # noqa: E402

CASES = cases.cases()
IDS = [n for n, _l, _p in CASES]


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "voronoi.npz"), allow_pickle=False)


def golden_draws(g, name):
    flat, at = g[f"draws_{name}"], [0]

    def draw(shape):
        n = int(np.prod(shape))
        part = flat[at[0]:at[0] + n]
        at[0] += n
        assert part.size == n
        return part.reshape(shape)

    draw.used = lambda: at[0]
    return draw


def statements(g, name, latent, params, variant=None):
    """Per call: (fp64 statement, ambiguous, fp32 statement); computed once per case and variant."""
    key = (name, variant)
    if key not in statements.cache:
        g64 = R.Generator(latent, params, golden_draws(g, name), np.float64, variant)
        g32 = R.Generator(latent, params, golden_draws(g, name), np.float32, variant)
        calls = []
        for _ in range(cases.CALLS):
            want, amb = g64.generate()
            got32, _ = g32.generate()
            assert got32.dtype == np.float32
            calls.append((want, amb, got32))
        assert g64.draw.used() == g[f"draws_{name}"].size  # every recorded draw was taken, none twice
        statements.cache[key] = (calls, g64)
    return statements.cache[key]


statements.cache = {}


def cap(name):
    return 1e-2 if name in cases.WIDE else 1e-3


# ------------------------------------------------------------------------------------------------ the statement is the reference
@pytest.mark.parametrize("name, latent, params", CASES, ids=IDS)
def test_the_reference_lies_within_the_fp32_statements_error_of_the_fp64_statement(g, name, latent, params):
    calls, gen = statements(g, name, latent, params)
    for i, (want, amb, got32) in enumerate(calls):
        share = float(amb.mean())
        err32, err_ref = R.error(got32, want, amb), R.error(g[f"out_{name}"][i], want, amb)
        print(f"{name} call {i}: fp32 statement {err32:.3e}  reference {err_ref:.3e}  bound {R.bound(err32, want):.3e}  ambiguous {share:.2e}")
        assert share <= cap(name), f"call {i}: ambiguous share {share:.2e}"
        assert err_ref <= R.bound(err32, want), f"call {i}: reference {err_ref:.3e}, fp32 statement {err32:.3e}"
    assert np.array_equal(g[f"z_{name}"], np.array([gen.z_curr, gen.z_increment]))


@pytest.mark.parametrize("variant, name", [("no_wrap", "d_euclidean"), ("swap_f1_f2", "r_diff2"), ("swap_f1_f2", "d_euclidean"),
                                           ("true_l1", "d_manhatten")])
def test_negative_controls_fail_the_comparison(g, variant, name):
    _n, latent, params = next(c for c in CASES if c[0] == name)
    good, _ = statements(g, name, latent, params)
    bad, _ = statements(g, name, latent, params, variant)
    for i in range(cases.CALLS):
        want, amb, got32 = good[i]
        assert R.error(g[f"out_{name}"][i], bad[i][0], amb | bad[i][1]) > R.bound(R.error(got32, want, amb), want), (variant, i)


def test_the_golden_file_and_the_case_table_agree(g):
    meta = json.loads(str(g["meta_json"]))
    assert sorted(meta) == sorted(IDS) and len(IDS) == len(set(IDS))
    for name, latent, params in CASES:
        assert meta[name] == json.loads(json.dumps({"latent": latent, "params": params})), name
        out = g[f"out_{name}"]
        assert out.shape == (cases.CALLS, *latent) and out.dtype == np.float32 and np.isfinite(out).all() and g[f"next_{name}"].shape == (4,)
    assert g["item_out"].shape == (len(cases.ITEM["sigmas"]), *cases.ITEM["latent"]) and np.isfinite(g["item_out"]).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "voronoi.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "collatz.npz"))
    assert {p["octave_mode"] for _n, _l, p in CASES if "octave_mode" in p} == {"new_features", *cases.OCTAVE_MODES}
    assert {p["n_points"][0] for _n, _l, p in CASES} >= {1, 5, 33, cases.CHUNK_EDGE}


# ------------------------------------------------------------------------------------------------ the mode strings
def test_the_parser_flattens_what_the_reference_evaluates(nz):
    parse = nz.VoronoiNoiseGenerator.parse_modes
    d, r = parse("weight:name=fractal_norm:__name=chebyshev:_mode=sin:h=0.7+euclidean:dscale=0.5", "f1+ridge:rscale=0.25")
    assert d[0] == {"metric": "chebyshev", "xforms": (("weight", 0.7, 1.0, 0.25), ("fractal_sin", 0.1, 10.0, 0.0)), "scale": 0.5}
    assert d[1] == {"metric": "euclidean", "xforms": (), "scale": 0.25}
    assert r[0] == {"op": "f", "idx1": 0, "idx2": 0, "fns": (), "ridges": (), "scale": 0.5}
    assert r[1] == {"op": "diff", "idx1": 0, "idx2": 1, "fns": (), "ridges": (-10.0,), "scale": 0.125}
    # a `_key` beside `key` at one level collapses onto it, the later one winning, as in the reference's dict comprehension
    _, r = parse("euclidean", "ridge:name=ridge:_name=f2:exp=-3:_exp=2")
    assert r[0] == {"op": "f", "idx1": 1, "idx2": 1, "fns": (), "ridges": (2.0,), "scale": 1.0}
    _, r = parse("euclidean", "ridge:name=ridge:__name=f2:exp=-3:__exp=2")
    assert r[0]["ridges"] == (2.0, -3.0) and r[0]["op"] == "f" and r[0]["idx1"] == 1      # innermost first
    _, r = parse("euclidean", "fractal_norm:mode=cos:name=ridge:__name=diff2")
    assert r[0]["fns"] == (("fractal_cos", 0.1, 10.0),) and r[0]["ridges"] == (-10.0,) and r[0]["op"] == "diff2"
    _, r = parse("euclidean", "diff2+gradient_magnitude:name1=f2:name2=ridge:rscale=0.5+fuzz:name=diff:fuzz=0.1")
    assert r[1]["op"] == "gradient_magnitude" and r[1]["scale"] == 0.5 / 3 and [t["op"] for t in r[1]["inner"]] == ["f", "diff"]
    assert r[1]["inner"][0]["idx1"] == 1 and r[1]["inner"][1]["ridges"] == (-10.0,)
    assert r[2]["op"] == "fuzz" and r[2]["fuzz"] == 0.1 and r[2]["inner"][0]["op"] == "diff" and len(r[2]["inner"]) == 1
    _, r = parse("euclidean", "gradient_magnitude")
    assert len(r[0]["inner"]) == 1 and r[0]["inner"][0]["idx1"] == 3                       # name2 == name1: one plane
    _, r = parse("euclidean", "fuzz")                                                      # alone, a bare f inside is fine
    assert r[0]["inner"][0] == {"op": "f", "idx1": 0, "idx2": 0, "fns": (), "ridges": ()} and r[0]["fuzz"] == 0.25
    d, _ = parse("chebyshev+fuzz:name=weight:h=0.5:fuzz=0.1:dscale=0.5", "f1")
    assert d[1] == {"metric": "euclidean", "xforms": (("weight", 0.5, 1.0, 0.25),), "fuzz": 0.1, "scale": 0.25} and "fuzz" not in d[0]
    d, _ = parse("fuzz:name=angle_tanh:fuzz=0.1", "diff2")                                # NoiseType.VORONOI_FUZZ's
    assert d == [{"metric": "angle_tanh", "xforms": (), "idx": 2, "fuzz": 0.1, "scale": 1.0}]
    d, _ = parse(" Angle_Tanh :idx=-3", "cellid")
    assert d[0]["metric"] == "angle_tanh" and d[0]["idx"] == 0


def test_mode_errors_are_the_references(nz):
    parse = nz.VoronoiNoiseGenerator.parse_modes
    with pytest.raises(ValueError, match="Bad Voronoi distance mode manhattan"):
        parse("manhattan", "f1")
    with pytest.raises(ValueError, match="Bad Voronoi result mode f5"):
        parse("euclidean", "f5")
    with pytest.raises(ValueError, match="Bad Voronoi result mode f9"):
        parse("euclidean", "ridge:name=f9")
    with pytest.raises(ValueError, match="Bad mode parameter for fractal_norm distance mode, must be one of: sin, cos"):
        parse("fractal_norm:mode=tan", "f1")
    with pytest.raises(ValueError, match="Bad mode parameter for fractal_norm result mode, must be one of: sin, cos"):
        parse("euclidean", "fractal_norm:mode=tan")
    with pytest.raises(ValueError):
        parse("minkowski:p", "f1")             # a keyword without a value: dict() of a 1-tuple
    with pytest.raises(ValueError):
        parse("minkowski:p=abc", "f1")
    with pytest.raises(IndexError):
        parse("angle:idx=3", "f1")


@pytest.mark.parametrize("dmode, rmode, text", [
    ("euclidean", "median_distance", "median_distance"), ("euclidean", "softmin:use_sorted=1", "use_sorted"),
    ("euclidean", "f:idx=4", "f:idx=4"), ("euclidean", "f:idx=-1", "f:idx=-1"), ("euclidean", "diff:idx2=5", "diff:idx2=5"),
    ("euclidean", "gradient_magnitude:pad_mode=reflect", "pad_mode=replicate only"), ("euclidean", "ridge:name=gradient_magnitude", "outermost"),
    ("euclidean", "fuzz:name=fuzz", "outermost"), ("euclidean", "gradient_magnitude:name1=fuzz", "outermost"),
    ("euclidean", "f1+gradient_magnitude", "beside a bare f term"), ("euclidean", "fuzz+diff2", "beside a bare f term"),
    ("euclidean", "gradient_magnitude:name1=median_distance", "median_distance"),
    ("fuzz+fuzz:name=chebyshev", "diff2", "at most one fuzz term"), ("weight:name=fuzz:__name=chebyshev", "f1", "outermost"),
    ("fuzz:name=fuzz", "f1", "outermost"),
    ("weight:name=fuzz", "f1", "weight:name=fuzz"), ("euclidean", "ridge:name=median_distance", "ridge:name=median_distance")])
def test_refused_modes_name_the_expression(nz, dmode, rmode, text):
    with pytest.raises(NotImplementedError, match=re.escape(text)):
        nz.VoronoiNoiseGenerator.parse_modes(dmode, rmode)


def test_the_statement_refuses_and_errs_alike():
    for dmode, rmode, exc in (("manhattan", "f1", ValueError), ("euclidean", "f5", ValueError), ("fractal_norm:mode=tan", "f1", ValueError),
                              ("euclidean", "fractal_norm:mode=tan", ValueError), ("euclidean", "median_distance", NotImplementedError),
                              ("euclidean", "softmin:use_sorted=1", NotImplementedError), ("euclidean", "f:idx=4", NotImplementedError),
                              ("euclidean", "gradient_magnitude:pad_mode=reflect", NotImplementedError)):
        gen = R.Generator((1, 1, 2, 2), dict(n_points=(5,), distance_mode=(dmode,), result_mode=(rmode,)), lambda s: np.full(s, 0.25, np.float32))
        with pytest.raises(exc):
            gen.generate()


# ------------------------------------------------------------------------------------------------ the public interface
def test_the_generator_and_the_item_exist_with_the_reference_parameters(nz):
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    gen = nz.VoronoiNoiseGenerator
    assert gen.__name__ == "VoronoiNoiseGenerator" and gen.name == "voronoi" and issubclass(gen, ng.NoiseGenerator) and gen.MIN_DIMS == gen.MAX_DIMS == 4
    own = gen.ng_params(no_super=True)
    assert {k: own[k] for k in R.DEFAULTS} == R.DEFAULTS and own["noise_sampler_factory"] is None and own["normalized"] is False
    assert set(gen.ng_params()) == set(own) | set(ng.NoiseGenerator.ng_params())
    assert gen.voronoi_distance_modes == R.DISTANCE_MODES and gen.voronoi_result_modes == R.RESULT_MODES
    item_cls = nz.AdvancedVoronoiNoise
    assert issubclass(item_cls, nz.AdvancedNoiseBase) and item_cls.ns_factory_arg_keys == tuple(own)
    item = item_cls(0.5, custom_noise=None, **cases.ITEM["params"])
    assert item.ns_factory is gen
    with pytest.raises(ValueError, match="Can only handle 4\\+ dimensional latents"):
        item.make_noise_sampler(torch.zeros(4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)
    with pytest.raises(nz.hip_lib.SonarHipError):  # a launchable call on a CPU latent: no host fallback
        item.make_noise_sampler(torch.zeros(1, 4, 8, 8), 0.03, 14.6, seed=1, cpu=True, normalized=True)


def test_a_clone_is_independent(nz):
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    item = nz.AdvancedVoronoiNoise(0.5, custom_noise=chain, **cases.ITEM["params"])
    twin = item.clone()
    assert twin is not item and twin.custom_noise is not chain and twin.custom_noise.items[0] is not chain.items[0]
    assert twin.factor == 0.5 and twin.n_points == (33,) and twin.result_mode == ("diff2",)
    twin.custom_noise.add(nz.CustomNoiseItem(2.0, noise_type="uniform"))
    twin.set_factor(0.25)
    assert len(chain.items) == 1 and item.factor == 0.5


def test_the_registry_is_unchanged(reg, nz):
    assert len(reg.NODE_CLASS_MAPPINGS) == 54 and len(reg.IMPLEMENTED_KEYS) == 42
    off = sorted(k for k, cls in reg.NODE_CLASS_MAPPINGS.items() if cls.__name__.startswith("OffPath_"))
    assert len(off) == 12 and "SonarAdvancedVoronoiNoise" in off and "SonarAdvancedVoronoiNoise" not in reg.IMPLEMENTED_KEYS
    assert len(nz.NoiseType) == 38 and set(nz.NOISE_SAMPLERS) == set(nz.NoiseType)
    for name in ("voronoi_fuzz", "voronoi_mix"):
        with pytest.raises(NotImplementedError):
            nz.get_noise_sampler(name, torch.zeros(1, 4, 8, 8), 0.03, 14.6, cpu=True)


# ------------------------------------------------------------------------------------------------ the entry point
def test_the_entry_point_is_declared_bound_and_exported(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64, "uint64_t": hl.C.c_uint64}
    for name in ("sonar_voronoi_octave_f32", "sonar_voronoi_fuzz_octave_f32", "sonar_voronoi_gradient_f32", "sonar_voronoi_fuzz_add_f32", "sonar_voronoi_acc_f32"):
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert restype is hl.C.c_int and len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), (name, p)
        assert hasattr(hl.load(), name)
    defines = {k: int(v) for k, v in re.findall(r"#define SONAR_VORONOI_(\w+) (\d+)", text)}
    assert {k: defines[f"D_{k.upper()}"] for k in hl.VORONOI_METRICS} == hl.VORONOI_METRICS
    assert {k: defines[f"X_{k.upper()}"] for k in hl.VORONOI_XFORMS} == hl.VORONOI_XFORMS
    assert {k: defines[f"R_{k.upper()}"] for k in hl.VORONOI_OPS} == hl.VORONOI_OPS
    assert (defines["MAX_TERMS"], defines["MAX_CHAIN"], defines["MAX_POINTS"], defines["CHUNK"], defines["FINAL_DIV"]) == (
        hl.VORONOI_MAX_TERMS, hl.VORONOI_MAX_CHAIN, hl.VORONOI_MAX_POINTS, hl.VORONOI_CHUNK, hl.VORONOI_FINAL_DIV)
    assert cases.CHUNK_EDGE == hl.VORONOI_CHUNK + 1
    # the ctypes mirrors have the header's layout: 4-byte fields only, in declaration order
    assert hl.C.sizeof(hl.VoronoiDTerm) == 4 * (3 + 4 * 4 + 3) and hl.C.sizeof(hl.VoronoiRTerm) == 4 * (5 + 4 * 4 + 3)
    assert hl.C.sizeof(hl.VoronoiProgram) == 8 + 4 * hl.C.sizeof(hl.VoronoiDTerm) + 4 * hl.C.sizeof(hl.VoronoiRTerm)
    for struct, cname in ((hl.VoronoiDTerm, "sonar_voronoi_dterm"), (hl.VoronoiRTerm, "sonar_voronoi_rterm"), (hl.VoronoiProgram, "sonar_voronoi_program")):
        body = re.search(rf"typedef struct {cname} \{{(.*?)\}} {cname};", text, flags=re.S).group(1)
        assert re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", body) == [f for f, _t in struct._fields_], cname


def test_bad_arguments_come_back_as_error_codes_without_a_device(pkg, nz):
    """The checks run before anything touches the HIP runtime: the pointers below are never dereferenced."""
    hl = pkg.hip_lib
    lib = hl.load()
    fn = lib.sonar_voronoi_octave_f32
    f, o, a = 4096, 8192, 12288

    def program(dmode="euclidean", rmode="diff2"):
        return hl.voronoi_program(*nz.VoronoiNoiseGenerator.parse_modes(dmode, rmode))

    def call(fp=f, out=o, aux=None, shape=(2, 3, 8, 12), n=33, flags=0, prog=None):
        prog = program() if prog is None else prog
        return fn(fp, out, aux, *shape, n, 1.0, 0.25, 1.0, 1.0, flags, hl.C.addressof(prog) if prog != 0 else None, None)

    assert call(fp=None) == hl.ERR_ARG and call(out=None) == hl.ERR_ARG and call(prog=0) == hl.ERR_ARG
    assert call(out=f) == hl.ERR_ARG and b"out must not be fp" in lib.sonar_last_error()
    assert call(aux=o) == hl.ERR_ARG
    for bad in ((-2, 3, 8, 12), (2, -3, 8, 12), (2, 3, -8, 12), (2, 3, 8, -12), (1 << 31, 3, 8, 12), (2, 3, 8, 1 << 31)):
        assert call(shape=bad) == hl.ERR_ARG, bad
    assert call(shape=(1 << 16, 1 << 15, 1, 1)) == hl.ERR_ARG and call(shape=(1, 1, 1 << 16, 1 << 15)) == hl.ERR_ARG   # 2^31 planes, pixels
    assert call(shape=(1 << 10, 1 << 10, 1 << 10, 2)) == hl.ERR_ARG and b"2^31 output values" in lib.sonar_last_error()
    assert call(n=-1) == hl.ERR_ARG and call(n=0) == hl.ERR_ARG and call(n=1) == hl.ERR_ARG and call(n=1 << 31) == hl.ERR_ARG
    assert call(n=hl.VORONOI_MAX_POINTS + 1) == hl.ERR_UNSUPPORTED
    assert call(flags=2) == hl.ERR_ARG and call(flags=-1) == hl.ERR_ARG
    assert call(prog=program(rmode="cellid")) == hl.ERR_ARG and b"without aux" in lib.sonar_last_error()
    for field, value in (("n_d", 0), ("n_d", 5), ("n_r", 0), ("n_r", 5)):
        prog = program()
        setattr(prog, field, value)
        assert call(prog=prog) == hl.ERR_ARG, (field, value)
    for where, field, value in (("d", "metric", 8), ("d", "metric", -1), ("d", "idx", 3), ("d", "n_xform", 5), ("r", "op", 7), ("r", "op", -1),
                                ("r", "idx1", 4), ("r", "idx2", -1), ("r", "n_fn", 5), ("r", "n_ridge", -1)):
        prog = program()
        setattr(getattr(prog, where)[0], field, value)
        assert call(prog=prog) == hl.ERR_ARG, (where, field, value)
    prog = program(dmode="weight")
    prog.d[0].xform[0] = 3
    assert call(prog=prog) == hl.ERR_ARG
    prog = program(rmode="fractal_norm")
    prog.r[0].fn[0] = 0
    assert call(prog=prog) == hl.ERR_ARG
    for empty in ((0, 3, 8, 12), (2, 0, 8, 12), (2, 3, 0, 12), (2, 3, 8, 0)):   # nothing to launch, whatever N says
        assert call(shape=empty) == 0 and call(shape=empty, n=0) == 0
    with pytest.raises(NotImplementedError, match="at most 4"):
        program(dmode="+".join(["euclidean"] * 5))
    fz, st, u = lib.sonar_voronoi_fuzz_octave_f32, 16384, 20480

    def fcall(fp=f, out=o, aux=None, u_=u, stats=st, shape=(2, 3, 8, 12), n=33, flags=0, prog=None, fpass=2, term=0, value=0.1, stream_id=5, offset=0):
        prog = program() if prog is None else prog
        return fz(fp, out, aux, u_, stats, *shape, n, 1.0, 0.25, 1.0, 1.0, flags, hl.C.addressof(prog) if prog != 0 else None, fpass, term, value,
                  7, stream_id, offset, None)

    assert fcall(stats=None) == hl.ERR_ARG and fcall(stats=o) == hl.ERR_ARG and fcall(stats=f) == hl.ERR_ARG and fcall(stats=u) == hl.ERR_ARG
    assert fcall(u_=o) == hl.ERR_ARG and fcall(fpass=-1) == hl.ERR_ARG and fcall(fpass=3) == hl.ERR_ARG
    assert fcall(term=1) == hl.ERR_ARG and fcall(term=-1) == hl.ERR_ARG and fcall(value=float("nan")) == hl.ERR_ARG
    assert fcall(offset=-1) == hl.ERR_ARG and fcall(offset=1 << 48) == hl.ERR_ARG and fcall(stream_id=1 << 48) == hl.ERR_ARG
    assert fcall(fp=None) == hl.ERR_ARG and fcall(out=None) == hl.ERR_ARG and fcall(prog=0) == hl.ERR_ARG and fcall(out=f) == hl.ERR_ARG
    assert fcall(n=1) == hl.ERR_ARG and fcall(n=hl.VORONOI_MAX_POINTS + 1) == hl.ERR_UNSUPPORTED and fcall(flags=2) == hl.ERR_ARG
    assert fcall(shape=(2, 3, -8, 12)) == hl.ERR_ARG and fcall(shape=(1 << 10, 1 << 10, 1 << 10, 2)) == hl.ERR_ARG
    for fpass in (0, 1, 2):   # an empty output launches nothing; the reducing passes take no output
        assert fcall(shape=(2, 0, 8, 12), fpass=fpass, u_=None) == 0 and fcall(shape=(0, 3, 8, 12), fpass=fpass, out=None if fpass < 2 else o) == 0
    grad, fuzz, acc = lib.sonar_voronoi_gradient_f32, lib.sonar_voronoi_fuzz_add_f32, lib.sonar_voronoi_acc_f32
    assert grad(None, f, o, 6, 8, 12, 1.0, None) == hl.ERR_ARG and grad(f, None, o, 6, 8, 12, 1.0, None) == hl.ERR_ARG
    assert grad(f, f, None, 6, 8, 12, 1.0, None) == hl.ERR_ARG and grad(f, a, f, 6, 8, 12, 1.0, None) == hl.ERR_ARG and grad(a, f, f, 6, 8, 12, 1.0, None) == hl.ERR_ARG
    for bad in ((-6, 8, 12), (6, -8, 12), (6, 8, -12), (1 << 31, 8, 12), (1 << 10, 1 << 11, 1 << 10), (1, 1 << 16, 1 << 15)):
        assert grad(f, f, o, *bad, 1.0, None) == hl.ERR_ARG, bad
    for empty in ((0, 8, 12), (6, 0, 12), (6, 8, 0)):
        assert grad(f, f, o, *empty, 1.0, None) == 0
    assert fuzz(None, f, 8, 0.5, 0.25, None) == hl.ERR_ARG and fuzz(o, None, 8, 0.5, 0.25, None) == hl.ERR_ARG and fuzz(o, o, 8, 0.5, 0.25, None) == hl.ERR_ARG
    assert fuzz(o, f, -1, 0.5, 0.25, None) == hl.ERR_ARG and fuzz(o, f, 1 << 31, 0.5, 0.25, None) == hl.ERR_ARG and fuzz(o, f, 0, 0.5, 0.25, None) == 0
    assert acc(None, f, 8, 1.0, 1.0, 0, None) == hl.ERR_ARG and acc(o, None, 8, 1.0, 1.0, 0, None) == hl.ERR_ARG and acc(o, o, 8, 1.0, 1.0, 0, None) == hl.ERR_ARG
    assert acc(o, f, -1, 1.0, 1.0, 0, None) == hl.ERR_ARG and acc(o, f, 1 << 31, 1.0, 1.0, 0, None) == hl.ERR_ARG and acc(o, f, 8, 1.0, 1.0, 2, None) == hl.ERR_ARG
    assert acc(o, f, 0, 1.0, 1.0, 1, None) == 0
