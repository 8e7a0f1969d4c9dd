"""CPU: reductions over any dims for PowerLawNoiseGenerator's ``div_max_dims`` and scale_noise's ``normalize_dims`` -- the segments the
kernels are handed for every case of tests/golden/reduce_dims.npz, the refusal of a seventh segment (before the draw), the end of the
"adjacent dimensions" refusal, the new entry points declared, bound, exported and replayable, and the golden file against its tables."""
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import reduce_dims_cases as cases  # noqa: E402

ENTRY_POINTS = ("sonar_group_peak_f32", "sonar_group_div_f32", "sonar_group_divided_mean_f32", "sonar_group_scale_noise_f32")
SIG = (torch.tensor(cases.SIGMA[0]), torch.tensor(cases.SIGMA[1]))


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def ng(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise_generation")


@pytest.mark.parametrize("latent,key", sorted(cases.SEGMENTS))
def test_segments_of_every_case(pkg, latent, key):
    sizes, first, groups = pkg.hip_lib.group_segments(cases.SHAPES[latent], cases.DIMS[latent][key])
    assert (sizes, first, groups) == cases.SEGMENTS[(latent, key)]
    assert 1 <= len(sizes) <= pkg.hip_lib.GROUP_MAX_SEGMENTS == 6
    assert int(np.prod(sizes)) == int(np.prod(cases.SHAPES[latent]))
    reduced = [n for k, n in enumerate(sizes) if (k % 2 == 1) != bool(first)]
    assert groups * int(np.prod(reduced)) == int(np.prod(sizes))


def test_the_tables_cover_what_they_claim():
    assert sorted(cases.SEGMENTS) == sorted((latent, key) for latent, table in cases.DIMS.items() for key in table)
    assert max(len(s[0]) for s in cases.SEGMENTS.values()) == 6
    assert {s[1] for s in cases.SEGMENTS.values()} == {0, 1}
    both = {(c["use_sign"], c["use_div_max_abs"], c["alpha"]) for c in cases.POWERLAW.values()}
    assert len(both) == 8
    assert {c["factor"] for c in cases.SCALE.values()} == {1.0, 0.35} and {c["offset"] for c in cases.SCALE.values()} == {False, True}
    for table in (cases.POWERLAW, cases.SCALE):
        assert {(c["latent"], c["dims"]) for c in table.values()} == set(cases.SEGMENTS)


def test_a_seventh_segment_is_refused(pkg, ng):
    hl = pkg.hip_lib
    with pytest.raises(hl.SonarHipError, match="6 segments"):
        hl.group_segments((2, 3, 2, 3, 2, 3, 2), (0, 2, 4, 6))
    with pytest.raises(hl.SonarHipError, match="6 segments"):  # ... by the generator too (before it draws)
        ng.PowerLawNoiseGenerator.div_max_route((0, 2, 4, 6), (2, 3, 2, 3, 2, 3, 2))
    assert ng.PowerLawNoiseGenerator.div_max_route((0, 2, 4), (2, 3, 2, 3, 2, 3, 2)) == ("group", (0, 2, 4))  # six: the last two merge


@pytest.mark.parametrize("shape,dims", [((3, 5, 6, 7), (0, 2)), ((3, 5, 6, 7), (1, 3)), ((3, 5, 6, 7), (0, 3)), ((2, 3, 4, 5, 6), (1, 3))])
def test_non_adjacent_div_max_dims_end_at_the_device_check(nz, ng, shape, dims):
    """On a CPU latent the request is launchable and so ends where every launchable request on a CPU tensor ends; the route it is given is
    the strided pair (the parent commit has no such route: on the device it refuses the request as "adjacent dimensions")."""
    hl = nz.hip_lib
    with pytest.raises(hl.SonarHipError) as caught:
        nz.get_noise_sampler("grey", torch.zeros(shape), 0.03, 14.6, seed=cases.SEED, cpu=True, normalized=False, alpha=2.0,
                             div_max_dims=dims)(*SIG)
    assert "adjacent" not in str(caught.value) and "ROCm device" in str(caught.value)
    assert ng.PowerLawNoiseGenerator.div_max_route(dims, shape) == ("group", tuple(sorted(d % len(shape) for d in dims)))
    assert ng.PowerLawNoiseGenerator.PLAN_STATIC is True


def test_adjacent_div_max_dims_keep_their_route(ng):
    route = lambda dims: ng.PowerLawNoiseGenerator.div_max_route(dims, (3, 4, 16, 12))  # noqa: E731
    assert route(None) is None
    assert route((-3, -2, -1)) == ("mid", 3, 768, 1) and route(()) == ("mid", 1, 2304, 1)
    assert route(0) == ("mid", 1, 3, 768) and route(1) == ("mid", 3, 4, 192) and route((1, 2)) == ("mid", 3, 64, 12)


def test_entry_points_are_declared_bound_exported_and_replayable(pkg):
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
        assert lib.sonar_plan_fn_id(name.encode()) >= 0, f"{name} is not replayable"
        assert lib.sonar_plan_fn_nargs(lib.sonar_plan_fn_id(name.encode())) == len(argtypes)


def test_refused_arguments_come_back_as_error_codes(pkg):
    """Host checks only: nothing is launched, so no device is needed."""
    hl = pkg.hip_lib
    lib = hl.load()
    seven, negative = (7, 1, 2, 2, 2, 2, 2, 2), (2, 1, -1, 21, 1, 1, 1, 1)
    for seg in (seven, negative):
        assert lib.sonar_group_peak_f32(None, *seg, 1, None, None, None) == hl.ERR_ARG
        assert lib.sonar_group_div_f32(None, *seg, None, None) == hl.ERR_ARG
        assert lib.sonar_group_divided_mean_f32(None, *seg, None, None, None, None) == hl.ERR_ARG
        assert lib.sonar_group_scale_noise_f32(None, *seg, None, None, 1.0, None) == hl.ERR_ARG
    ok = (2, 1, 30, 24, 1, 1, 1, 1)
    assert lib.sonar_group_peak_f32(None, *ok, 1, None, None, None) == hl.ERR_ARG          # no tensor
    assert lib.sonar_group_div_f32(None, *ok, None, None) == hl.ERR_ARG
    assert lib.sonar_group_peak_f32(None, 2, 1, 0, 24, 1, 1, 1, 1, 1, None, None, None) == 0  # an empty tensor launches nothing
    assert lib.sonar_group_scale_noise_f32(None, 2, 1, 0, 24, 1, 1, 1, 1, None, None, 1.0, None) == 0


def test_scale_noise_with_non_trailing_dims_on_a_cpu_tensor_raises_sonar_hip_error(pkg):
    utils = importlib.import_module("comfyui_sonar_amd.py.utils")
    for dims in ((0, 2), (1, 3), (-1,)):
        with pytest.raises(pkg.hip_lib.SonarHipError):
            utils.scale_noise(torch.randn(3, 5, 6, 7), 1.0, normalized=True, normalize_dims=dims)


def test_the_golden_file_and_the_case_tables_agree():
    g = np.load(os.path.join(ROOT, "tests", "golden", "reduce_dims.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta_json"]))
    assert sorted(meta) == sorted([f"pl_{n}" for n in cases.POWERLAW] + [f"sn_{n}" for n in cases.SCALE])
    for latent, shape in cases.SHAPES.items():
        assert tuple(g[f"draw_{latent}"].shape) == shape and torch.equal(torch.from_numpy(g[f"draw_{latent}"]), cases.draw(torch, latent))
    for name, case in cases.POWERLAW.items():  # the stored output is the stored pre-division tensor over its amax: an exact division
        pre = torch.from_numpy(g[cases.pre_key(case)])
        peak = torch.amax(pre.abs() if case["use_div_max_abs"] else pre, dim=tuple(cases.DIMS[case["latent"]][case["dims"]]), keepdim=True)
        assert torch.equal(torch.from_numpy(g["pl_" + name]), pre / peak), name
    for prefix, table in (("pl_", cases.POWERLAW), ("sn_", cases.SCALE)):
        for name, case in table.items():
            m, out = meta[prefix + name], g[prefix + name]
            assert all(m[k] == v for k, v in case.items() if k != "dims") and m["dims"] == list(cases.DIMS[case["latent"]][case["dims"]])
            assert out.dtype == np.float32 and tuple(out.shape) == cases.SHAPES[case["latent"]]
    seen = set()
    for name, case in cases.SCALE.items():
        m = meta["sn_" + name]
        if m["all_nan"]:
            assert np.isnan(g["sn_" + name]).all()
            continue
        assert np.isfinite(g["sn_" + name]).all() and m["reference_fp32_error"] <= m["bound"]
        if case["offset"]:
            flags = g["flags_" + name]
            assert flags.size == cases.SEGMENTS[(case["latent"], case["dims"])][2] and 0 < int(flags.sum()) < flags.size
            seen |= set(flags.tolist())
    assert seen == {0, 1}
