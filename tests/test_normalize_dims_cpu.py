"""CPU: NormalizeToScaleNoise with any ``mean_dims`` / ``std_dims`` -- what torch refuses is refused with torch's exception types before the
device check, a launchable call on a CPU tensor still raises SonarHipError, the registry is unchanged, the strided entry points
(csrc/group_stats.hip) are declared, bound, exported and replayable, the segment collapse, and the golden file against its case table."""
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
import normalize_dims_cases as cases  # noqa: E402

ENTRY_POINTS = ("sonar_group_stats_f32", "sonar_group_affine_f32", "sonar_group_minmax_rescale_f32", "sonar_group_adjust_f32")
SIG = (torch.tensor(cases.SIGMA[0]), torch.tensor(cases.SIGMA[1]))


@pytest.fixture(scope="module")
def nz(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.noise")


@pytest.fixture(scope="module")
def reg(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry")


def _item(nz, case):
    chain = nz.CustomNoiseChain()
    chain.add(nz.CustomNoiseItem(1.0, noise_type="gaussian"))
    return nz.NormalizeToScaleNoise(case["factor"], noise=chain, **cases.item_kwargs(case))


@pytest.mark.parametrize("name", sorted(n for n, c in cases.CASES.items() if c["error"]))
def test_what_torch_refuses_is_refused_with_its_exception_type(nz, name):
    """On a CPU latent: the dims are checked before anything asks where the tensor lives.  torch itself is asked the same question."""
    case = cases.CASES[name]
    want = {"RuntimeError": RuntimeError, "IndexError": IndexError}[case["error"]]
    x = torch.zeros(cases.LATENTS[case["latent"]])
    with pytest.raises(want) as torch_says:
        x.mean(dim=case["mean_dims"], keepdim=True)
        x.std(dim=case["std_dims"], keepdim=True)
    assert type(torch_says.value) is want
    with pytest.raises(want) as ours:
        _item(nz, case).make_noise_sampler(x, 0.03, 14.6, seed=1, cpu=True, normalized=True)
    assert type(ours.value) is want and not isinstance(ours.value, nz.hip_lib.SonarHipError)


def test_a_dimension_a_skipped_step_names_is_not_checked(nz):
    """mean_multiplier == 0 skips the step in the reference, so its dims are never handed to torch."""
    case = dict(cases.CASES["g_out_of_range"], mean_multiplier=0.0, std_dims=(0,))
    with pytest.raises(nz.hip_lib.SonarHipError):  # the call is launchable: on the CPU it ends at the device check
        _item(nz, case).make_noise_sampler(torch.zeros(cases.LATENTS["l4"]), 0.03, 14.6, seed=1, cpu=True, normalized=True)(*SIG)


@pytest.mark.parametrize("name", ["a_l4_0", "a_l4_m3_m2_m1", "c_simple_1"])
def test_a_launchable_call_on_a_cpu_tensor_raises_sonar_hip_error(nz, name):
    case = cases.CASES[name]
    with pytest.raises(nz.hip_lib.SonarHipError):
        _item(nz, case).make_noise_sampler(torch.zeros(cases.LATENTS[case["latent"]]), 0.03, 14.6, seed=1, cpu=True, normalized=True)(*SIG)


def test_the_registry_is_unchanged(reg):
    assert len(reg.NODE_CLASS_MAPPINGS) == 54 and len(reg.IMPLEMENTED_KEYS) == 42
    assert "SonarNormalizeNoiseToScale" in reg.IMPLEMENTED_KEYS
    off = sorted(k for k, cls in reg.NODE_CLASS_MAPPINGS.items() if cls.__name__.startswith("OffPath_"))
    assert len(off) == 12 and not set(off) & set(reg.IMPLEMENTED_KEYS)


def test_entry_points_are_declared_bound_exported_and_replayable(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64}
    lib = hl.load()
    for name in (*ENTRY_POINTS, "sonar_group_stats_ws_doubles"):
        decl = re.search(rf"\b(int|int64_t) {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [" ".join(p.split()) for p in decl.group(2).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert restype is kinds[decl.group(1)] and len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), (name, p)
        assert hasattr(lib, name), f"{name} is not exported by the built library"
    for name in ENTRY_POINTS:
        assert lib.sonar_plan_fn_id(name.encode()) >= 0, f"{name} is not replayable"
        assert lib.sonar_plan_fn_nargs(lib.sonar_plan_fn_id(name.encode())) == len(hl.SIGNATURES[name][1])
    assert "sonar_group_stats_ws_doubles" in hl._HOST_QUERIES
    assert int(re.search(r"#define SONAR_GROUP_MAX_SEGMENTS (\d+)", text).group(1)) == hl.GROUP_MAX_SEGMENTS == 6
    assert os.path.exists(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "group_stats.hip"))


def test_segment_collapse(pkg):
    """Adjacent dimensions of one kind merge, size-1 dimensions drop, the kinds alternate; groups = the kept sizes' product."""
    seg = pkg.hip_lib.group_segments
    assert seg((512, 4, 128, 128), (0,)) == ([512, 65536], 1, 65536)
    assert seg((512, 4, 128, 128), (1,)) == ([512, 4, 16384], 0, 512 * 16384)
    assert seg((512, 4, 128, 128), (0, 2, 3)) == ([512, 4, 16384], 1, 4)
    assert seg((512, 4, 128, 128), (-2,)) == ([2048, 128, 128], 0, 2048 * 128)
    assert seg((512, 4, 128, 128), ()) == ([512 * 4 * 128 * 128], 1, 1)
    assert seg((512, 4, 128, 128), (1, 2, 3)) == ([512, 65536], 0, 512)
    assert seg((1, 3, 4, 5), (0,)) == ([60], 0, 60)                      # the reduced dimension has one member
    assert seg((2, 1, 3, 1, 4), (0, 4)) == ([2, 3, 4], 1, 3)             # size-1 dimensions between the others
    assert seg((2, 3, 2, 3, 2, 3), (0, 2, 4)) == ([2, 3, 2, 3, 2, 3], 1, 27)
    assert seg((2, 3, 2, 3, 2, 3), (1, 3, 5)) == ([2, 3, 2, 3, 2, 3], 0, 8)
    assert seg((1, 1), (0,)) == ([1], 0, 1) and seg((), ()) == ([1], 0, 1)
    assert seg((0, 4), (0,)) == ([0, 4], 1, 4)
    with pytest.raises(pkg.hip_lib.SonarHipError, match="6 segments"):
        seg((2, 3, 2, 3, 2, 3, 2), (0, 2, 4, 6))
    with pytest.raises(IndexError):
        seg((2, 3), (2,))
    with pytest.raises(RuntimeError):
        seg((2, 3), (1, -1))


def test_workspace_query(pkg):
    """Host arithmetic only: unsplit shapes need none, split ones S x groups per stored plane; bad arguments come back as error codes."""
    hl = pkg.hip_lib
    lib = hl.load()
    q = lib.sonar_group_stats_ws_doubles
    assert q(2, 1, 30, 24, 1, 1, 1, 1, 1, 0) == 0                      # 24 lanes walk 30 members each
    assert q(2, 1, 2049, 21, 1, 1, 1, 1, 1, 0) == 33 * 21 * 2          # (2049, 3, 7) over (0,): 33 slices of 63
    assert q(2, 1, 2049, 21, 1, 1, 1, 1, 1, 1) == 33 * 21 * 4
    assert q(3, 1, 5, 3, 700, 1, 1, 1, 1, 0) == 4 * 3 * 2              # (5, 3, 700) over (0, 2): 4 slices of 875
    assert q(2, 0, 24, 1024, 1, 1, 1, 1, 1, 0) == 0                    # runs of 1024: one wave each
    assert q(2, 0, 24, 1025, 1, 1, 1, 1, 0, 1) == 2 * 24 * 2
    assert q(2, 1, 0, 21, 1, 1, 1, 1, 1, 1) == 0
    assert q(0, 1, 1, 1, 1, 1, 1, 1, 1, 0) == hl.ERR_ARG and q(7, 1, 2, 2, 2, 2, 2, 2, 1, 0) == hl.ERR_ARG
    assert q(2, 1, -1, 21, 1, 1, 1, 1, 1, 0) == hl.ERR_ARG
    assert q(2, 1, 1 << 16, 1 << 15, 1, 1, 1, 1, 1, 0) == hl.ERR_UNSUPPORTED


def test_the_golden_file_and_the_case_table_agree():
    g = np.load(os.path.join(ROOT, "tests", "golden", "normalize_dims.npz"), allow_pickle=False)
    meta = json.loads(str(g["meta_json"]))
    assert sorted(meta) == sorted(cases.CASES)
    for latent, shape in cases.LATENTS.items():
        assert tuple(g[f"planes_{latent}"].shape) == shape
        assert torch.equal(torch.from_numpy(g[f"planes_{latent}"]), cases.planted(torch, latent))
    for name, case in cases.CASES.items():
        m = meta[name]
        for key, value in case.items():
            assert m[key] == (list(value) if isinstance(value, tuple) else value), (name, key)
        if case["error"]:
            assert m["reference_error"]["type"] == case["error"] and f"out_{name}" not in g
            continue
        out = g[f"out_{name}"]
        assert m["reference_error"] is None and out.dtype == np.float32 and tuple(out.shape) == cases.LATENTS[case["latent"]]
        if case["all_nan"]:
            assert np.isnan(out).all()
        else:
            assert np.isfinite(out).all() and m["reference_fp32_error"] <= m["bound"]
    # every family of the table is there
    trailing = [n for n, c in cases.CASES.items() if not c["error"] and sorted(d % 4 for d in c["mean_dims"]) == [1, 2, 3] and c["latent"] == "l4"]
    assert trailing and any(c["mode"] == "simple" for c in cases.CASES.values()) and any(c["mean_dims"] != c["std_dims"] for c in cases.CASES.values())
