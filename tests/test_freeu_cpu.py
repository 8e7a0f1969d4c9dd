"""CPU: FreeU Extreme's host logic against the reference's recorded answers (tests/golden/freeu_extreme.npz), the fp64 statement
(tests/freeu_refs.py) against the reference's fp32 outputs, the entry points declared / bound / exported, the unchanged registry, and
patch_model on a stub model."""
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import freeu_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(pkg):
    return importlib.import_module("comfyui_sonar_amd.py.nodes.freeu_extreme")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "freeu_extreme.npz"), allow_pickle=False))


def chain(fx, spec):
    nxt, made = None, []
    for i in reversed(range(len(spec))):
        nxt = fx.FreeUExtremeConfig(**spec[i], frux_config_opt=nxt)
        nxt.tag = i
        made.append(nxt)
    return nxt, made[::-1]


def test_statement_matches_the_reference_in_fp32(g):
    E = R.reference_error(g)
    assert 0 < E < 2.0 ** -20  # a few fp32 roundings of a unit-range output
    for tag, (_shape, kw, fname) in R.CASES.items():
        for d in ("float16", "bfloat16"):  # the reference's own half outputs: a handful of roundings of the dtype
            st = R.apply_ref(torch.from_numpy(g[f"{tag}_x"]).to(getattr(torch, d)).float().numpy(), g.get(f"{tag}_filter") if fname else None, **kw)
            assert R.distance(g[f"{tag}_out_{d}"], st) < 4 * R.HALF_EPS[d]
    assert np.isnan(g["zero_out"]).all()


def test_config_list_and_matching(fx, g):
    head, cfgs = chain(fx, R.CHAIN)
    assert [c.tag for c in head.get_config_list()] == g["chain_list"].tolist()
    bad, _ = chain(fx, R.CHAIN_BAD_HEAD)
    assert [c.tag for c in bad.get_config_list()] == g["chain_bad_head_list"].tolist()
    got = np.array([[bool(c.check_match(*q)) for q in R.QUERIES] for c in cfgs])
    assert np.array_equal(got, g["check_match"])
    c = cfgs[1].clone()
    assert c is not cfgs[1] and all(getattr(c, k) == getattr(cfgs[1], k) for k in c._keys) and repr(c).startswith("<FRUXConfig: {'target': 'skip'")
    assert fx.FreeUExtremeConfig._keys[-2:] == ("sonar_power_filter", "frux_config")


def test_slice_arithmetic(fx):
    mk = lambda **kw: fx.FreeUExtremeConfig(target="both", **kw)  # noqa: E731
    assert mk(slice=0.5).slice_bounds(5) == (0, 2)
    assert mk(slice=0.75, slice_offset=0.5).slice_bounds(8) == (4, 4)
    assert mk(slice=0.25, slice_offset=0.25).slice_bounds(8) == (2, 2)
    assert mk(slice=0.25).slice_bounds(3) == (0, 0)
    assert mk(slice=1.0, slice_offset=1.5).slice_bounds(4)[1] == 0
    for c, s, o in ((8, 0.3, 0.9), (7, 1.0, 0.0), (5, 0.5, 0.5), (6, 2.0, 0.1)):
        c0, cn = mk(slice=s, slice_offset=o).slice_bounds(c)
        assert list(range(c))[R.slice_of(c, s, o)] == list(range(c0, c0 + cn))


def test_handler_sequences_and_out_patch_skip(fx, g, monkeypatch):
    applied = []
    monkeypatch.setattr(fx.FreeUExtremeConfig, "apply", lambda self, idx, x, cache, cpu_fft=False: (applied.append((idx, self.tag)), x)[1])
    head, _ = chain(fx, R.CHAIN)
    inp, mid, outp = fx.make_block_patches(model_channels=R.MODEL_CHANNELS, timestep=lambda s: s, input_config=head, output_config=head)
    assert mid is None
    row = 0
    for ch in R.HANDLER_CHANNELS:
        for sg in R.HANDLER_SIGMAS:
            top = {"sigmas": torch.tensor([sg, sg * 0.5])}
            h, hsp = torch.zeros(1, ch, 2, 2), torch.zeros(1, ch + 1, 2, 2)
            applied.clear()
            assert inp(h, top) is h
            assert [t for _i, t in applied] == [t for t in g["handler_input"][row].tolist() if t >= 0]
            applied.clear()
            a, b = outp(h, hsp, top)
            assert a is h and b is hsp
            assert [t for _i, t in applied] == [t for t in g["handler_output"][row].tolist() if t >= 0]
            assert [i for i, _t in applied] == [i for i in g["handler_output_idx"][row].tolist() if i >= 0]
            row += 1


def test_patch_model_registers_what_is_given(fx):
    calls = []

    class Model:
        model = types.SimpleNamespace(model_config=types.SimpleNamespace(unet_config={"model_channels": 4}))

        def clone(self):
            calls.append("clone")
            return Model()

        def get_model_object(self, name):
            calls.append(name)
            return types.SimpleNamespace(timestep=lambda s: s)

        def set_model_input_block_patch(self, p):
            calls.append("input")

        def set_model_patch(self, p, name):
            calls.append(name)

        def set_model_output_block_patch(self, p):
            calls.append("output")

    cfg = fx.FreeUExtremeConfig(target="both", stage_1=True)
    src = Model()
    m = fx.patch_model(src, cpu_fft=True, middle_config=cfg)
    assert m is not src and calls == ["clone", "model_sampling", "middle_block_patch"]
    calls.clear()
    fx.patch_model(src, input_config=cfg, output_config=cfg)
    assert calls == ["clone", "model_sampling", "input", "output"]
    calls.clear()
    fx.patch_model(src)
    assert calls == ["clone", "model_sampling"]


def test_refusals_without_a_device(fx, pkg):
    hl = pkg.hip_lib
    cfg = fx.FreeUExtremeConfig(target="both", stage_1=True)
    with pytest.raises(hl.SonarHipError, match="ROCm device"):
        cfg.apply(0, torch.zeros(1, 4, 8, 8), {})
    with pytest.raises(NotImplementedError, match="float64"):
        cfg.apply(0, torch.zeros(1, 4, 8, 8, dtype=torch.float64), {})
    with pytest.raises(hl.SonarHipError, match=r"\[B, C, H, W\]"):
        cfg.apply(0, torch.zeros(4, 8, 8), {})
    with pytest.raises(hl.SonarHipError, match="ROCm device"):
        cfg.get_scale(torch.zeros(1, 4, 8, 8))  # hidden_mean is on: the map is made on the device
    assert fx.FreeUExtremeConfig(target="both", hidden_mean=False, scale=1.25).get_scale(torch.zeros(1, 4, 8, 8)) == 1.25


def test_registry_unchanged(pkg):
    reg = importlib.import_module("comfyui_sonar_amd.py.nodes.registry")
    keys = reg.NODE_CLASS_MAPPINGS
    assert len(keys) == 54 and len(reg.IMPLEMENTED_KEYS) == 42 and sum(v.__name__.startswith("OffPath_") for v in keys.values()) == 12
    for k in ("FreeUExtreme", "FreeUExtremeConfig"):
        assert k not in reg.IMPLEMENTED_KEYS and keys[k].__name__ == f"OffPath_{k}"


def test_entry_points_declared_bound_and_exported(pkg):
    hl = pkg.hip_lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64}
    for name, n in (("sonar_freeu_hidden_mean", 12), ("sonar_freeu_apply", 19)):
        decl = re.search(rf"\bint {name}\s*\(([^)]*)\)\s*;", text)
        assert decl is not None, f"{name} is not declared in include/sonar_hip.h"
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        restype, argtypes = hl.SIGNATURES[name]
        assert restype is hl.C.c_int and len(params) == len(argtypes) == n
        for p, a in zip(params, argtypes):
            typ = p.rsplit(" ", 1)[0]
            assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), p
        assert hasattr(hl.load(), name)
    define = lambda nm: int(re.search(rf"#define {nm} (\d+)", text).group(1))  # noqa: E731
    assert (define("SONAR_FREEU_PLAIN"), define("SONAR_FREEU_FUSED"), define("SONAR_FREEU_FILTERED")) == (hl.FREEU_PLAIN, hl.FREEU_FUSED, hl.FREEU_FILTERED)
    lib = hl.load()
    groups = lib.sonar_freeu_hidden_mean_groups
    assert (groups(2, 1280, 1024), groups(2, 320, 16384), groups(2, 320, 256), groups(1, 4, 64), groups(0, 0, 0)) == (16, 1, 10, 1, 1)
    # checked before any launch: the pointers below are never dereferenced
    ok = [0, 0x1000, 1, 4, 8, 8, 256, 64, 0, 4, hl.FREEU_PLAIN, None, None, None, None, 1.0, -1, 1.0, None]
    for pos, bad in ((0, 3), (10, 3), (16, 3), (8, 3), (9, 5), (7, 63), (1, 0x1001)):
        a = list(ok)
        a[pos] = bad
        a[0] = 1 if pos == 1 else a[0]
        assert lib.sonar_freeu_apply(*a) == hl.ERR_ARG, (pos, bad)
    a = list(ok)
    a[4], a[5], a[6], a[7], a[10], a[11] = 5, 7, 140, 35, hl.FREEU_FUSED, 0x2000
    assert lib.sonar_freeu_apply(*a) == hl.ERR_UNSUPPORTED
    a = list(ok)
    a[9] = 0
    assert lib.sonar_freeu_apply(*a) == 0  # an empty window launches nothing
