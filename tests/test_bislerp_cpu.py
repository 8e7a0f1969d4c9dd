"""CPU: bislerp without a device -- hip_lib's axis-table builder against the definition, the known values of the fp64 statement
(tests/bislerp_refs.py), the entry point's declaration, the unchanged refusal of ``scale_samples`` and the four presets' construction.
tests/test_gpu_bislerp.py holds the kernel, ``utils.bislerp`` and the presets to the same statement.

**Parity unpinned**: the reference calls ComfyUI's ``bislerp`` through ``common_upscale`` and vendors no ComfyUI, and none is installed
where these tests run (``import comfy.utils`` fails), so no goldens exist; the statement in tests/bislerp_refs.py is what is built.

The kernel cases' Gaussian seeds (``bislerp_refs.case_seed``) are chosen so that the statement leaves no pixel out of a comparison: no
fp64 dot lies within 2e-6 of a threshold (asserted below).  Over those cases the statement in fp32 lies within 1.235e-05 (relative to the
summed norms of a pixel's four source vectors) of the statement in fp64; the kernel's bound is four times the figure the run measures."""
import importlib
import math
import os
import re

import pytest
import torch

from tests import bislerp_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sonar_bislerp_acc_f32"
PRESETS = ("pyramid_bislerp", "highres_pyramid_bislerp", "pyramid_old_bislerp", "pyramid_mix_bislerp")


@pytest.fixture(scope="module")
def hl(pkg):
    return pkg.hip_lib


# ------------------------------------------------------------------------------------------------ tables
def test_the_table_builder_is_the_definition_bit_for_bit(hl):
    for old in range(1, 41):
        for new in range(1, 41):
            got, want = hl.bislerp_axis(old, new), R.axis_tables(old, new)
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and g.shape == w.shape == (new,) and torch.equal(g, w), (old, new)
            c1, c2, ratio = got
            assert int(c1.min()) >= 0 and int(c2.max()) <= old - 1 and bool((c2 >= c1).all()) and bool(((ratio >= 0) & (ratio < 1)).all())


# ------------------------------------------------------------------------------------------------ known values of the statement
KNOWN = R.known_inputs()
TIGHT = 1e-12  # fp64 rounding of a handful of operations on values of order 1


def _ratios(old, new):
    return R.axis_tables(old, new)[2].double()


def test_same_size_is_the_identity():
    src, W, H = KNOWN["same_size"]
    out, _ = R.bislerp(src, W, H)
    assert float((out - src.double()).abs().max()) <= TIGHT * float(src.abs().max())


def test_one_channel_takes_the_first_sample_or_the_linear_mix():
    src, W, H = KNOWN["one_channel"]
    S = src.double()
    out, dots = R.bislerp(src, W, H)
    assert bool((dots.abs() == 1.0).all())  # every dot is exactly +-1: no pixel near a threshold

    def axis(t, dim, new):  # b1 where the two samples have the same sign, the linear mix where they differ
        c1, c2, r = R.axis_tables(t.shape[dim], new)
        shape = [1, 1, 1, 1]
        shape[dim] = new
        r = r.double().reshape(shape)
        b1, b2 = t.index_select(dim, c1), t.index_select(dim, c2)
        return torch.where(b1 * b2 > 0, b1, b1 * (1.0 - r) + b2 * r)

    want = axis(axis(S, 3, W), 2, H)
    assert float((out - want).abs().max()) <= TIGHT * float(S.abs().max())


@pytest.mark.parametrize("name", ["zero_then_vector", "zero_then_vector_c16"])
def test_a_zero_vector_beside_a_vector(name):
    src, W, H = KNOWN[name]
    v = src[0, :, 0, 1].double()
    c1, c2, r = R.axis_tables(2, W)
    out, _ = R.bislerp(src, W, H)
    for X in range(W):
        rx = float(r[X])
        want = v * (math.sin(rx * math.pi / 2) * rx) if (int(c1[X]), int(c2[X])) == (0, 1) else v
        assert (int(c1[X]), int(c2[X])) in ((0, 1), (1, 1))
        for Y in range(H):  # the rows are copies: the height pass sees identical (or zero) neighbours
            assert float((out[0, :, Y, X] - want).abs().max()) <= TIGHT * float(v.abs().max()), (X, Y)


def test_identical_neighbours_give_the_first():
    src, W, H = KNOWN["identical"]
    out, _ = R.bislerp(src, W, H)
    assert torch.equal(out, src[0, :, 0, 0].double().reshape(1, -1, 1, 1).expand_as(out))


def test_negated_neighbours_give_the_linear_mix():
    src, W, H = KNOWN["negated"]
    v = src[0, :, 0, 0].double()
    c1, c2, r = R.axis_tables(2, W)
    out, _ = R.bislerp(src, W, H)
    for X in range(W):
        rx = float(r[X])
        want = v * (1.0 - rx) + (-v) * rx if (int(c1[X]), int(c2[X])) == (0, 1) else -v
        assert float((out[0, :, 0, X] - want).abs().max()) <= TIGHT * float(v.abs().max()), X


def test_the_kernel_cases_leave_no_pixel_out_and_fix_the_bound():
    left_out = 0
    for index, (_src, (H, W)) in enumerate(R.SIZES):
        for C in R.CHANNELS:
            src, _base, _ = R.case_input(index, C)
            _, dots = R.bislerp(src, W, H)
            left_out += int(R.near_threshold(dots).sum())
    assert left_out == 0
    err = R.fp32_statement_error()
    print(f"fp32 statement against the fp64 statement over the kernel cases: {err:.3e} (kernel bound {R.kernel_bound():.3e})")
    assert 0.0 < err < 1e-3  # an fp32 restatement of order-1 values: anything larger is a mistake in the statement itself


# ------------------------------------------------------------------------------------------------ the entry point
def test_the_entry_point_is_declared_bound_and_exported(hl):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sonar_hip.h")).read(), flags=re.S)
    kinds = {"float": hl.C.c_float, "double": hl.C.c_double, "int": hl.C.c_int, "int64_t": hl.C.c_int64, "uint64_t": hl.C.c_uint64}
    decl = re.search(rf"\bint {NAME}\s*\(([^)]*)\)\s*;", text)
    assert decl is not None, f"{NAME} is not declared in include/sonar_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = hl.SIGNATURES[NAME]
    assert restype is hl.C.c_int and len(params) == len(argtypes) == 18
    for p, a in zip(params, argtypes):
        typ = p.rsplit(" ", 1)[0]
        assert a is (hl.C.c_void_p if "*" in typ else kinds[typ]), p
    assert hasattr(hl.load(), NAME) and callable(hl.bislerp_acc_) and callable(hl.bislerp_tables)
    assert hl.BISLERP == "bislerp" and hl.BISLERP not in hl.UPSCALE_MODES and hl.LEVEL_MODES == hl.UPSCALE_MODES + ("bislerp",)


def test_bad_arguments_come_back_as_error_codes_without_a_device(hl):
    """The checks run before anything touches the HIP runtime: the pointers below are never dereferenced."""
    fn = hl.load().sonar_bislerp_acc_f32
    p = 4096
    good = [p, p, 1, 4, 8, 8, 4, 4, 1.0, 0, p, p, p, p, p, p, None, None]
    for at, bad in ((0, None), (1, None), (2, -1), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (10, None), (15, None)):
        args = list(good)
        args[at] = bad
        assert fn(*args) == hl.ERR_ARG, at
    args = list(good)
    args[4] = 1 << 24
    assert fn(*args) == hl.ERR_UNSUPPORTED
    args = list(good)
    args[2] = 0  # an empty batch: nothing to launch
    assert fn(*args) == 0


# ------------------------------------------------------------------------------------------------ what stays refused, what is accepted
def test_scale_samples_still_refuses_with_the_switch_off(pkg):
    utils = importlib.import_module("comfyui_sonar_amd.py.utils")
    assert utils.BISLERP_IN_SCALE_SAMPLES is (os.environ.get("SONAR_BISLERP_SCALE", "0") != "0")
    before = utils.BISLERP_IN_SCALE_SAMPLES
    utils.BISLERP_IN_SCALE_SAMPLES = False
    try:
        with pytest.raises((NotImplementedError, pkg.hip_lib.SonarHipError)):  # (a CPU tensor is refused first, as for every mode)
            utils.scale_samples(torch.zeros(1, 4, 4, 4), 8, 8, mode="bislerp")
    finally:
        utils.BISLERP_IN_SCALE_SAMPLES = before
    assert callable(utils.bislerp) and "bislerp" in utils.UPSCALE_METHODS


def test_the_presets_are_registered_and_their_generators_take_the_mode(pkg):
    """A sampler is only built on a device latent (tests/test_gpu_bislerp.py does); without one: the four registry entries exist, and a
    generator whose ``upscale_mode`` is bislerp gets past the mode check of ``generate`` -- a bare object then fails on its first missing
    attribute, where it used to raise the NotImplementedError of the refusal -- while an unknown mode is still refused."""
    nz = importlib.import_module("comfyui_sonar_amd.py.noise")
    for name in PRESETS:
        assert callable(nz.NOISE_SAMPLERS[nz.NoiseType[name.upper()]])
    for cls in (nz.PyramidNoiseGenerator, nz.HighresPyramidNoiseGenerator, nz.PyramidOldNoiseGenerator):
        gen = object.__new__(cls)
        gen.upscale_mode = "bislerp"
        with pytest.raises(AttributeError):
            gen.generate(None, None)
        gen.upscale_mode = "lanczos"
        with pytest.raises(NotImplementedError):
            gen.generate(None, None)
    gen = object.__new__(nz.PyramidNoiseGenerator)
    gen.upscale_mode, gen.cpu = "bislerp", True
    assert gen.generate_normalized(1.0) is None and gen.generate_raw_stats() is None  # replay mode: the caller takes the ordinary path
