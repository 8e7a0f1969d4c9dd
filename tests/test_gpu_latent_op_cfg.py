"""GPU: SonarApplyLatentOperationCFG.  The two fused kernels (hip_lib.cfg_op_prepare / cfg_op_finish) against the same arithmetic written
in torch on the device -- on the shapes where they can go wrong: a vector that straddles the sample boundary, a tail only, several blocks,
unaligned views, no elements -- their argument checks, and the node through every case of tests/golden/latent_op_cfg.npz (the reference's
own values, tests/golden/make_latent_op_cfg_golden.py), the objects its disabled paths hand back, and float16 / bfloat16 predictions."""
import ctypes
import importlib
import json
import zlib

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.golden import latent_op_cfg_cases as lc

pytestmark = pytest.mark.gpu

TOL = 4e-6  # the standing bar for elementwise compositions (tests/test_gpu_quantile.py)
# (shape, views offset by one element from a 16-byte boundary)
SHAPES = {"straddle_2x3x5x7": ((2, 3, 5, 7), False), "tail_1x1x1x3": ((1, 1, 1, 3), False), "blocks_2x4x64x64": ((2, 4, 64, 64), False),
          "unaligned_2x3x5x7": ((2, 3, 5, 7), True), "unaligned_2x4x16x16": ((2, 4, 16, 16), True), "inner_below_vector_5x3": ((5, 3), False),
          "empty_0x4x8x8": ((0, 4, 8, 8), False), "empty_2x0x3": ((2, 0, 3), False)}
SIGMAS = ("none", "one", "per_sample")
GRID = [(s, t2, sig) for s in SHAPES for t2 in (False, True) for sig in SIGMAS]
GRID_IDS = [f"{s}-{'t2' if t2 else 'not2'}-sigma_{sig}" for s, t2, sig in GRID]


def _golden():
    g = np.load(f"{GOLDEN}/latent_op_cfg.npz", allow_pickle=False)
    return g, json.loads(str(g["meta_json"]))


def _close(got, want, what=""):
    peak = float(want.abs().max()) if want.numel() else 1.0
    torch.testing.assert_close(got, want, rtol=TOL, atol=TOL * max(1.0, peak), msg=lambda m: f"{what}: {m}")


def _tensor(shape, offset, gen, scale=1.0):
    """A contiguous device tensor of ``shape``; ``offset``: a view that starts 4 bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    flat = (torch.randn(n + 1, generator=gen) * scale).cuda()
    t = flat[1:] if offset else flat[:n]
    assert t.data_ptr() % 16 == (4 if offset else 0) or n == 0
    return t.view(shape)


def _operands(shape_key, with_t2, sigma_kind):
    shape, offset = SHAPES[shape_key]
    gen = torch.Generator().manual_seed(zlib.crc32(repr((shape_key, with_t2, sigma_kind)).encode()))
    x, t1, t2, res = (_tensor(shape, offset, gen) for _ in range(4))
    batch = shape[0]
    sigma = None
    if sigma_kind == "one":
        sigma = torch.tensor([3.7], device="cuda")
    elif sigma_kind == "per_sample":
        sigma = (torch.rand(batch, generator=gen) * 9.0 + 0.5).cuda()
    return x, t1, (t2 if with_t2 else None), res, sigma


def _bcast(sigma, like):
    return sigma.reshape(-1, *((1,) * (like.ndim - 1)))


def _torch_prepare(x, t1, t2, sigma):
    def f(t):
        return (x - t) / _bcast(sigma, t) if sigma is not None else t

    f2 = None if t2 is None else f(t2) + 0.0
    return (f(t1) - f2 if t2 is not None else f(t1) + 0.0), f2


def _torch_finish(result, t2f, x, sigma, t1_orig, mode, w):
    r = result + t2f if t2f is not None else result
    if sigma is not None:
        r = x - _bcast(sigma, r) * r
    if mode is None:
        return r + 0.0
    return {"lerp": lambda: torch.lerp(t1_orig, r, w), "inject": lambda: t1_orig + r * w, "subtract_b": lambda: t1_orig - r * w}[mode]()


@pytest.mark.parametrize("shape_key,with_t2,sigma_kind", GRID, ids=GRID_IDS)
def test_prepare_against_torch(pkg, shape_key, with_t2, sigma_kind):
    hl = pkg.hip_lib
    x, t1, t2, _, sigma = _operands(shape_key, with_t2, sigma_kind)
    before = [None if t is None else t.clone() for t in (x, t1, t2, sigma)]
    result, t2f = hl.cfg_op_prepare(x, t1, t2, sigma)
    torch.cuda.synchronize()
    want, want2 = _torch_prepare(x, t1, t2, sigma)
    assert result.dtype == torch.float32 and result.shape == t1.shape and result.data_ptr() not in {t.data_ptr() for t in (x, t1) if t.numel()}
    _close(result, want, "result")
    assert (t2f is None) == (t2 is None)
    if t2 is not None:
        assert t2f.dtype == torch.float32 and t2f.shape == t2.shape and (t2f.data_ptr() != t2.data_ptr() or not t2.numel())
        _close(t2f, want2, "t2_out")
    for t, b in zip((x, t1, t2, sigma), before):
        assert t is None or torch.equal(t, b), "an input changed"


@pytest.mark.parametrize("shape_key,with_t2,sigma_kind", GRID, ids=GRID_IDS)
def test_finish_against_torch(pkg, shape_key, with_t2, sigma_kind):
    hl = pkg.hip_lib
    x, t1_orig, t2f, result, sigma = _operands(shape_key, with_t2, sigma_kind)
    before = [None if t is None else t.clone() for t in (x, t1_orig, t2f, result, sigma)]
    for mode, w in ((None, 0.5), ("lerp", 0.3), ("lerp", 0.8), ("inject", 0.6), ("subtract_b", -0.4)):
        out = hl.cfg_op_finish(result, t2f, x, sigma, t1_orig, mode, w)
        torch.cuda.synchronize()
        assert out.dtype == t1_orig.dtype and out.shape == t1_orig.shape
        assert not out.numel() or out.data_ptr() not in {t.data_ptr() for t in (x, t1_orig, result)}
        _close(out, _torch_finish(result, t2f, x, sigma, t1_orig, mode, w), f"{mode} {w}")
    assert torch.equal(hl.cfg_op_finish(result, t2f, x, sigma, t1_orig, "none", 0.5), hl.cfg_op_finish(result, t2f, x, sigma, t1_orig, None, 0.0))
    for t, b in zip((x, t1_orig, t2f, result, sigma), before):
        assert t is None or torch.equal(t, b), "an input changed"


def test_blend_is_sonar_blend(pkg):
    """The finish kernel evaluates the blend with the device function of sonar_blend_f32: without t2 and flip the bits are hip_lib.blend's."""
    hl = pkg.hip_lib
    x, t1_orig, _, result, _ = _operands("blocks_2x4x64x64", False, "none")
    for mode, w in (("lerp", 0.3), ("lerp", 0.8), ("lerp", -0.6), ("inject", 0.6), ("subtract_b", 1.3)):
        assert torch.equal(hl.cfg_op_finish(result, None, None, None, t1_orig, mode, w), hl.blend(mode, t1_orig, result, w)), (mode, w)


def test_bad_arguments(pkg):
    hl = pkg.hip_lib
    lib = hl.load()
    t = [torch.zeros(24, device="cuda") for _ in range(6)]
    x, t1, t2, res, t2o, out = (v.data_ptr() for v in t)
    sig = torch.ones(8, device="cuda").data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def prepare(dtype=0, x=x, t1=t1, t2=t2, sigma=None, sigma_n=1, result=res, t2_out=t2o, n=24, inner=12):
        return lib.sonar_cfg_op_prepare(dtype, x, t1, t2, sigma, sigma_n, result, t2_out, n, inner, st)

    def finish(dtype=0, result=res, t2=t2o, x=x, sigma=None, sigma_n=1, t1_orig=t1, blend=0, w=0.5, out=out, n=24, inner=12):
        return lib.sonar_cfg_op_finish(dtype, result, t2, x, sigma, sigma_n, t1_orig, blend, w, out, n, inner, st)

    assert prepare() == 0 and finish() == 0 and prepare(sigma=sig, sigma_n=2) == 0 and finish(sigma=sig, sigma_n=2) == 0
    assert prepare(n=0, inner=1) == 0 and finish(n=0, inner=1) == 0  # nothing to do is not an error
    assert prepare(x=None) == 0 and prepare(t2=None, t2_out=None) == 0 and finish(t2=None) == 0 and finish(blend=-1, t1_orig=None) == 0
    for call in (prepare, finish):
        for bad in (dict(n=-1), dict(inner=0), dict(inner=-12), dict(inner=5), dict(inner=48), dict(sigma=sig, sigma_n=3), dict(sigma=sig, sigma_n=0),
                    dict(sigma=sig, sigma_n=2, x=None), dict(dtype=3), dict(dtype=-1), dict(result=None)):
            assert call(**bad) == hl.ERR_ARG, (call.__name__, bad)
            assert call.__name__ in lib.sonar_last_error().decode()
    for bad in (dict(t1=None), dict(t2_out=None)):
        assert prepare(**bad) == hl.ERR_ARG, bad
    for bad in (dict(blend=3), dict(blend=-2), dict(t1_orig=None), dict(out=None)):
        assert finish(**bad) == hl.ERR_ARG, bad
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0.0 for v in t)


def test_wrapper_refusals(pkg):
    hl = pkg.hip_lib
    a, b = torch.zeros(2, 4, 6, device="cuda"), torch.zeros(2, 4, 5, device="cuda")
    three = torch.ones(3, device="cuda")
    with pytest.raises(hl.SonarHipError, match="shape mismatch"):
        hl.cfg_op_prepare(a, a, b, None)
    with pytest.raises(hl.SonarHipError, match="shape mismatch"):
        hl.cfg_op_prepare(b, a, None, three[:1])
    with pytest.raises(hl.SonarHipError, match="3 sigmas for a batch of 2"):
        hl.cfg_op_prepare(a, a, None, three)
    with pytest.raises(hl.SonarHipError, match="shape mismatch"):
        hl.cfg_op_finish(a, None, None, None, b, "lerp", 0.5)
    with pytest.raises(hl.SonarHipError, match="3 sigmas for a batch of 2"):
        hl.cfg_op_finish(a, None, a, three, a, "lerp", 0.5)
    with pytest.raises(hl.SonarHipError):
        hl.cfg_op_prepare(None, a.cpu(), None, None)
    with pytest.raises(hl.SonarHipError, match="float64"):
        hl.cfg_op_prepare(None, a.double(), None, None)
    with pytest.raises(hl.SonarHipError, match="contiguous"):
        hl.cfg_op_prepare(None, a.transpose(1, 2), None, None)
    with pytest.raises(hl.SonarHipError):
        hl.cfg_op_prepare(a.half(), a, None, three[:1])  # one dtype for x, t1 and t2
    with pytest.raises(KeyError):
        hl.cfg_op_finish(a, None, None, None, a, "no_such_blend", 0.5)


# ------------------------------------------------------------------------------------------------ the node
def _mappings():
    return importlib.import_module("comfyui_sonar_amd.py.nodes.registry").NODE_CLASS_MAPPINGS


def _check_case(g, entry, key, tensors, dtype=torch.float32):
    before = {k: v.clone() for k, v in tensors.items()}
    base, model, result, args = lc.run_case(_mappings(), entry, tensors)
    torch.cuda.synchronize()
    assert model is not base and model.hooks() == entry["hooks"] and base.hooks() == {"post_cfg": 0, "pre_cfg": 0, "unet_wrapper": 0}
    for k, v in tensors.items():
        assert torch.equal(v, before[k]), f"{k} was written through"
    if entry["returned"] is not None:  # a disabled call hands back the very object it was given
        assert result is args[entry["returned"]]
        return None
    assert f"out_{key}" in g.files
    if "replaced" in entry:  # pre-CFG: a new list, the other entry untouched
        conds = args["conds_out"]
        assert isinstance(result, list) and result is not conds and len(result) == len(conds)
        for i, (a, b) in enumerate(zip(result, conds)):
            assert (a is not b) if i == entry["replaced"] else (a is b)
        result = result[entry["replaced"]]
    assert isinstance(result, torch.Tensor) and result.is_cuda and result.dtype == dtype and tuple(result.shape) == lc.SHAPE
    assert result.data_ptr() not in {v.data_ptr() for v in tensors.values()}
    return result.cpu(), torch.from_numpy(g[f"out_{key}"])


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_reference_cases(pkg, name):
    g, meta = _golden()
    entry = meta["cases"][name]
    assert {k: entry[k] for k in ("node", "ops", "sigma", "has_uncond")} == lc.CASES[name]
    tensors = {k: torch.from_numpy(g[f"in_{k}"]).cuda() for k in ("x", "cond", "uncond", "denoised")}
    pair = _check_case(g, entry, name, tensors)
    if pair is not None:
        print(f"{name}: max |got - want| = {float((pair[0] - pair[1]).abs().max()):.3e}, peak {float(pair[1].abs().max()):.3e}")
        _close(*pair, name)


@pytest.mark.parametrize("name", sorted(lc.SEQUENCES))
def test_reference_sequences(pkg, name):
    """One node, its hook called several times: the mode the patch keeps from call to call, the gates and the window follow the reference."""
    g, meta = _golden()
    entry = meta["sequences"][name]
    assert {k: entry[k] for k in ("node", "ops", "calls")} == lc.SEQUENCES[name]
    tensors = {k: torch.from_numpy(g[f"in_{k}"]).cuda() for k in ("x", "cond", "uncond", "denoised")}
    before = {k: v.clone() for k, v in tensors.items()}
    calls = lc.run_sequence(_mappings(), entry, tensors)
    assert len(calls) == len(entry["results"])
    for i, ((result, args), want) in enumerate(zip(calls, entry["results"])):
        if want["returned"] is not None:
            assert result is args[want["returned"]], (name, i)
            continue
        if "replaced" in want:
            conds = args["conds_out"]
            assert isinstance(result, list) and result is not conds and len(result) == len(conds)
            assert [j for j, (a, b) in enumerate(zip(result, conds)) if a is not b] == [want["replaced"]], (name, i)
            result = result[want["replaced"]]
        assert isinstance(result, torch.Tensor) and result.dtype == torch.float32
        _close(result.cpu(), torch.from_numpy(g[f"out_{name}__{i}"]), f"{name} call {i}")
    assert all(torch.equal(v, before[k]) for k, v in tensors.items())


HALF_KERNEL_SHAPES = ("straddle_2x3x5x7", "unaligned_2x3x5x7", "tail_1x1x1x3", "inner_below_vector_5x3")


@pytest.mark.parametrize("tag", sorted(lc.HALF_DTYPES))
@pytest.mark.parametrize("shape_key", HALF_KERNEL_SHAPES)
def test_half_types_at_kernel_level(pkg, shape_key, tag):
    """float16 / bfloat16 through both kernels where their packing can go wrong: a per-sample sigma that changes inside a 4-element item, the
    n % 4 tail, the one-element route (a view 2 bytes past a 16-byte boundary).  prepare only widens, so it must agree with torch computing
    in fp32 on the same values to the fp32 bar; finish adds one rounding: one unit in the last place of the dtype."""
    hl = pkg.hip_lib
    dtype = lc.HALF_DTYPES[tag]
    shape, offset = SHAPES[shape_key]
    n = int(np.prod(shape))
    gen = torch.Generator().manual_seed(zlib.crc32(repr((shape_key, tag)).encode()))

    def half(scale=1.0):
        flat = (torch.randn(n + 1, generator=gen) * scale).to(dtype).cuda()
        t = flat[1:] if offset else flat[:n]
        assert t.data_ptr() % 16 == (2 if offset else 0)
        return t.view(shape)

    x, t1, t2 = half(), half(), half()
    sigma = (torch.rand(shape[0], generator=gen) * 9.0 + 0.5).cuda()
    before = [t.clone() for t in (x, t1, t2)]
    result, t2f = hl.cfg_op_prepare(x, t1, t2, sigma)
    want, want2 = _torch_prepare(x.float(), t1.float(), t2.float(), sigma)
    assert result.dtype == t2f.dtype == torch.float32
    _close(result, want, "result")
    _close(t2f, want2, "t2_out")
    for mode, w in ((None, 0.0), ("lerp", 0.3), ("inject", 0.6)):
        out = hl.cfg_op_finish(result, t2f, x, sigma, t1, mode, w)
        assert out.dtype == dtype and out.shape == t1.shape
        want_out = _torch_finish(result, t2f, x.float(), sigma, t1.float(), mode, w)
        err = float(((out.float() - want_out).abs() / _ulp(want_out, dtype)).max())
        print(f"{shape_key} {tag} {mode}: max error {err:.3f} ulp")
        assert err <= 1.0
    torch.cuda.synchronize()
    assert all(torch.equal(t, b) for t, b in zip((x, t1, t2), before)), "an input changed"


def _ulp(want, dtype):
    """Spacing of ``dtype`` at the magnitude of each (fp32) expected value."""
    info = torch.finfo(dtype)
    mant = {torch.float16: 10, torch.bfloat16: 7}[dtype]
    exp = torch.floor(torch.log2(want.abs().clamp(min=info.smallest_normal)))
    return torch.exp2(exp - mant)


@pytest.mark.parametrize("key", sorted(f"{n}__{t}" for n in lc.HALF_CASES for t in lc.HALF_DTYPES))
def test_half_precision_inputs(pkg, key):
    """float16 / bfloat16 predictions go to the kernels as they are; the arithmetic is fp32, so against the reference run in fp32 on the same
    rounded values the one final rounding is the only added error: one unit in the last place of the dtype at the output's magnitude."""
    g, meta = _golden()
    entry = meta["half"][key]
    dtype = lc.HALF_DTYPES[entry["dtype"]]
    tensors = {k: torch.from_numpy(g[f"in_{k}"]).to(dtype).cuda() for k in ("x", "cond", "uncond", "denoised")}
    got, want = _check_case(g, entry, key, tensors, dtype)
    err = (got.float() - want).abs() / _ulp(want, dtype)
    print(f"{key}: max error {float(err.max()):.3f} ulp")
    assert float(err.max()) <= 1.0


def test_result_is_the_patchs_own_buffer(pkg):
    """Without t2 and flip an operation may return its input as it is: what it was handed is the patch's copy, never the caller's tensor."""
    g, _ = _golden()
    tensors = {k: torch.from_numpy(g[f"in_{k}"]).cuda() for k in ("x", "cond", "uncond", "denoised")}
    seen = []

    def op(latent):
        seen.append(latent)
        return latent

    case = dict(node=lc.DEFAULTS | dict(mode="cond", blend_strength=1.0), ops=[], sigma=lc.PER_SAMPLE, has_uncond=True)
    cls = _mappings()["SonarApplyLatentOperationCFG"]
    (model,) = cls.go(model=lc.ModelPatcher(), operation_1=op, **case["node"])
    result, args = lc.run_patched(model, tensors, torch.tensor(case["sigma"], device="cuda"), True)
    own = {v.data_ptr() for v in tensors.values()}
    assert len(seen) == 1 and seen[0].dtype == torch.float32 and seen[0].data_ptr() not in own
    assert result[0].data_ptr() not in own | {seen[0].data_ptr()} and result[1] is tensors["uncond"]
    assert torch.equal(result[0], tensors["cond"]) and torch.equal(seen[0], tensors["cond"])
