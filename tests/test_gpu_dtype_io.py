"""-m gpu: the shared element layer (csrc/dtype_io.h: widen, narrow, the 4-element and the one-element load / store) through two entry-point
families that exist already, against torch on the CPU (``.to(dtype)``), bit for bit.

  widen    all 65 536 patterns of float16 and of bfloat16 -> float32 through noise_params_tail (no fix, no normalisation, factor 1)
  narrow   float32 -> float16 / bfloat16 through the same call: for every finite 16-bit pattern the exact midpoint to its successor (a tie)
           and that midpoint's two float32 neighbours; +-0, float32 subnormals, the values around the largest finite float16, +-inf, NaNs
  cfg_op   cfg_op_prepare (widen) + cfg_op_finish (narrow) return every non-NaN 16-bit pattern unchanged

each on three routes: an aligned buffer of 4k elements (4-element accesses), 4k + 3 elements (plus the one-element tail) and a view that
starts one element into its buffer (one-element accesses).  The wrappers allocate their outputs, so the store side of the last route and
the guards go through the C entry points of the same launches: an output inside a NaN-filled buffer, the same bits expected, the NaN
guards on both sides untouched.  A bfloat16 NaN result is 0x7FC0; a float16 NaN result is a NaN (no suite pins its payload).

None of the family suites (test_gpu_noise_params.py, test_gpu_latent_op_cfg.py, test_gpu_freeu.py, test_gpu_elementwise.py) asserts any
of this exhaustively: they compare seeded tensors within one ulp of a float64 reference."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 64  # guard elements on either side of a prefilled output (128 bytes of a 16-bit type: the output stays 16-byte aligned)
ROUTES = ("vector", "tail", "scalar")
HALVES = [pytest.param(torch.float16, id="fp16"), pytest.param(torch.bfloat16, id="bf16")]
# (mantissa bits, smallest normal exponent, first non-finite pattern of the positive half)
FORMAT = {torch.float16: (10, -14, 0x7C00), torch.bfloat16: (7, -126, 0x7F80)}
NAN_BITS = (0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000, 0x7FC12345)  # quiet, the smallest signalling payload, all ones, signalling, mixed


@pytest.fixture(scope="module")
def api(pkg):
    lib = pkg.hip_lib.load()
    return types.SimpleNamespace(hl=pkg.hip_lib, lib=lib)


def bits16(t):
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bits32(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def all_patterns(dtype):
    """every 16-bit pattern as ``dtype`` (65 536 values, on the CPU)"""
    return torch.arange(-32768, 32768, dtype=torch.int16).view(dtype)


def is_tie(x, dtype):
    """float32 values exactly halfway between two neighbouring values of ``dtype`` (the format continued past its largest finite value)"""
    mant, emin, _ = FORMAT[dtype]
    a = np.abs(x.double().numpy())
    ok = np.isfinite(a) & (a > 0)
    a = np.where(ok, a, 1.0)
    _, e = np.frexp(a)
    half_ulp = np.ldexp(1.0, np.maximum(e - 1, emin) - mant - 1)
    q = a / half_ulp  # exact: a power of two divides
    return ok & (q == np.floor(q)) & (np.mod(q, 2.0) == 1.0)


@functools.lru_cache(maxsize=None)
def narrow_case(dtype):
    """(float32 inputs, their reference in ``dtype``) with the classes counted"""
    mant, _, first_inf = FORMAT[dtype]
    mags = torch.arange(first_inf, dtype=torch.int32).to(torch.int16).view(dtype).double()  # every finite magnitude, ascending
    succ = torch.cat((mags[1:], mags[-1:] + 2.0 ** (mags[-1].log2().floor() - mant)))       # ... and the value after it
    mid = ((mags + succ) / 2).float()
    assert torch.equal(mid.double() * 2, mags + succ), "a midpoint is not a float32"
    edge = torch.cat((mid, torch.nextafter(mid, torch.tensor(float("inf"))), torch.nextafter(mid, torch.tensor(0.0))))
    top = torch.tensor([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 99999.0, 3.4028234663852886e38])  # around float16's largest finite value
    tiny = torch.tensor([0x00000001, 0x00400000, 0x007FFFFF], dtype=torch.int32).view(torch.float32)   # float32 subnormals
    finite = torch.cat((edge, top, tiny, torch.tensor([0.0, float("inf")])))
    nans = torch.tensor(NAN_BITS, dtype=torch.int32).view(torch.float32)
    x = torch.cat((finite, -finite, nans, (bits32(nans) | -0x80000000).view(torch.float32)))
    want = x.to(dtype)
    # the classes the case is made for are all there: one tie per finite pattern, the overflows, the NaNs, both zeros, both infinities
    n_over = int((torch.isfinite(x) & torch.isinf(want.float())).sum())
    assert int(is_tie(x, dtype).sum()) == 2 * first_inf + (2 if dtype == torch.float16 else 0)  # (65520 is in `top` as well)
    # float16: the top midpoint 65520 (a tie to even = infinity), its upper neighbour, and 65520, 65520.004, 65536, 99999, float32's largest of `top`;
    # bfloat16: the top midpoint 0x7F7F8000 and its upper neighbour, and float32's largest value (0x7F7FFFFF, above that midpoint)
    assert n_over == 2 * (7 if dtype == torch.float16 else 3), n_over
    assert int(torch.isnan(x).sum()) == 2 * len(NAN_BITS) == int(torch.isnan(want).sum())
    assert int((bits32(x) == 0).sum()) == 1 and int((bits32(x) == -0x80000000).sum()) == 1 and int(torch.isinf(x).sum()) == 2
    assert int(((x != 0) & (x.abs() < 2.0 ** -126)).sum()) >= 2 * 3
    return x, want


def on_route(src, route):
    """``src`` (CPU, 1-D) on the device for one route -> (device tensor, the CPU values it holds)"""
    n = src.numel() // 4 * 4
    if route == "vector":
        cpu = src[:n] if n == src.numel() else torch.cat((src, src[: n + 4 - src.numel()]))
        dev = cpu.cuda()
    elif route == "tail":
        cpu = torch.cat((src, src[: (3 - src.numel()) % 4]))
        dev = cpu.cuda()
        assert cpu.numel() % 4 == 3
    else:
        cpu = src
        dev = torch.cat((src[:1], src)).cuda()[1:]
        assert dev.is_contiguous() and dev.data_ptr() % 16 != 0
    assert cpu.numel() >= src.numel() and (route == "scalar" or dev.data_ptr() % 16 == 0)
    return dev, cpu


def guarded(n, dtype, route):
    """(whole, view): ``n`` elements inside a NaN-filled buffer, PAD guards before and after; one element off alignment on the scalar route"""
    off = 1 if route == "scalar" else 0
    whole = torch.full((n + 2 * PAD + 1,), float("nan"), dtype=dtype, device="cuda")
    return whole, whole[PAD + off:PAD + off + n]


def guards_intact(whole, view):
    start = view.storage_offset()
    return bool(torch.isnan(whole[:start]).all()) and bool(torch.isnan(whole[start + view.numel():]).all())


def tail(api, src, out_dtype, route):
    """noise_params_tail as a pure conversion; the same launch once more into a guarded output, through sonar_noise_params_apply"""
    hl, n = api.hl, src.numel()
    got = hl.noise_params_tail(src, (n,), out_dtype, 1, n, n, fix_invalid=False, normalized=False, factor=1.0)
    whole, out = guarded(n, out_dtype, route)
    hl._check(api.lib.sonar_noise_params_apply(hl.DTYPE_IDS[src.dtype], src.data_ptr(), hl.DTYPE_IDS[out_dtype], out.data_ptr(), 1, n, n, 0, 0, 1.0, 2.5,
                                               None, hl._stream()), "sonar_noise_params_apply")
    torch.cuda.synchronize()
    assert guards_intact(whole, out), "wrote outside its output"
    return got.cpu(), out.cpu()


def same_bits(got, want, what):
    """non-NaN: the reference's bits; NaN exactly where the reference has one"""
    bits = bits32 if want.dtype == torch.float32 else bits16
    nan = torch.isnan(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaNs in other places than the reference's"
    bad = (bits(got) != bits(want)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values differ, first at {int(bad.nonzero()[0])}"
    if want.dtype == torch.bfloat16:
        assert bool((bits16(got)[nan] == 0x7FC0).all()), f"{what}: a bfloat16 NaN that is not 0x7FC0"


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", HALVES)
def test_widen_every_pattern(api, dtype, route):
    src, cpu = on_route(all_patterns(dtype), route)
    want = cpu.float()
    assert int(torch.isnan(want).sum()) >= 2 * (0x8000 - FORMAT[dtype][2] - 1)
    for got in tail(api, src, torch.float32, route):
        same_bits(got, want, f"widen {dtype} {route}")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", HALVES)
def test_narrow_at_its_edges(api, dtype, route):
    x, _ = narrow_case(dtype)
    src, cpu = on_route(x, route)
    want = cpu.to(dtype)
    for got in tail(api, src, dtype, route):
        same_bits(got, want, f"narrow {dtype} {route}")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", HALVES)
def test_cfg_op_round_trip(api, dtype, route):
    """prepare without flip or t2 is the widening, finish without t2, flip or blend the narrowing: t1 comes back"""
    hl = api.hl
    t1, cpu = on_route(all_patterns(dtype), route)
    result, none = hl.cfg_op_prepare(None, t1, None, None)
    assert none is None and result.dtype == torch.float32
    same_bits(result.cpu(), cpu.float(), f"cfg_op_prepare {dtype} {route}")
    got = hl.cfg_op_finish(result, None, None, None, t1, None, 0.0)
    n = t1.numel()
    whole, out = guarded(n, dtype, route)
    hl._check(api.lib.sonar_cfg_op_finish(hl.DTYPE_IDS[dtype], result.data_ptr(), None, None, None, 0, None, hl.CFG_BLEND_NONE, 0.0, out.data_ptr(), n, n,
                                          hl._stream()), "sonar_cfg_op_finish")
    whole_r, res = guarded(n, torch.float32, route)
    hl._check(api.lib.sonar_cfg_op_prepare(hl.DTYPE_IDS[dtype], None, t1.data_ptr(), None, None, 0, res.data_ptr(), None, n, n, hl._stream()),
              "sonar_cfg_op_prepare")
    torch.cuda.synchronize()
    assert guards_intact(whole, out) and guards_intact(whole_r, res), "wrote outside its output"
    assert torch.equal(bits32(res.cpu()), bits32(result.cpu()))
    for back in (got.cpu(), out.cpu()):
        nan = torch.isnan(cpu)
        assert back.dtype == dtype and torch.equal(torch.isnan(back), nan)
        assert torch.equal(bits16(back)[~nan], bits16(cpu)[~nan]), f"cfg_op round trip {dtype} {route}"
