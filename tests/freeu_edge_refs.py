"""The FreeU kernels (csrc/freeu.hip) at their plan, access, group and window edges: the fp64 statements of the two entry points, the derived
bounds and the case tables that tests/test_freeu_edges_cpu.py pins and tests/test_gpu_freeu_edges.py runs through the C ABI.

Statements
    hidden_mean_ref   sonar_freeu_hidden_mean: the mean over ALL channels and each sample's (min, max) of it.
    apply_abi_ref     sonar_freeu_apply's documented contract (include/sonar_hip.h, "sonar_freeu_apply"), given the fp32 ``mean`` /
                      ``extremes`` arrays the KERNEL is handed: they are inputs of the test, not the hidden-mean kernel's output, so the two
                      entry points are pinned independently of each other.

The fused kernel's call sites are the general-size plane kernel's (tests/power_any_sites.py) in the small codelet family -- the plan
``sonar_freeu_apply`` computes is ``sonar_power_any_plan(H, W, family=0)`` -- named "freeu" here because the kernel inlines every pass
separately, plus the access form a size gets when everything is aligned.  ``FREEU_SWEEP`` is a committed list of plane sizes that reaches
every such site over the whole kind-2 domain (tests/test_freeu_edges_cpu.py holds it to that); ``FREEU_FIXED`` are the twelve fixed planes
of ``sonar_power_plane_kind == 1``, which the plan query refuses and FreeU runs through the same kernel.

``python -m tests.freeu_edge_refs`` prints a fresh ``FREEU_SWEEP`` after a change to the plan rules or the codelet set.
"""
import itertools
import math

import numpy as np

from tests import freeu_refs as R
from tests import power_any_sites as S

U32 = 2.0 ** -24  # unit roundoff of fp32
PLAIN, FUSED, FILTERED = 0, 1, 2          # SONAR_FREEU_*
BLEND_NONE, LERP, INJECT, SUBTRACT_B = -1, 0, 1, 2   # SONAR_CFG_BLEND_NONE, SONAR_BLEND_*
DTYPE_ID = {"float32": 0, "float16": 1, "bfloat16": 2}  # SONAR_DTYPE_*
MEAN_SLICES = 8  # kMeanSlices: the waves of a hidden-mean workgroup, each a slice of the channels


# ---- statements ------------------------------------------------------------------------------------------------------------------------------
def hidden_mean_ref(x64):
    """(mean [B, HW], extremes [B, 2]) of x [B, C, HW] (or [B, C, H, W]) in fp64."""
    x = np.asarray(x64, dtype=np.float64)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    with np.errstate(invalid="ignore"):
        m = x.mean(axis=1)
        return m, np.stack([m.min(axis=1), m.max(axis=1)], axis=1)


def mean_bound(x, per_group, groups):
    """Forward-error bound of the hidden-mean kernels' summation tree, per position [B, HW]:

        (ceil(per_group / 8) + 7 + groups + 2) * 2^-24 * mean_c |x|.

    Derivation.  In a sum of fp32 values formed by any tree of additions, each rounded with relative error at most u = 2^-24, a term
    that passes through d additions carries a factor (1 + e)^d, so |fl(sum) - sum| <= ((1 + u)^d - 1) * sum |x_c| with d the deepest
    path.  The kernel's tree: a wave owns every eighth channel of its group, at most ceil(per_group / 8) of them, and adds them in one
    chain (the four-way unrolled trips add pairs first: shallower, never deeper) -- ceil(per_group / 8) additions, counting the one onto
    the zero accumulator; seven additions across the eight slices; at most ``groups`` additions of the groups' partial sums in the extremes
    kernel (groups - 1, rounded up); one rounding of the division by C.  The last unit covers the second-order terms:
    (1 + u)^d - 1 <= d u + (d u)^2 <= (d + 1) u for d <= 2^12.  Divided by C, sum |x_c| is mean_c |x|.  The inputs are exact: a 16-bit
    tensor is widened without rounding, and the reference is taken of the widened values."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    x = x.reshape(x.shape[0], x.shape[1], -1)
    return (math.ceil(per_group / MEAN_SLICES) + 7 + groups + 2) * U32 * x.mean(axis=1)


def f32(v):
    return float(np.float32(v))


def scalars_of(scale):
    """((float)scale, (float)(scale - 1.0)) as sonar_freeu_apply forms them: the difference in double, then one rounding."""
    return f32(scale), f32(float(scale) - 1.0)


def _scale_terms(B, HW, mean, extremes, scale):
    """(s, n, sm1): the scale per [B, 1, HW] position, the normalised mean (None for the scalar) and (float)(scale - 1)."""
    sc, sm1 = scalars_of(scale)
    if mean is None:
        return sc, None, sm1
    m = np.asarray(mean, dtype=np.float64).reshape(B, 1, HW)
    ex = np.asarray(extremes, dtype=np.float64).reshape(B, 2)
    lo, hi = ex[:, 0].reshape(B, 1, 1), ex[:, 1].reshape(B, 1, 1)
    n = (m - lo) / (hi - lo)
    return 1.0 + sm1 * n, n, sm1


def _filtered_values(a, H, W, mode, filt, filtered):
    if mode == PLAIN:
        return a
    if mode == FILTERED:
        return np.asarray(filtered, dtype=np.float64).reshape(a.shape)
    f = np.asarray(filt, dtype=np.float64).reshape(H, W // 2 + 1)
    return np.fft.irfft2(np.fft.rfft2(a, norm="ortho") * f, s=(H, W), norm="ortho")


def _blend(mode, a, v, t):
    if mode == BLEND_NONE:
        return v
    if mode == LERP:  # as sonar_blend_f32 (and torch.lerp): from the nearer end, so an infinite v gives what the kernel gives
        return a + t * (v - a) if abs(t) < 0.5 else v + (t - 1.0) * (v - a)
    if mode == INJECT:
        return v * t + a
    if mode == SUBTRACT_B:
        return a - v * t
    raise KeyError(mode)


def apply_abi_ref(x, c0, cn, mode, *, filt=None, filtered=None, mean=None, extremes=None, scale=1.0, blend_mode=BLEND_NONE, blend=1.0,
                  with_bound=False):
    """sonar_freeu_apply on x [B, C, H, W] in fp64: a new array, the channels c0 .. c0 + cn - 1 of every sample rewritten.

    mean [B, HW] / extremes [B, 2] are the fp32 arrays the kernel is given (None: the scalar scale); scale - 1 is taken in double and
    rounded to fp32, scale itself is rounded to fp32, ``blend`` is the fp32 value of the call.  0 / 0 and x / 0 are what IEEE makes of
    them (callers compare the NaN / inf pattern).

    with_bound: also the forward-error bound of the fp32 finishing arithmetic on an EXACT f, per element of the window -- the count of
    roundings of  s = 1 + sm1 * ((m - lo) / (hi - lo)),  v = f * s,  blend(x, v, t):
        the two subtractions and the division, each a relative u on n, and the multiplication by sm1: 4 u |sm1 n|; the addition: u |s|
        the multiplication: |f| e_s + u |v|
        the blend: the difference (u |v - x|), the product (u |t v|; the written multiply-add of lerp rounds once, the bound keeps both)
                   and the sum (u |out|), on top of e_v at a weight of at most max(|t|, |1 - t|, 1)."""
    x = np.array(x, dtype=np.float64)
    B, C, H, W = x.shape
    HW = H * W
    out = x.copy()
    bound = np.zeros_like(x)
    if B == 0 or cn == 0:
        return (out, bound) if with_bound else out
    a = x[:, c0:c0 + cn]
    t = float(blend)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        f = _filtered_values(a, H, W, mode, filt, filtered)
        s, n, sm1 = _scale_terms(B, HW, mean, extremes, scale)
        if n is not None:
            s, n = s.reshape(B, 1, H, W), n.reshape(B, 1, H, W)
        v = f * s
        res = _blend(blend_mode, a, v, t)
        out[:, c0:c0 + cn] = res
        if with_bound:
            e_s = U32 * (4.0 * np.abs(sm1 * n) + np.abs(s)) if n is not None else 0.0
            e_v = np.abs(f) * e_s + U32 * np.abs(v)
            if blend_mode == BLEND_NONE:
                e = e_v
            else:
                e = max(abs(t), abs(1.0 - t), 1.0) * e_v + U32 * (np.abs(v - a) + np.abs(t * v) + np.abs(res))
            bound[:, c0:c0 + cn] = e
    return (out, bound) if with_bound else out


# ---- the hidden mean's cases -----------------------------------------------------------------------------------------------------------------
# (B, C, HW) -> the channel groups sonar_freeu_hidden_mean_groups gives it (the CPU test asserts it: a change to the heuristic fails there
# instead of silently moving a case onto another path), the dtypes it runs in, what it is there for
ALL_DTYPES = R.DTYPES
MEAN_CASES = (
    ((2, 1, 64), 1, ALL_DTYPES, "seven waves without a channel"),
    ((2, 5, 64), 1, ALL_DTYPES, "three waves without a channel"),
    ((1, 8, 64), 1, ALL_DTYPES, "exactly one channel per wave"),
    ((1, 9, 70), 1, ALL_DTYPES, "one remainder trip more on wave 0; a tail chunk"),
    ((1, 32, 64), 1, ALL_DTYPES, "exactly one unrolled trip"),
    ((1, 33, 65), 1, ALL_DTYPES, "one unrolled trip and a remainder trip"),
    ((1, 40, 1), 1, ALL_DTYPES, "unrolled plus remainder on every wave; one position"),
    ((1, 63, 63), 1, ALL_DTYPES, "just under two unrolled trips"),
    ((1, 65, 16), 2, ALL_DTYPES, "two groups, 33 + 32"),
    ((1, 100, 100), 3, ALL_DTYPES, "three groups, 34 + 34 + 32"),
    ((1, 1290, 1030), 16, ("float16", "float32"), "the cap of 16 groups, 15 x 81 + 75; the extremes kernel's second trip"),
    ((3, 96, 70), 3, ALL_DTYPES, "groups with B > 1 and a tail chunk"),
)
WS_FORMS = ("helper", "null", "two", "one")  # the workspace the helper asks for; none; room for exactly two groups; room for one


def ws_room(form, want):
    """How many copies of the mean the workspace of a form has room for (0: no workspace)."""
    return {"helper": want if want > 1 else 0, "null": 0, "two": 2, "one": 1}[form]


def groups_run(C, want, room):
    """(groups, per_group) as sonar_freeu_hidden_mean lays the channels out, given the helper's answer and the workspace's room."""
    g = min(want, room)
    g = 1 if g < 2 else g
    per = -(-C // g)
    return -(-C // per), per


def mean_input(shape, seed):
    """freeu_refs.make_input for [B, C, HW] (offsets per sample for up to four samples)."""
    B, C, HW = shape
    return R.make_input((B, C, HW, 1), seed).reshape(B, C, HW)


# ---- the sweep kernel's cases: pairwise over the factors -------------------------------------------------------------------------------------
# layout: (H, W, pointer offset in elements, stride_c - HW) -> the access width in the comment
SWEEP_LAYOUTS = (
    (4, 4, 0, 0),   # HW = 16: four elements per access
    (2, 3, 0, 0),   # HW = 6: two
    (3, 5, 0, 0),   # HW = 15: one
    (4, 4, 1, 0),   # the pointer aligned to one element only: one
    (4, 4, 2, 0),   # to two elements: two
    (4, 4, 0, 2),   # aligned pointer, stride_c = HW + 2: two
    (4, 4, 0, 1),   # stride_c = HW + 1: one
)
SWEEP_C = 5
SWEEP_WINDOWS = ((0, SWEEP_C), (1, 2), (SWEEP_C - 1, 1))
SWEEP_FACTORS = (SWEEP_LAYOUTS, ALL_DTYPES, (PLAIN, FILTERED), ("map", "scalar"), (BLEND_NONE, LERP, INJECT, SUBTRACT_B), SWEEP_WINDOWS)


def pairwise(factors):
    """A short list of combinations in which every pair of values of two different factors occurs: greedily, always the combination of the
    full product that holds the most pairs not seen yet, the first of equals (deterministic)."""
    idx = [range(len(f)) for f in factors]
    need = {(i, a, j, b) for i, j in itertools.combinations(range(len(factors)), 2) for a in idx[i] for b in idx[j]}
    every = list(itertools.product(*idx))
    pairs_of = lambda combo: {(i, combo[i], j, combo[j]) for i, j in itertools.combinations(range(len(combo)), 2)}  # noqa: E731
    picked = []
    while need:
        best = max(every, key=lambda c: len(pairs_of(c) & need))
        picked.append(best)
        need -= pairs_of(best)
    return [tuple(f[k] for f, k in zip(factors, combo)) for combo in picked]


SWEEP_CASES = pairwise(SWEEP_FACTORS)


# ---- the fused kernel's sites ----------------------------------------------------------------------------------------------------------------
def freeu_plan(lib, H, W):
    """The plan sonar_freeu_apply computes for a kind-2 plane (any_plan_fill over kFreeuSet = the small codelet family)."""
    return S.plan(lib, H, W, family=0)


def freeu_sites(lib, H, W):
    p = freeu_plan(lib, H, W)
    sites = {("freeu",) + s[1:] for s in S.sites_of(p, H, W)}
    sites.add(("freeu", "access", 4 if W % 4 == 0 else 2))  # the access form when pointer and strides are aligned
    return frozenset(sites)


def domain_sites(lib):
    """{size: its sites} over every kind-2 plane, ascending by area."""
    return {hw: freeu_sites(lib, *hw) for hw in S.accepted_sizes(lib)}


# greedy_cover over the 34,706 kind-2 sizes (75 sites), (2, 2) first
FREEU_SWEEP = (
    (2, 2), (2, 6), (14, 28), (16, 30), (144, 4), (40, 32), (4, 412), (4, 618), (6, 548), (10, 328), (54, 60), (20, 200),
    (10, 410), (6, 822), (70, 72), (10, 574), (10, 656), (20, 328), (10, 738), (10, 820), (20, 410), (10, 902), (10, 984), (20, 492),
    (88, 112), (20, 574), (108, 128), (20, 738), (20, 820), (20, 902), (18, 1008), (100, 242), (182, 162), (132, 288),
)
# sonar_power_plane_kind == 1: the plan query refuses them, sonar_freeu_apply runs them through the same kernel
FREEU_FIXED = ((16, 16), (32, 32), (64, 32), (32, 64), (64, 64), (128, 64), (64, 128), (128, 128), (256, 64), (64, 256), (256, 128), (128, 256))

FUSED_WINDOW = (1, 2)  # of [2, 3, H, W]: four planes
FUSED_REF_KW = dict(scale=1.3, hidden_mean=True, blend=0.7, blend_mode="lerp", slice=0.7, slice_offset=0.4)  # int(2.1) = 2 from int(1.2) = 1
ACCESS_SIZES = ((14, 28), (2, 6), (16, 30), (4, 2))  # M even with W % 4 == 0; M odd; M odd; M = 1


def fused_inputs(hw, B=2, C=3):
    """(x [B, C, H, W] fp32, filter [H, W/2+1] fp32): make_input normals with per-sample offsets, and the filter of
    tests/test_gpu_power_any_sites._inputs -- rand + 0.5, no symmetry in ky, the kx = 0 and kx = W/2 columns scaled apart: every bin matters."""
    h, w = hw
    rng = np.random.default_rng(1000 * h + w)
    filt = (rng.random((h, w // 2 + 1)) + 0.5).astype(np.float32)
    filt[:, 0] *= np.float32(1.25)
    filt[:, -1] *= np.float32(0.75)
    return R.make_input((B, C, h, w), 7000 + 1000 * h + w), filt


def mean_arrays(x):
    """The fp32 (mean [B, HW], extremes [B, 2]) a test hands to sonar_freeu_apply: the fp64 mean rounded once, and ITS extremes."""
    m, _ = hidden_mean_ref(x)
    m = m.astype(np.float32)
    return m, np.stack([m.min(axis=1), m.max(axis=1)], axis=1)


if __name__ == "__main__":
    import sonar_pkg

    _lib = sonar_pkg.load().hip_lib.load()
    _by_size = domain_sites(_lib)
    _cover = S.greedy_cover(_by_size)
    print(f"# {len(_by_size)} sizes, {len(set().union(*_by_size.values()))} sites, {len(_cover)} sizes cover them, "
          f"largest {max(_cover, key=lambda s: s[0] * s[1])}")
    print("FREEU_SWEEP = (")
    for i in range(0, len(_cover), 12):
        print("    " + " ".join(f"({h}, {w})," for h, w in _cover[i:i + 12]))
    print(")")
