"""CPU: what tests/test_gpu_freeu_edges.py stands on, through the library's host queries only -- FREEU_SWEEP reaches every call site the
fused FreeU kernel has over the kind-2 domain, the hidden-mean cases sit on the channel-group counts they name, and the fp64 statements of
tests/freeu_edge_refs.py agree with tests/freeu_refs.apply_ref and the reference's recorded outputs."""
import itertools
import os

import numpy as np
import pytest

from tests import freeu_edge_refs as F
from tests import freeu_refs as R
from tests import power_any_sites as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLEND_ID = {None: F.BLEND_NONE, "lerp": F.LERP, "inject": F.INJECT, "subtract_b": F.SUBTRACT_B}


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load()


@pytest.fixture(scope="module")
def by_size(lib):
    return F.domain_sites(lib)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "freeu_extreme.npz"), allow_pickle=False))


def test_sweep_reaches_every_site_of_the_freeu_domain(lib, by_size):
    """Coverage is a condition: every site any kind-2 size has under the small codelet family is run by a size of FREEU_SWEEP, none
    waived.  A change to best_split, to the codelet set or to the fold rule that creates a site fails here until FREEU_SWEEP is
    regenerated (python -m tests.freeu_edge_refs)."""
    assert len(by_size) == 34706
    assert len(set(F.FREEU_SWEEP)) == len(F.FREEU_SWEEP) and all(hw in by_size for hw in F.FREEU_SWEEP)
    assert all(lib.sonar_power_plane_kind(*hw) == 2 and F.freeu_plan(lib, *hw) is not None for hw in F.FREEU_SWEEP)  # every size is accepted
    every = set().union(*by_size.values())
    reached = set().union(*(by_size[hw] for hw in F.FREEU_SWEEP))
    assert not every - reached, f"sites no size of FREEU_SWEEP runs: {sorted(map(str, every - reached))}"
    assert F.FREEU_SWEEP[0] == (2, 2) and all(s[0] == "freeu" for s in every)
    # by name: both workgroup sizes, both access forms, the folded first pass in one and in two row batches, the direct sums, lines of
    # one value, absent second passes, and every codelet length at every axis and pass (an even line of 3 x n2 points with n2 <= 3 is
    # one codelet of 6: no column first pass of 3; a folded 12-point first pass never needs a second batch within the LDS limit)
    assert {("freeu", "threads", 512), ("freeu", "threads", 1024), ("freeu", "access", 4), ("freeu", "access", 2)} <= reached
    assert {s[5] for s in reached if len(s) == 6 and s[4] == "fold"} == {1, 2}
    assert {("freeu", "cols", 0, "direct"), ("freeu", "rows", 0, "direct", "pre", 0), ("freeu", "rows", 0, "direct1", "pre", 0)} <= reached
    for ax in ("cols", "rows"):
        assert {("freeu", ax, 1, "direct"), ("freeu", ax, 1, "absent")} <= reached
    for n in range(2, 13):
        assert ("freeu", "cols", 0, n) in reached or n == 3
        assert {("freeu", "cols", 1, n), ("freeu", "rows", 1, n), ("freeu", "rows", 0, n, "pre", 0), ("freeu", "rows", 0, n, "fold", 1)} <= reached
        assert ("freeu", "rows", 0, n, "fold", 2) in reached or n == 12
    assert ("freeu", "cols", 0, 3) not in every and ("freeu", "rows", 0, 12, "fold", 2) not in every
    # the issue's example: 104 x 152 has M = 76 = 4 x 19 as a codelet and direct sums in the small family; power noise routes it elsewhere
    p = F.freeu_plan(lib, 104, 152)
    assert (p["mn1"], p["mn2"], p["run_mn1"], p["run_mn2"]) == (4, 19, 1, 0) and S.plan(lib, 104, 152)["family"] != 0
    # lines of one value, and the sizes the access forms are run at
    assert F.freeu_plan(lib, 2, 2)["mn1"] == 1 and all(lib.sonar_power_plane_kind(*hw) == 2 for hw in F.ACCESS_SIZES)
    assert [hw[1] % 4 == 0 for hw in F.ACCESS_SIZES] == [True, False, False, False] and [(hw[1] // 2) % 2 for hw in F.ACCESS_SIZES] == [0, 1, 1, 1]


def test_fixed_planes_are_the_twelve_the_query_refuses(lib):
    assert len(set(F.FREEU_FIXED)) == 12
    for hw in F.FREEU_FIXED:
        assert lib.sonar_power_plane_kind(*hw) == 1 and F.freeu_plan(lib, *hw) is None
    assert sum(lib.sonar_power_plane_kind(h, w) == 1 for h in range(2, 513, 2) for w in range(2, 1025, 2)) == 12


def test_recorded_reference_errors_cover_the_fused_sizes(g):
    """tests/golden/freeu_edges.npz (make_freeu_edges_golden.py): one E_size per size the fused test runs, each a few fp32 roundings of
    the output's range like E itself -- the reference's fp32 FFT does not lose more at 18 x 1008 than at 8 x 8."""
    e = np.load(os.path.join(ROOT, "tests", "golden", "freeu_edges.npz"), allow_pickle=False)
    assert sorted(e.files) == ["e_size", "sizes"] and e["e_size"].dtype == np.float64
    assert [tuple(int(v) for v in s) for s in e["sizes"]] == list(F.FREEU_SWEEP + F.FREEU_FIXED)
    assert ((e["e_size"] > 0) & (e["e_size"] < 2.0 ** -20)).all()
    assert e["e_size"].max() < 2 * R.reference_error(g)


def test_hidden_mean_cases_sit_on_their_group_counts(lib):
    groups = lib.sonar_freeu_hidden_mean_groups
    for (B, C, HW), want, _dtypes, what in F.MEAN_CASES:
        assert groups(B, C, HW) == want, (B, C, HW, what)
    # the layouts the table names, as the entry point lays the channels out
    assert F.groups_run(65, 2, 2) == (2, 33) and F.groups_run(100, 3, 3) == (3, 34) and F.groups_run(1290, 16, 16) == (16, 81)
    assert 1290 - 15 * 81 == 75 and F.groups_run(1290, 16, 2) == (2, 645) and F.groups_run(96, 3, 3) == (3, 32) and F.groups_run(96, 3, 1) == (1, 96)
    assert any(g > 2 for _s, g, _d, _w in F.MEAN_CASES)  # the two-group workspace is smaller than what the helper wants somewhere
    # the helper's corners
    assert [groups(1, c, 64) for c in (1, 31, 32, 63, 64, 95, 96)] == [1, 1, 1, 1, 2, 2, 3]          # C < 32 -> 1; C // 32 is the limit
    assert [groups(1, c, 64) for c in (16 * 32 - 1, 16 * 32, 17 * 32, 4096)] == [15, 16, 16, 16]      # the cap of 16
    assert [groups(b, 4096, 64) for b in (511, 512, 513)] == [2, 1, 1]                               # B * ceil(HW / 64) >= 512 -> 1
    assert [groups(1, 4096, hw) for hw in (64 * 511, 64 * 511 + 1, 64 * 512)] == [2, 1, 1]
    assert [groups(4, 4096, hw) for hw in (64 * 127, 64 * 127 + 1)] == [2, 1]                        # a tail chunk counts as a chunk
    assert [groups(1, 4096, hw) for hw in (64 * 32, 64 * 32 + 1, 64 * 33)] == [16, 16, 16] and groups(1, 4096, 64 * 34) == 16
    assert groups(1, 4096, 64 * 35) == 15
    for bad in ((0, 64, 64), (-1, 64, 64), (1, 0, 64), (1, -5, 64), (1, 64, 0), (1, 64, -64)):
        assert groups(*bad) == 1


def test_the_no_empty_group_recomputation_is_out_of_reach():
    """sonar_freeu_hidden_mean recomputes groups = ceil(C / per_group) after per_group = ceil(C / groups).  With the helper's limit
    groups <= C // 32 and its cap of 16 (a smaller workspace only lowers the count), that never changes the count: it would need
    C <= g (g - 1) with C >= 32 g.  Held over every C <= 4096 and every count the helper or a workspace can give."""
    for C in range(1, 4097):
        for g in range(1, min(16, max(1, C // 32)) + 1):
            per = -(-C // g)
            assert -(-C // per) == g, (C, g)


def test_sweep_cases_hold_every_pair():
    cases = F.SWEEP_CASES
    assert len(cases) == len(set(cases)) and len(cases) < 40
    for i, j in itertools.combinations(range(len(F.SWEEP_FACTORS)), 2):
        assert {(c[i], c[j]) for c in cases} == set(itertools.product(F.SWEEP_FACTORS[i], F.SWEEP_FACTORS[j])), (i, j)
    assert [h * w for h, w, _o, _s in F.SWEEP_LAYOUTS[:3]] == [16, 6, 15]


def _abi_from_config(x, filt, kw, mean64=None):
    """apply_abi_ref fed what FreeUExtremeConfig.apply would hand the entry point, with the fp64 mean in place of the kernel's."""
    B, C, H, W = x.shape
    sl = R.slice_of(C, kw.get("slice", 1.0), kw.get("slice_offset", 0.0))
    c0, c1, _ = sl.indices(C)
    blend = kw.get("blend", 1.0)
    mean = ext = None
    if kw.get("hidden_mean", True):
        mean, ext = F.hidden_mean_ref(x) if mean64 is None else mean64
    return F.apply_abi_ref(x, c0, max(0, c1 - c0), F.PLAIN if filt is None else F.FUSED, filt=filt, mean=mean, extremes=ext, scale=kw.get("scale", 1.0),
                           blend_mode=F.BLEND_NONE if blend == 1.0 else BLEND_ID[kw["blend_mode"]], blend=blend)


def test_statements_agree_with_apply_ref_and_the_golden(g):
    """apply_abi_ref with the fp64 mean is freeu_refs.apply_ref to 1e-12 of the range at all nine golden cases -- apply_ref is given the
    scale whose fp64 (scale - 1), or whose value for the scalar, is exactly the fp32 number the entry point forms -- and, with the
    configured scale, within the reference's own E of the recorded fp32 outputs."""
    E = R.reference_error(g)
    for tag, (shape, kw, fname) in R.CASES.items():
        x = np.asarray(g[f"{tag}_x"], dtype=np.float64)
        filt = g[f"{tag}_filter"] if fname else None
        sc, sm1 = F.scalars_of(kw["scale"])
        exact = dict(kw, scale=1.0 + sm1 if kw.get("hidden_mean", True) else sc)
        assert (exact["scale"] - 1.0 == sm1) if kw.get("hidden_mean", True) else True
        got = _abi_from_config(x, filt, kw)
        want = R.apply_ref(x, filt, **exact)
        assert got.shape == tuple(shape) and np.abs(got - want).max() <= 1e-12 * R.spread(want), tag
        assert R.distance(np.asarray(g[f"{tag}_out_float32"]), got) <= E + 2.0 ** -23, tag  # E, and the fp32 rounding of the two scalars
        assert abs(R.distance(got, R.apply_ref(x, filt, **kw))) <= 2.0 ** -23, tag
    m, ext = F.hidden_mean_ref(g["a_x"])
    assert np.array_equal(m.reshape(2, 1, 8, 8), np.asarray(g["a_x"], dtype=np.float64).mean(1, keepdims=True)) and ext.shape == (2, 2)
    assert np.array_equal(ext[:, 0], m.min(1)) and np.array_equal(ext[:, 1], m.max(1))


def test_statement_modes_windows_and_bound():
    x = R.make_input((2, 5, 4, 6), 11).astype(np.float64)
    filtered = np.random.default_rng(3).standard_normal((2, 2, 4, 6))
    mean, ext = F.mean_arrays(x)
    out, bound = F.apply_abi_ref(x, 1, 2, F.FILTERED, filtered=filtered, mean=mean, extremes=ext, scale=1.3, blend_mode=F.INJECT, blend=F.f32(0.7),
                                 with_bound=True)
    keep = [0, 3, 4]
    assert np.array_equal(out[:, keep], x[:, keep]) and (bound[:, keep] == 0).all() and (bound[:, 1:3] > 0).all()
    e64 = ext.astype(np.float64)
    n = (mean.astype(np.float64) - e64[:, :1]) / (e64[:, 1:] - e64[:, :1])
    want = filtered * (1.0 + F.scalars_of(1.3)[1] * n).reshape(2, 1, 4, 6) * F.f32(0.7) + x[:, 1:3]
    assert np.abs(out[:, 1:3] - want).max() < 1e-14
    assert bound.max() < 16 * F.U32 * np.abs(out).max()  # a handful of roundings, no more
    assert np.array_equal(F.apply_abi_ref(x, 2, 0, F.PLAIN, scale=2.0), x)
    plain = F.apply_abi_ref(x, 4, 1, F.PLAIN, scale=0.9)
    assert np.array_equal(plain[:, :4], x[:, :4]) and np.array_equal(plain[:, 4], x[:, 4] * F.f32(0.9))
    # lerp from the nearer end, like the kernel: the same number either way where everything is finite
    for t in (0.25, 0.7):
        lerp = F.apply_abi_ref(x, 0, 5, F.PLAIN, scale=1.5, blend_mode=F.LERP, blend=t)
        assert np.abs(lerp - (x + t * (x * 1.5 - x))).max() < 1e-14
    # hi == lo: 0 / 0 and x / 0 go through as IEEE has them
    flat = np.stack([ext[:, 0], ext[:, 0]], axis=1)
    with np.errstate(all="ignore"):
        bad = F.apply_abi_ref(x, 0, 5, F.PLAIN, mean=mean, extremes=flat, scale=1.3)
    assert np.isnan(bad).sum() == 2 * 5 and np.isinf(bad).sum() == bad.size - 10


def test_mean_bound_is_the_stated_count():
    x = F.mean_input((1, 100, 100), 5)
    b = F.mean_bound(x, 34, 3)
    assert b.shape == (1, 100) and np.allclose(b, (5 + 7 + 3 + 2) * 2.0 ** -24 * np.abs(x).astype(np.float64).mean(1), rtol=1e-15)
    assert np.allclose(F.mean_bound(x, 100, 1), (13 + 7 + 1 + 2) * 2.0 ** -24 * np.abs(x).astype(np.float64).mean(1), rtol=1e-15)
    # an fp32 sum in the kernel's order stays inside it
    for per, groups in ((34, 3), (100, 1)):
        parts = []
        for cb in range(0, 100, per):
            ce = min(100, cb + per)
            waves = []
            for w in range(F.MEAN_SLICES):
                acc = np.zeros(100, dtype=np.float32)
                for c in range(cb + w, ce, F.MEAN_SLICES):
                    acc = acc + x[0, c]
                waves.append(acc)
            s = waves[0]
            for k in range(1, F.MEAN_SLICES):
                s = s + waves[k]
            parts.append(s)
        tot = parts[0]
        for part in parts[1:]:
            tot = tot + part
        m = tot / np.float32(100)
        assert m.dtype == np.float32
        assert (np.abs(m.astype(np.float64) - F.hidden_mean_ref(x)[0][0]) <= F.mean_bound(x, per, groups)[0]).all()
