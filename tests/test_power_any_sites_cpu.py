"""CPU: the plan of the general-size power-noise kernels (sonar_power_any_plan, no GPU work) over every plane size they accept --
tests/power_any_sites.SWEEP reaches every call site there is, the SDXL buckets' compile-time factor pairs are the ones best_split picks,
and the query refuses what sonar_power_plane_kind refuses."""
import os
import re

import pytest

from tests import power_any_sites as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.hip_lib.load()


@pytest.fixture(scope="module")
def by_size(lib):
    return S.domain_sites(lib)


def header_buckets():
    """[(H, W, hn1, hn2, mn1, mn2)] as csrc/power_buckets.h writes them."""
    text = open(os.path.join(ROOT, "comfyui-sonar_amd", "csrc", "power_buckets.h")).read()
    rows = []
    for name in ("SONAR_BUCKETS_A", "SONAR_BUCKETS_B"):
        line = re.search(rf"#define {name}\(X\)(.*)", text).group(1)
        rows += [tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", line)]
    return rows


def test_sweep_reaches_every_site_of_the_accepted_domain(by_size):
    """Coverage is a condition: every site that any accepted size runs is run by a size of SWEEP, none waived.  A change to best_split,
    to a codelet set or to the fold rule that creates a site fails here until SWEEP is regenerated (python -m tests.power_any_sites)."""
    assert len(by_size) == 34706  # even H <= 512, even W <= 1024 within the LDS limit, less the twelve fixed-size planes
    assert len(set(S.SWEEP)) == len(S.SWEEP) and all(hw in by_size for hw in S.SWEEP)
    every = set().union(*by_size.values())
    reached = set().union(*(by_size[hw] for hw in S.SWEEP))
    assert not every - reached, f"sites no size of SWEEP runs: {sorted(map(str, every - reached))}"
    assert (2, 2) in S.SWEEP
    # what was untested before: every codelet of both run-time families at its call sites (an even line of 3 x n2 points with
    # n2 <= 3 is one codelet of 6, so no column first pass of 3), the direct-sum passes, lines of one value, both workgroup sizes
    for fam, lengths in (("small", range(2, 13)), ("all", [*range(2, 17), 17, 19])):
        for n in lengths:
            assert (fam, "cols", 0, n) in reached or n == 3
            assert {(fam, "cols", 1, n), (fam, "rows", 1, n)} <= reached or n > 16
            assert {(fam, "rows", 0, n, "fold", 1), (fam, "rows", 0, n, "pre", 0)} <= reached
        for ax in ("cols", "rows"):
            assert {(fam, ax, 1, "direct"), (fam, ax, 1, "absent")} <= reached
        assert {(fam, "cols", 0, "direct"), (fam, "rows", 0, "direct", "pre", 0), (fam, "rows", 0, "direct1", "pre", 0), (fam, "threads", 512),
                (fam, "threads", 1024)} <= reached
    assert {s[5] for s in reached if len(s) == 6 and s[4] == "fold"} == {1, 2}  # c2r_pass0 in one and in two row batches


def test_buckets_hold_the_pairs_best_split_picks(lib):
    """power_buckets.h: 'checked against best_split at run time' -- the launch only compares the products, so here: each bucket size is
    routed to its bucket kernel with the header's pairs, and they are what best_split gives the size over every codelet length."""
    rows = header_buckets()
    assert len(rows) == 8 and len({r[:2] for r in rows}) == 8
    for H, W, *pairs in rows:
        p = S.plan(lib, H, W)
        assert p["family"] == 2, (H, W)
        assert [p["hn1"], p["hn2"], p["mn1"], p["mn2"]] == pairs, (H, W)
        q = S.plan(lib, H, W, family=1)
        assert q["family"] == 1 and [q["hn1"], q["hn2"], q["mn1"], q["mn2"]] == pairs, (H, W, q)
        assert [p["run_hn1"], p["run_hn2"], p["run_mn1"], p["run_mn2"]] == [1, 1, 1, 1]
        assert (H, W) in S.SWEEP
    assert sum(S.plan(lib, *hw)["family"] == 2 for hw in S.accepted_sizes(lib)) == 8


def test_forced_families_and_plan_fields(lib, by_size):
    for (H, W) in S.SWEEP:
        p = S.plan(lib, H, W)
        assert p["hn1"] * p["hn2"] == H and p["mn1"] * p["mn2"] == W // 2
        assert p["threads"] in (512, 1024) and (p["fold_batches"] in (1, 2)) == bool(p["c2r_fuse"])
        if p["family"] < 2:
            assert S.plan(lib, H, W, family=p["family"]) == p  # forcing the routed family changes nothing
    # 46 = 2 x 23: no codelet of 23 points in either set -- a codelet first pass, a direct second one; with every length 26 = 13 x 2
    assert (lambda p: (p["family"], p["hn1"], p["hn2"], p["run_hn1"], p["run_hn2"]))(S.plan(lib, 46, 8)) == (0, 2, 23, 1, 0)
    assert (lambda p: (p["family"], p["hn1"], p["hn2"], p["run_hn2"]))(S.plan(lib, 26, 8)) == (1, 13, 2, 1)
    assert (lambda p: (p["family"], p["hn1"], p["hn2"], p["run_hn2"]))(S.plan(lib, 26, 8, family=0)) == (0, 2, 13, 0)


@pytest.mark.parametrize("hw", [(95, 160), (96, 161), (514, 8), (8, 1026), (0, 8), (8, 0), (200, 200), (512, 1024), (256, 256)])
def test_sizes_outside_the_domain_are_refused(lib, hw):
    """Odd H, odd W, H = 514, W = 1026, nothing, and half-spectra over the LDS limit: not kind 2, and the query says so."""
    import ctypes as C

    assert lib.sonar_power_plane_kind(*hw) != 2
    for family in (-1, 0, 1):
        out = (C.c_int32 * 12)(*([-7] * 12))
        assert lib.sonar_power_any_plan(*hw, family, out) == -2
        assert list(out) == [-7] * 12


def test_the_query_refuses_what_it_cannot_answer(lib):
    import ctypes as C

    out = (C.c_int32 * 12)()
    assert lib.sonar_power_any_plan(128, 128, -1, out) == -2  # a fixed-size plane (kind 1)
    assert lib.sonar_power_any_plan(96, 96, 2, out) != 0 and lib.sonar_power_any_plan(96, 96, -2, out) != 0
    assert lib.sonar_power_any_plan(96, 96, -1, None) != 0
    assert lib.sonar_power_any_plan(96, 96, -1, out) == 0
    # the last accepted sizes along each edge of the domain
    assert S.plan(lib, 512, 2) and S.plan(lib, 2, 1024) and S.plan(lib, 36, 1024) and not S.plan(lib, 38, 1024)
