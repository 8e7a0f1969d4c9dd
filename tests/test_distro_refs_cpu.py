"""CPU: tests/distro_refs.py, the fp64 statement of Distro noise's rejection-sampled families, is right -- one-sample tests of its values
against the exact laws (scipy.stats) over the grid that tests/test_gpu_distro_streams.py holds the kernel to, its fp32 evaluation against
its fp64 one, the cap on the share of elements it calls ambiguous, and controls that show the comparison failing on a wrong block allotment."""
import importlib
import math
from collections import namedtuple

import numpy as np
import pytest
import torch
from scipy import stats

from tests import distro_refs as R

SEED, STREAM = (0x5EED << 32) | 20260101, 3  # a seed with a non-zero high word
N_LAW = 1 << 18
ALPHA = 1e-4  # as tests/test_gpu_distro.py's KS_BOUND
KS_ONE = math.sqrt(-math.log(ALPHA / 2) / (2 * N_LAW))
KS_TWO = math.sqrt(-math.log(ALPHA / 2) / 2) * math.sqrt(2 / N_LAW)
AMBIGUOUS_CAP = 1e-3
f32 = np.float32

# name, family, kernel parameters (hip_lib.distro_fill's keywords), law: values -> (values, frozen scipy law[, lower clamp, upper clamp])
Case = namedtuple("Case", "name family params law")


def _p(family, **kw):
    return dict(family=R.CODES[family], **kw)


def _r(x):
    return float(f32(x))  # the parameter the kernel receives


DIRICHLET_3 = (0.3, 0.5, 2.0)
DIRICHLET_16 = (0.1, 2.0, 0.3, 1.0, 0.7, 5.0, 1.5, 0.2, 3.0, 0.5, 4.0, 0.15, 2.5, 0.9, 1.2, 5.0)  # mixed, 0.1 to 5; rows 0 and 15 the extremes


def vonmises_params(loc, kappa):
    return _p("vonmises", a=loc, b=kappa, c=R.vonmises_rm1(kappa))


def _unwrap(loc):
    return lambda x: (np.mod(x - _r(loc) + np.pi, 2 * np.pi) - np.pi)


def scalar_cases():
    """Every case of the grid but the matrix families'."""
    out = []
    for al in (0.05, 0.4, 0.999, 1.0, 1.001, 3.0, 1e3):
        out.append(Case(f"gamma-{al:g}", "gamma", _p("gamma", a=al, b=2.0), lambda x, al=al: (x, stats.gamma(_r(al), scale=0.5), R.FLT_MIN / 2.0, None)))
        out.append(Case(f"inverse_gamma-{al:g}", "inverse_gamma", _p("inverse_gamma", a=al, b=0.5),
                        lambda x, al=al: (x, stats.invgamma(_r(al), scale=0.5), None, 0.5 / R.FLT_MIN)))
    for a, b in ((0.5, 2.0), (30.0, 0.3)):
        out.append(Case(f"beta-{a:g}-{b:g}", "beta", _p("beta", a=a, b=b), lambda x, a=a, b=b: (x, stats.beta(_r(a), _r(b)))))
    for a, b in ((3.5, 5.0), (0.8, 200.0)):
        out.append(Case(f"fisher_snedecor-{a:g}-{b:g}", "fisher_snedecor", _p("fisher_snedecor", a=a, b=b),
                        lambda x, a=a, b=b: (x, stats.f(_r(a), _r(b)))))
    for df in (0.5, 2.7, 100.0):
        out.append(Case(f"studentt-{df:g}", "studentt", _p("studentt", a=0.5, b=2.0, c=df), lambda x, df=df: (x, stats.t(_r(df), loc=0.5, scale=2.0))))
    for conc, rows in ((DIRICHLET_3, (0, 1, 2)), (DIRICHLET_16, (0, 15))):
        total = sum(_r(c) for c in conc)
        for row in rows:
            out.append(Case(f"dirichlet-{len(conc)}-row{row}", "dirichlet", _p("dirichlet", k=len(conc), row=row, v=list(conc)),
                            lambda x, a=_r(conc[row]), t=total: (x, stats.beta(a, t - a))))
    for rate in (0.3, 9.99, 10.0, 10.01, 30.0, 1e3, 1e4, 1e5, 1e6):
        out.append(Case(f"poisson-{rate:g}", "poisson", _p("poisson", a=rate), lambda x, rate=rate: (x, stats.poisson(_r(rate)))))
    for kappa, loc in ((1e-6, 0.0), (1.0, -2.0), (4.0, 3.1), (100.0, 0.0), (1e3, -2.0), (1e4, 3.1), (1e5, 0.0), (1e6, -2.0)):
        out.append(Case(f"vonmises-{kappa:g}", "vonmises", vonmises_params(loc, kappa),
                        lambda x, kappa=kappa, loc=loc: (_unwrap(loc)(x), stats.vonmises(_r(kappa)))))
    return out


# The wide-range cases, and the one case of the element-exact grid whose ambiguous share exceeds AMBIGUOUS_CAP: alpha = 1e3, 3.8e-3 of the
# elements (measured from the statement alone; the guard grows with d in Marsaglia-Tsang's d - d v + d log v).  They are compared without
# the cap and, on the device, tested against the exact law as well.
WIDE = ("vonmises-10000", "vonmises-100000", "vonmises-1e+06", "poisson-10000", "poisson-100000", "poisson-1e+06",
        "gamma-1000", "inverse_gamma-1000")
SCALAR = {c.name: c for c in scalar_cases()}
EXACT = tuple(n for n in SCALAR if n not in WIDE)
assert set(WIDE) <= set(SCALAR)

# matrix families: (d, parameter); every (row, col) is a case
LKJ = tuple((d, eta) for d in (2, 3, 8) for eta in (0.5, 2.0))
WISHART = tuple((d, d + 1.5) for d in (2, 3, 8))
WISHART_MULT = 0.5


def lkj_params(d, eta, row, col):
    return _p("lkjcholesky", k=d, row=row, col=col, a=eta)


def wishart_params(d, df, row, col):
    return _p("wishart", k=d, row=row, col=col, a=df, b=WISHART_MULT)


def idx_of(n, offset=0):
    return np.arange(n, dtype=np.uint64) + np.uint64(offset)


_memo = {}


def statement(name, params, n, offset=0, dtype=np.float64, family=None):
    """The statement's Draw for a case, computed once per process and shared (never written to)."""
    key = (name, n, offset, dtype)
    if key not in _memo:
        _memo[key] = R.distro_ref(family or SCALAR[name].family, params, SEED, STREAM, idx_of(n, offset), dtype)
        for arr in _memo[key]:
            arr.setflags(write=False)
    return _memo[key]


# ------------------------------------------------------------------------------------------------ the one-sample tests
def law_ok(law, values):
    """(ok, statistic, bound) of ``values`` against the exact law: KS for a continuous law, chi-square against the pmf (bins with
    expectation below 20 pooled) for Poisson."""
    x, dist, *clamp = law(np.asarray(values, dtype=np.float64))
    lo, hi = clamp if clamp else (None, None)
    if isinstance(dist.dist, stats.rv_discrete):
        lo, hi = int(dist.ppf(1e-12)), int(dist.isf(1e-12)) + 1
        ks = np.arange(max(min(int(x.min()), lo), 0), max(int(x.max()), hi) + 1)
        if x.min() < 0 or not np.all(x == np.floor(x)):
            return False, float("nan"), ALPHA
        obs = np.bincount((x - ks[0]).astype(np.int64), minlength=ks.size).astype(np.float64)
        exp = x.size * dist.pmf(ks)
        keep = exp >= 20
        obs, exp = np.append(obs[keep], obs[~keep].sum()), np.append(exp[keep], x.size - exp[keep].sum())
        if exp[-1] < 20:  # the pooled bin joins its smallest neighbour
            i = int(np.argmin(exp[:-1]))
            obs[i], exp[i] = obs[i] + obs[-1], exp[i] + exp[-1]
            obs, exp = obs[:-1], exp[:-1]
        p = stats.chisquare(obs, exp).pvalue
        return bool(p > ALPHA), float(p), ALPHA
    # sup |F_n - F| on both sides of every sample point; a law clamped at ``lo`` / ``hi`` (FLT_MIN under a gamma) has an atom there
    xs, counts = np.unique(x, return_counts=True)
    right = np.cumsum(counts) / x.size
    left = right - counts / x.size
    f_left = f_right = dist.cdf(xs)
    if lo is not None:
        f_left, f_right = np.where(xs <= lo, 0.0, f_left), np.where(xs < lo, 0.0, f_right)
    if hi is not None:
        f_left, f_right = np.where(xs > hi, 1.0, f_left), np.where(xs >= hi, 1.0, f_right)
    d = max(np.abs(right - f_right).max(), np.abs(left - f_left).max())
    bound = math.sqrt(-math.log(ALPHA / 2) / (2 * x.size))
    return bool(d < bound), float(d), bound


@pytest.mark.parametrize("name", sorted(SCALAR))
def test_statement_follows_the_exact_law(name):
    case = SCALAR[name]
    ok, stat, bound = law_ok(case.law, statement(name, case.params, N_LAW).value)
    assert ok, (name, stat, bound)


def test_law_check_sees_a_wrong_parameter():
    case = SCALAR["gamma-3"]
    assert not law_ok(lambda x: (x, stats.gamma(3.0, scale=0.5 * 1.02)), statement("gamma-3", case.params, N_LAW).value)[0]
    assert not law_ok(lambda x: (x, stats.poisson(30.0 * 1.01)), statement("poisson-30", SCALAR["poisson-30"].params, N_LAW).value)[0]


def _matrix_draws(family, d, par, make_params):
    cache, idx = {}, idx_of(N_LAW)
    return lambda row, col: R.distro_ref(family, make_params(d, par, row, col), SEED, STREAM, idx, cache=cache).value


@pytest.mark.parametrize("d,eta", LKJ)
def test_lkjcholesky_statement(d, eta):
    """Diagonal: 1 - L_ii^2 ~ Beta(i - 1/2, eta + (d - 2) / 2 - (i - 1) / 2); below it a two-sample test against torch; the rows are unit
    vectors."""
    draw = _matrix_draws("lkjcholesky", d, eta, lkj_params)
    torch.manual_seed(d * 10 + int(eta * 2))
    host = torch.distributions.LKJCholesky(d, torch.tensor(eta)).sample((N_LAW,)).double().numpy()
    assert np.all(draw(0, 0) == 1.0) and np.all(draw(0, d - 1) == 0.0)
    for i in range(1, d):
        ok, stat, bound = law_ok(lambda x, i=i: (1.0 - x * x, stats.beta(i - 0.5, eta + 0.5 * (d - 2) - 0.5 * (i - 1))), draw(i, i))
        assert ok, (d, eta, i, stat, bound)
        norm = sum(draw(i, j) ** 2 for j in range(i + 1))
        assert np.abs(norm - 1.0).max() < 1e-12
        for j in range(i):
            stat = stats.ks_2samp(draw(i, j), host[:, i, j]).statistic
            assert stat < KS_TWO, (d, eta, i, j, stat, KS_TWO)


@pytest.mark.parametrize("d,df", WISHART)
def test_wishart_statement(d, df):
    """Diagonal / multiplier ~ chi2(df); off the diagonal a two-sample test against torch; the matrix is symmetric."""
    draw = _matrix_draws("wishart", d, df, wishart_params)
    torch.manual_seed(d)
    host = torch.distributions.Wishart(torch.tensor(df), covariance_matrix=WISHART_MULT * torch.eye(d)).sample((N_LAW,)).double().numpy()
    for i in range(d):
        ok, stat, bound = law_ok(lambda x: (x / WISHART_MULT, stats.chi2(df)), draw(i, i))
        assert ok, (d, df, i, stat, bound)
        for j in range(i):
            assert np.array_equal(draw(i, j), draw(j, i))
            stat = stats.ks_2samp(draw(i, j), host[:, i, j]).statistic
            assert stat < KS_TWO, (d, df, i, j, stat, KS_TWO)


# ------------------------------------------------------------------------------------------------ fp32 evaluation, the ambiguity cap
@pytest.mark.parametrize("name", EXACT)
def test_ambiguous_share_is_capped_and_fp32_takes_the_same_decisions(name):
    """From the statement alone: at most AMBIGUOUS_CAP of the elements of an element-exact case may be left out of the comparison on the
    device, and on every other element the fp32 evaluation takes the fp64 evaluation's decisions (the guard is wide enough)."""
    case = SCALAR[name]
    r64, r32 = statement(name, case.params, N_LAW), statement(name, case.params, N_LAW, dtype=np.float32)
    assert r64.ambiguous.mean() <= AMBIGUOUS_CAP, (name, r64.ambiguous.mean())
    clear = ~r64.ambiguous
    assert np.array_equal(r64.path[clear], r32.path[clear]), (name, int((r64.path != r32.path)[clear].sum()))
    assert r32.value.dtype == np.float32 and np.isfinite(r32.value).all()


@pytest.mark.parametrize("family,grid,make_params", (("lkjcholesky", LKJ, lkj_params), ("wishart", WISHART, wishart_params)))
def test_ambiguous_share_of_the_matrix_families(family, grid, make_params):
    n = (1 << 16)
    for d, par in grid:
        c64, c32, idx = {}, {}, idx_of(n)
        for row in range(d):
            for col in range(row + 1):
                r64 = R.distro_ref(family, make_params(d, par, row, col), SEED, STREAM, idx, cache=c64)
                r32 = R.distro_ref(family, make_params(d, par, row, col), SEED, STREAM, idx, np.float32, cache=c32)
                assert r64.ambiguous.mean() <= AMBIGUOUS_CAP, (family, d, par, row, col, r64.ambiguous.mean())
                assert np.array_equal(r64.path[~r64.ambiguous], r32.path[~r64.ambiguous])


# ------------------------------------------------------------------------------------------------ the statement and the host agree
def test_codes_and_host_parameters(pkg):
    hl = pkg.hip_lib
    for fam, code in R.CODES.items():
        assert getattr(hl, f"DISTRO_{fam.upper()}") == code
    assert (R.MAX_PROPOSALS, 16) == (hl.DISTRO_MAX_PROPOSALS, hl.DISTRO_MAX_EVENT)
    ng = importlib.import_module("comfyui_sonar_amd.py.noise_generation")
    for kappa in (1e-6, 0.5e-5, 2e-5, 1.0, 4.0, 1e3, 1e6):
        gen = ng.DistroNoiseGenerator.__new__(ng.DistroNoiseGenerator)  # kernel_params reads the family's name alone; no latent, no device
        gen.distro = "vonmises"
        dobj = torch.distributions.VonMises(torch.tensor([0.25]), torch.tensor([kappa]))
        p = gen.kernel_params(dobj, None, (0,))
        want = vonmises_params(0.25, kappa)
        assert p["family"] == want["family"] and p["a"] == want["a"] and p["b"] == _r(kappa)
        assert f32(p["c"]) == f32(want["c"]), (kappa, p["c"], want["c"])


# ------------------------------------------------------------------------------------------------ the comparison can fail
@pytest.mark.parametrize("name,mutate", (("beta-0.5-2", dict(block0=R.GAMMA_BLOCK0)),  # gamma slot 1 reads slot 0's blocks
                                         ("gamma-0.4", dict(boost_word=2)),            # the boost uniform taken from the acceptance word
                                         ("poisson-30", dict(block0=1)),               # proposals start one block late
                                         ("vonmises-4", dict(block0=1))))
def test_comparison_sees_a_wrong_allotment(name, mutate):
    case, n = SCALAR[name], (1 << 14) + 3
    r64, r32 = statement(name, case.params, n), statement(name, case.params, n, dtype=np.float32)
    bound, _own = R.tolerance(r64, r32)
    wrong = R.distro_ref(case.family, case.params, SEED, STREAM, idx_of(n), **mutate)
    ok, _worst, _left, where = R.compare(wrong.value, r64, bound, exact=case.family == "poisson")
    assert not ok and where.size
    assert (R.errors(wrong.value, r64.value) > bound).mean() > 0.5
    assert R.compare(r32.value, r64, bound, exact=case.family == "poisson")[0]  # and passes on the statement's own fp32 values
