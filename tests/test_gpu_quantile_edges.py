"""GPU: csrc/quantile.hip at the edges its other test never reaches, every case from a seeded CPU generator and compared -- output and the
per-row statistics (nq, max|x|, second statistic) -- with the float64 restatement of tests/quantile_refs.py, which
tests/test_quantile_refs_cpu.py pins to the reference's recorded outputs.

  A  row lengths on both sides of every row-kernel bucket (1024, 16384, 65536), odd lengths (the scalar layout, rows off a 16-byte
     boundary) and the multi-workgroup route from 65537 on, with a short last chunk
  B  a row pointer 4 bytes off, an output pointer 4 bytes off, permuted (channels-last) inputs
  C  more rows than the grid has workgroups
  D  ties between the two order statistics of the interpolation, q = 0 and the largest q below 1, constant and zero rows
  E  a mode that lies in a later window of the search, and a count tie between windows
  F  replace*: more than 1024 compaction chunks, a partly filled last chunk, outliers at the tensor's ends and at chunk boundaries
  G  one row of more than 2^24 values
  H  infinities
"""
import functools
import importlib
import zlib

import pytest
import torch

from tests import quantile_refs as R

pytestmark = pytest.mark.gpu

TRANSCENDENTAL = ("tanh", "sigmoid", "sin", "cos", "atan")
REPLACING = ("zero", "reverse_zero", "median", "mode_2dec")  # the output jumps at |p| = nq
Q1 = 0.99999994  # the largest fp32 below 1


def _utils():
    return importlib.import_module("comfyui_sonar_amd.py.utils")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _device_run(pkg, xd, q, dim, flatten, strategy, pow_fac=0.5, nq_fac=1.0):
    """(output of utils.quantile_normalize, the [rows, 3] statistics of a statistics-only launch over the same rows), both on the CPU."""
    utils, hl = _utils(), pkg.hip_lib
    got = utils.quantile_normalize(xd, quantile=q, dim=dim, flatten=flatten, strategy=strategy, pow_fac=pow_fac, nq_fac=nq_fac)
    handler = utils.quantile_handlers[strategy]
    rows_t, rows, inner = utils._quantile_layout(xd, dim, flatten)[:3]
    op = hl.Q_CLAMP if handler.replace is not None else handler.op
    stats = hl.quantile_rows(rows_t, rows, inner, abs(q), nq_fac, 1e-8, op, q < 0, pow_fac, None)
    torch.cuda.synchronize()
    return got.cpu(), stats.cpu()


def _compare(got, stats, want, ws, strategy, pow_fac=0.5, exact_nq=None):
    """Output at the project's 2e-6 (4e-6 for transcendental strategies and a general power) scaled by the peak; nq at 2e-6 -- exactly on
    the rows of ``exact_nq`` --, max|x|, median and mode exactly, the mean as the float64 mean rounded to fp32."""
    tol = 4e-6 if strategy.startswith(TRANSCENDENTAL) or pow_fac not in (0.0, 1.0, 0.5, 2.0) else 2e-6
    peak = float(want[torch.isfinite(want)].abs().max())
    print(f"{strategy}: max |got - want| {float((got.double() - want).abs().max()):.3e} (peak {peak:.3e}), "
          f"max rel nq error {float(((stats[:, 0] - ws.nq).abs() / ws.nq.abs()).max()):.3e}")
    assert tuple(stats.shape) == (ws.nq.numel(), 3)
    torch.testing.assert_close(stats[:, 0], ws.nq, rtol=2e-6, atol=0.0)
    if exact_nq is not None:
        assert torch.equal(stats[exact_nq, 0], ws.nq[exact_nq])
    assert torch.equal(stats[:, 1], ws.maxabs)
    if strategy == "scale_down":
        torch.testing.assert_close(stats[:, 2].double(), ws.second, rtol=2e-6, atol=0.0)
    else:  # the median, the mode, the rounded float64 mean; 0 for the strategies without a second statistic
        assert torch.equal(stats[:, 2], ws.second.float())
    torch.testing.assert_close(got.double(), want, rtol=tol, atol=tol * max(1.0, peak))


def _check(pkg, x, q, dim, flatten, strategy, pow_fac=0.5, xd=None, exact_nq=None):
    got, stats = _device_run(pkg, x.cuda() if xd is None else xd, q, dim, flatten, strategy, pow_fac)
    want, ws = R.restate(x, q, dim, flatten, strategy, pow_fac)
    _compare(got, stats, want, ws, strategy, pow_fac, exact_nq)
    return got, stats


# ------------------------------------------------------------------------------------------------ A: row length and route
LENGTHS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 1028, 4099, 16383, 16384, 16385, 16388, 65535, 65536, 65537, 65540, 81923)
A_STRATEGIES = (("clamp", 0.85, 0.5), ("median", -0.65, 0.5), ("mean", 0.8, 0.5), ("scale_down", -0.6, 0.5), ("mode_2dec", 0.9, 0.5),
                ("sin_keepsign", 0.7, 0.75), ("replace_3pt_flip", 0.7, 0.5))


@functools.lru_cache(maxsize=None)
def _three_rows(inner):
    return torch.randn(3, inner, generator=_gen("rows", inner))


@pytest.mark.parametrize("strategy,q,pow_fac", A_STRATEGIES, ids=[s[0] for s in A_STRATEGIES])
@pytest.mark.parametrize("inner", LENGTHS)
def test_row_lengths_and_routes(pkg, inner, strategy, q, pow_fac):
    """Three rows, so that rows 1 and 2 of an odd length start off a 16-byte boundary; 81923 is five full chunks of the multi-workgroup
    route and a tail of 3."""
    _check(pkg, _three_rows(inner), q, 1, True, strategy, pow_fac)


# ------------------------------------------------------------------------------------------------ B: pointer offset and layout
@pytest.mark.parametrize("strategy,q", (("clamp", 0.85), ("median", -0.65), ("mode_2dec", 0.9)))
@pytest.mark.parametrize("inner", (1024, 16384, 65536, 65540))
def test_rows_four_bytes_off(pkg, inner, strategy, q):
    """The same values behind an aligned pointer, behind a contiguous view that starts one float into its buffer, and written to an
    output that starts one float into its buffer: bit for bit the same result.  (At 65540 mode_2dec is the one strategy on <1024, 0>.)"""
    utils, hl = _utils(), pkg.hip_lib
    x = _three_rows(inner)
    aligned = x.cuda()
    buf = torch.empty(3 * inner + 1, device="cuda")
    view = buf[1:1 + 3 * inner].view(3, inner)
    view.copy_(aligned)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    got, stats = _check(pkg, x, q, 1, True, strategy)
    got_view, stats_view = _device_run(pkg, view, q, 1, True, strategy)
    assert torch.equal(got_view, got) and torch.equal(stats_view, stats)
    # the library call itself, with an output whose rows are 4 bytes off
    out_buf = torch.full((3 * inner + 2,), 7.0, device="cuda")
    out = out_buf[1:1 + 3 * inner].view(3, inner)
    stats_out = hl.quantile_rows(aligned, 3, inner, abs(q), 1.0, 1e-8, utils.quantile_handlers[strategy].op, q < 0, 0.5, out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), got) and torch.equal(stats_out.cpu(), stats)
    assert float(out_buf[0]) == 7.0 and float(out_buf[-1]) == 7.0  # nothing written beside the rows


@pytest.mark.parametrize("strategy", ("clamp", "median", "replace_2pt_keepsign"))
@pytest.mark.parametrize("dim,flatten", ((1, True), (1, False), (2, True), (2, False)))
def test_channels_last_input(pkg, dim, flatten, strategy):
    x = torch.randn(2, 4, 24, 20, generator=_gen("channels-last"))
    permuted = x.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not permuted.is_contiguous() and torch.equal(permuted.cpu(), x)
    got, stats = _check(pkg, x, 0.8, dim, flatten, strategy)
    got_p, stats_p = _device_run(pkg, permuted, 0.8, dim, flatten, strategy)
    assert torch.equal(got_p, got) and torch.equal(stats_p, stats)


# ------------------------------------------------------------------------------------------------ C: more rows than the grid
@functools.lru_cache(maxsize=None)
def _many_rows(inner):
    return torch.randn(70001, inner, generator=_gen("many", inner))


@pytest.mark.parametrize("strategy,q", (("clamp", 0.85), ("median", -0.65), ("mode_1dec", 0.9), ("tanh_outliers", 0.7)))
@pytest.mark.parametrize("inner", (3, 260))
def test_more_rows_than_workgroups(pkg, inner, strategy, q):
    """70001 rows on a grid of 65535 workgroups: rows 65535 and up are a workgroup's second trip through its loop."""
    x = _many_rows(inner)
    got, stats = _device_run(pkg, x.cuda(), q, 1, True, strategy)
    want, ws = R.restate(x, q, 1, True, strategy)
    _compare(got[65535:], stats[65535:], want[65535:], R.RowStats(*(s[65535:] for s in ws)), strategy)
    _compare(got, stats, want, ws, strategy)


# ------------------------------------------------------------------------------------------------ D: ties and extreme ranks
TIE_ROWS = ("ties", "equal", "different", "last", "constant", "zeros")


def _tie_rows(inner, q):
    """[6, inner]: half-integer steps with a quarter zeros; three rows whose |p| order statistics lo and lo + 1 are planted (equal; far
    apart; far apart and held by the row's last two elements); one repeated value; zeros.  For q < 0 the rows are built so that the
    centered proxy has these magnitudes: |x| = M - m, M = max m + 0.5 (all values multiples of 0.25: the subtraction is exact)."""
    g = _gen("ties", inner, q)
    lo = R.rank_split(q, inner)[0]
    hi = min(lo + 1, inner - 1)
    base = torch.round(torch.randn(4, inner, generator=g) * 2) / 2
    base[torch.rand(base.shape, generator=g) < 0.25] = 0
    rows = [base[0]]
    for k, kind in enumerate(("equal", "different", "last"), 1):
        m = base[k].abs().sort().values
        assert float(m[0]) == 0.0
        if kind == "equal":
            m[hi] = m[lo]
        elif hi > lo:
            m[hi:] += float(m[-1]) + 1.0  # vhi > 2 * vlo
        if q < 0:
            m = (float(m[-1]) + 0.5) - m
        perm = torch.randperm(inner, generator=g)
        if kind == "last":  # the two order statistics at the row's last two elements
            others = perm[(perm != lo) & (perm != hi)]
            perm = torch.cat([others, torch.tensor(sorted({lo, hi}))])
        sign = torch.where(torch.rand(inner, generator=g) < 0.5, -1.0, 1.0)
        rows.append(m[perm] * sign)
    rows += [torch.full((inner,), -2.75), torch.zeros(inner)]
    return torch.stack(rows)


def _safe_rows(x, q):
    """Rows in which no |p| lies within 1e-4 relative of nq other than those equal to it; rows whose two order statistics are equal."""
    _, ws = R.restate(x, q, 1, True, "clamp")
    maxabs = ws.maxabs.reshape(-1, 1)
    pa = (x.sign() * (maxabs - x.abs()) if q < 0 else x).abs().double()
    nq = ws.nq.double().reshape(-1, 1)
    safe = ((pa == nq) | ((pa - nq).abs() > 1e-4 * nq)).all(dim=1)
    srt = pa.sort(dim=1).values
    lo = R.rank_split(q, x.shape[1])[0]
    return safe, srt[:, lo] == srt[:, min(lo + 1, x.shape[1] - 1)]


@pytest.mark.parametrize("q", (0.0, 0.5, Q1, -0.5))
@pytest.mark.parametrize("inner", (1000, 4096, 65536, 98304))
def test_ties_and_extreme_ranks(pkg, inner, q):
    """nq is exact wherever the two order statistics are equal.  The strategies whose output jumps at nq run over the rows where a
    one-ulp nq could not move an element across the threshold, and that is asserted of the input here: every planted, constant and zero
    row, except the rows with different order statistics at (1000, Q1) -- there frac = 1 - 6.1e-5, so nq lies within 6.1e-5 relative
    of vhi whatever the two values are -- and the unplanted row at Q1, whose top two values are what they are."""
    x = _tie_rows(inner, q)
    lo = R.rank_split(q, inner)[0]
    assert lo == {0.0: 0, 0.5: (inner - 1) // 2, -0.5: (inner - 1) // 2, Q1: inner - 2}[q]  # Q1: lo + 1 is the row's last order statistic
    safe, equal = _safe_rows(x, q)
    assert bool(equal[1]) and bool(equal[4]) and bool(equal[5]) and not bool(equal[2]) and not bool(equal[3])
    must = torch.ones(len(TIE_ROWS), dtype=torch.bool)
    if q == Q1:
        must[0] = False
        if inner == 1000:
            must[2] = must[3] = False
    assert bool(safe[must].all()), [TIE_ROWS[i] for i in range(len(TIE_ROWS)) if must[i] and not safe[i]]
    _check(pkg, x, q, 1, True, "clamp", exact_nq=equal)
    for strategy in ("mean",) + REPLACING:  # (mean jumps at nq like them)
        _check(pkg, x[safe], q, 1, True, strategy, exact_nq=equal[safe])


def test_rank_at_the_last_order_statistic(pkg):
    """lo == inner - 1, where vhi has to fall back to vlo.  rank = q * (inner - 1) rounded to fp32 with q <= 1 - 2^-24 stays below
    inner - 1 for every 1 < inner <= 2^24 (the product lies at least half a spacing under inner - 1), so the one length that gets there is
    1 (test_row_lengths_and_routes has it at other quantiles)."""
    assert all(R.rank_split(Q1, n)[0] == n - 2 for n in (2, 3, 1000, 4096, 65536, 98304, 1 << 24))
    assert R.rank_split(Q1, 1)[0] == 0
    x = torch.tensor([[1.5], [-2.0], [0.0]])
    for q in (Q1, -Q1):
        for strategy in ("clamp", "mean") + REPLACING:
            _check(pkg, x, q, 1, True, strategy, exact_nq=torch.ones(3, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ E: the mode across windows
@pytest.mark.parametrize("q", (0.9, -0.9))
@pytest.mark.parametrize("extra", (0, 1), ids=("count-tie", "upper-wins"))
@pytest.mark.parametrize("inner", (4096, 70000))
def test_mode_in_a_later_window(pkg, inner, extra, q):
    """randn * 300 rounded to two decimals spans some 200000 keys, about 25 windows of 8192.  One value planted k times near the bottom of
    the range and another k (or k + 1) times near the top: the smaller value wins the tie, the larger one the majority."""
    k = 12 if inner == 4096 else 24
    g = _gen("mode", inner)
    row = torch.randn(inner, generator=g) * 300
    where = torch.randperm(inner, generator=g)[:2 * k + extra]
    row[where[:k]] = -700.25
    row[where[k:]] = 700.25
    x = row.reshape(1, inner)
    p = x.sign() * (x.abs().amax() - x.abs()) if q < 0 else x
    rounded = torch.round(p[0], decimals=2)
    lower, upper = rounded[where[0]], rounded[where[-1]]  # (the centered proxy keeps their order: sign(x) * (max|x| - 700.25))
    keys = torch.round(rounded * 100).long()
    assert int(keys.max() - keys.min()) > 20 * 8192
    assert float(upper - lower) * 100 > 8192  # the two planted values lie in different windows
    vals, counts = rounded.unique(return_counts=True)
    assert int(counts[(vals != lower) & (vals != upper)].max()) < k
    assert int(counts[vals == lower]) == k and int(counts[vals == upper]) == k + extra
    _, stats = _check(pkg, x, q, 1, True, "mode_2dec")
    assert float(stats[0, 2]) == float(upper if extra else lower)


# ------------------------------------------------------------------------------------------------ F: replace* compaction
@functools.lru_cache(maxsize=None)
def _long_tensor():
    return torch.randn(4263001, generator=_gen("replace-long"))


@pytest.mark.parametrize("shape,dim,flatten", (((1, 4263001), 1, True), ((4263001,), None, False)), ids=("one-row", "global"))
def test_replace_beyond_1024_chunks(pkg, shape, dim, flatten):
    """4263001 values are 1041 chunks of 4096: two chunk counts per thread of the scan, and a last chunk of 3161 values."""
    _check(pkg, _long_tensor().reshape(shape), 0.7, dim, flatten, "replace_2pt")


REPLACE_VARIANTS = tuple(f"replace_{c}pt{f}{s}" for c in (2, 3) for f in ("", "_flip") for s in ("", "_keepsign", "_avoidsign"))
EDGES = (0, 1, 2, 9099, 9100, 9101) + tuple(range(4094, 4099)) + tuple(range(8190, 8195))


@functools.lru_cache(maxsize=None)
def _three_chunks():
    g = _gen("replace-chunks")
    x = torch.randn(9102, generator=g)
    x[list(EDGES)] = torch.where(torch.rand(len(EDGES), generator=g) < 0.5, -1.0, 1.0) * (50.0 + torch.arange(len(EDGES)))
    return x.reshape(2, 3, 41, 37)


@pytest.mark.parametrize("strategy", REPLACE_VARIANTS)
@pytest.mark.parametrize("dim,flatten", ((1, True), (2, False)), ids=("dim1-flat", "dim2-stride37"))
def test_replace_variants_across_chunks(pkg, dim, flatten, strategy):
    """9102 values: three chunks with a tail.  The tensor's first and last three elements and the elements around both 4096 boundaries are
    outliers by construction, so the rolls wrap around the tensor's ends and cross the chunks."""
    x = _three_chunks()
    assert strategy in _utils().quantile_handlers
    rows, back = R._rows(x, dim, flatten)
    _, ws = R.restate(x, 0.7, dim, flatten, "clamp")
    outlier = back(rows.abs() > ws.nq.reshape(-1, 1)).reshape(-1)
    assert bool(outlier[list(EDGES)].all())
    _check(pkg, x, 0.7, dim, flatten, strategy)


@pytest.mark.parametrize("strategy", ("replace", "replace_3pt_flip_keepsign"))
def test_replace_with_one_candidate(pkg, strategy):
    g = _gen("replace-single")
    x = torch.randn(9102, generator=g).sign() * (torch.rand(9102, generator=g) + 1.0)
    x[5000] = 0.01
    x = x.reshape(2, 3, 41, 37)
    got, _ = _check(pkg, x, 0.0, 0, True, strategy)
    assert int((got.abs().reshape(-1) - 0.1).abs().lt(1e-6).sum()) == 9102  # sqrt(0.01) everywhere


# ------------------------------------------------------------------------------------------------ G: a row beyond 2^24
@functools.lru_cache(maxsize=None)
def _huge_row():
    return torch.randn(1, 16777216 + 4099, generator=_gen("huge"))


@pytest.mark.parametrize("strategy,q", (("clamp", 0.75), ("median", -0.5)))
def test_a_row_of_more_than_2_pow_24_values(pkg, strategy, q):
    """torch.quantile refuses this row; the restatement sorts it (a couple of seconds on the CPU)."""
    _check(pkg, _huge_row(), q, 1, True, strategy)


# ------------------------------------------------------------------------------------------------ H: infinities
@pytest.mark.parametrize("strategy", ("clamp", "median", "zero"))
@pytest.mark.parametrize("inner", (1025, 65537))
def test_infinities_in_a_row(pkg, inner, strategy):
    """+inf and -inf sort above every finite |x|; max|x| is inf.  (NaN: tests/test_gpu_quantile.py pins what a row with one does.)"""
    x = _three_rows(inner).clone()
    x[0, 0], x[0, inner // 2], x[1, inner - 1], x[2, 1], x[2, inner - 2] = float("inf"), -float("inf"), float("inf"), -float("inf"), -float("inf")
    got, stats = _check(pkg, x, 0.85, 1, True, strategy)
    assert bool(torch.isinf(stats[:, 1]).all()) and bool(torch.isfinite(got).all())
