"""-m gpu: the wave / block reductions of extremes and of the NaN flag (csrc/range_reduce.h) at their edges, through the entry points that
use them: minmax_rows, amax_mid with inner == 1, signed_rescale, image_noise_compose + image_rescale_, freeu_hidden_mean.

Min and max of floats are exact and the flag is a boolean, so every comparison is torch.equal against torch.amin / torch.amax of the CPU
tensor (tests/elementwise_refs.py for the rescales).  No case plants a mixed +0 / -0: their order is not part of the contract.

Row lengths: one wave short of, at and past the wave (63, 64, 65) and the 256-thread workgroup (255, 256, 257), more than one pass
(1025), and kLongRow = 8192 -- the first length on the 1024-thread, 16-wave instantiation -- from below, at, the next multiple of four
and far above (8191, 8192, 8196, 16387).  Each length once 16-byte aligned (row_visit's float4 path where the length allows) and once as a
view one float into its buffer (the scalar path).  Three rows per case, uniform in (-1, 1), with +1000 and -1000 planted at positions from
{0, L - 1, L / 2, 64, 1023}, different in every row: an extreme held only by wave 1, or by the last lane of the last wave, must come out.
`planted_rows` itself asserts that the reference shows the planted values.

Row loops: 2049 rows for the kernels whose grid stops at 2048 workgroups, 4097 for signed_rescale (4096): workgroup 0 reduces row 0 and
the last row through the same LDS.  Only those two rows carry planted values, +-1000 in row 0 and +-500 in the last, so a value left over
from the first row shows in the second."""
import pytest
import torch

from tests import elementwise_refs as R

pytestmark = pytest.mark.gpu

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1025, 8191, 8192, 8196, 16387]
BIG = 1000.0
NAN, INF = float("nan"), float("inf")
SIGNED_TARGETS = (-4.3, 0.0, -1.0, 3.7)  # both inner targets come from the row's own data (max_neg >= 0, min_pos < 0)


def spots(length):
    return sorted({p for p in (0, length - 1, length // 2, 64, 1023) if 0 <= p < length})


def base_rows(rows, length, seed):
    return torch.rand((rows, length), generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0


def planted_rows(length, rows=3):
    """([rows, length] on the CPU, expected min [rows], expected max [rows]); a row of one value holds +BIG or -BIG alone."""
    x = base_rows(rows, length, 1000 + length)
    at = spots(length)
    lo, hi = torch.empty(rows), torch.empty(rows)
    for r in range(rows):
        if length == 1:
            x[r, 0] = lo[r] = hi[r] = BIG if r % 2 == 0 else -BIG
            continue
        i_hi, i_lo = r % len(at), (len(at) - 1 - r) % len(at)  # the maxima walk the positions upwards, the minima downwards
        if i_lo == i_hi:
            i_lo = (i_lo + 1) % len(at)
        x[r, at[i_hi]], x[r, at[i_lo]] = BIG, -BIG
        lo[r], hi[r] = -BIG, BIG
    assert torch.equal(x.amin(dim=1), lo) and torch.equal(x.amax(dim=1), hi), "the reference does not show the planted values"
    if length > 1 and rows == 3:
        used = [(int(x[r].argmax()), int(x[r].argmin())) for r in range(rows)]
        assert len(set(used)) == rows and {p for pair in used for p in pair} == set(at), "every position is used, no two rows alike"
    return x, lo, hi


def on_device(x, aligned):
    """x [rows, length] on the GPU: at the start of its allocation, or as a contiguous view one float into a larger one."""
    rows, length = x.shape
    if aligned:
        d = x.cuda()
    else:
        buf = torch.empty(rows * length + 1, device="cuda")
        d = buf[1:].view(rows, length)
        d.copy_(x)
    assert tuple(d.shape) == (rows, length) and d.is_contiguous() and d.data_ptr() % 16 == (0 if aligned else 4)
    return d


def loop_rows(rows, length=65):
    """Row-loop input: +-BIG in row 0 (first and last position), +-BIG / 2 in the last row (last and first), nothing planted between."""
    x = base_rows(rows, length, 77)
    x[0, 0], x[0, length - 1] = BIG, -BIG
    x[rows - 1, length - 1], x[rows - 1, 0] = BIG / 2, -BIG / 2
    lo, hi = x.amin(dim=1), x.amax(dim=1)
    assert (lo[0], hi[0], lo[-1], hi[-1]) == (-BIG, BIG, -BIG / 2, BIG / 2) and bool((lo[1:-1] > -1).all()) and bool((hi[1:-1] < 1).all())
    return x


@pytest.fixture(scope="module")
def hl(pkg):
    pkg.hip_lib.load()
    return pkg.hip_lib


# ------------------------------------------------------------------------------------------------ minmax_rows: a NaN never wins
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("length", LENGTHS)
def test_minmax_rows_planted(hl, length, aligned):
    x, lo, hi = planted_rows(length)
    got_lo, got_hi = hl.minmax_rows(on_device(x, aligned), 3, length)
    assert torch.equal(got_lo.cpu(), lo) and torch.equal(got_hi.cpu(), hi)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("length", LENGTHS)
def test_minmax_rows_nan(hl, length, aligned):
    """Row 0 holds one NaN, in its last position: the extremes of the rest (none for a row of one).  Row 1 is all NaN: (+inf, -inf)."""
    x, _, _ = planted_rows(length)
    x[0, length - 1] = NAN
    x[1] = NAN
    gap = torch.isnan(x)
    lo, hi = torch.where(gap, INF, x).amin(dim=1), torch.where(gap, -INF, x).amax(dim=1)
    assert (lo[1], hi[1]) == (INF, -INF) and (length == 1 or bool(torch.isfinite(lo[0]) and torch.isfinite(hi[0])))
    got_lo, got_hi = hl.minmax_rows(on_device(x, aligned), 3, length)
    assert torch.equal(got_lo.cpu(), lo) and torch.equal(got_hi.cpu(), hi)


def test_minmax_rows_row_loop(hl):
    x = loop_rows(2049)
    got_lo, got_hi = hl.minmax_rows(x.cuda(), 2049, 65)
    assert torch.equal(got_lo.cpu(), x.amin(dim=1)) and torch.equal(got_hi.cpu(), x.amax(dim=1))


# ------------------------------------------------------------------------------------------------ amax_mid, inner == 1: a NaN poisons
@pytest.mark.parametrize("use_abs", [False, True])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("length", LENGTHS)
def test_amax_row_planted_and_nan(hl, length, aligned, use_abs):
    x, _, hi = planted_rows(length)
    want = R.amax_mid(x[:, :, None], use_abs)[:, 0]
    assert torch.equal(want, torch.full((3,), BIG) if use_abs else hi)
    assert torch.equal(hl.amax_mid(on_device(x, aligned), 3, length, 1, use_abs).cpu(), want)
    x[1, length - 1] = NAN  # the last lane that holds a value: row 1 is NaN, the others keep their peaks
    got = hl.amax_mid(on_device(x, aligned), 3, length, 1, use_abs).cpu()
    assert bool(torch.isnan(got[1])) and torch.equal(got[[0, 2]], want[[0, 2]])
    assert torch.equal(torch.isnan(got), torch.isnan(R.amax_mid(x[:, :, None], use_abs)[:, 0]))


@pytest.mark.parametrize("use_abs", [False, True])
def test_amax_row_row_loop(hl, use_abs):
    x = loop_rows(2049)
    x[2048, 3] = -BIG / 4 * 3  # |x| and x disagree about the last row's peak
    got = hl.amax_mid(x.cuda(), 2049, 65, 1, use_abs).cpu()
    assert torch.equal(got, R.amax_mid(x[:, :, None], use_abs)[:, 0]) and got[2048].item() == (BIG / 4 * 3 if use_abs else BIG / 2)


# ------------------------------------------------------------------------------------------------ signed_rescale: four extremes per row
@pytest.mark.parametrize("length", [65, 257])
def test_signed_rescale_one_signed_rows(hl, length):
    """Rows with no negatives, with no positives and all zero between two mixed rows: the empty sign's (+inf, -inf) is never used, the
    others' extremes are the planted ones, and the zero row stays zero."""
    x, _, _ = planted_rows(length, rows=5)
    x[1] = x[1].abs()
    x[2] = -x[2].abs()
    x[3] = 0.0
    assert bool((x[1] > 0).all()) and bool((x[2] < 0).all()) and x[1].max() == BIG and x[2].min() == -BIG
    got = hl.signed_rescale(x.cuda(), 5, length, *SIGNED_TARGETS).cpu()
    assert torch.equal(got, R.signed_rescale(x, *SIGNED_TARGETS)) and not bool(got[3].any())


def test_signed_rescale_row_loop(hl):
    x = loop_rows(4097)
    want = R.signed_rescale(x, *SIGNED_TARGETS)
    assert torch.equal(hl.signed_rescale(x.cuda(), 4097, 65, *SIGNED_TARGETS).cpu(), want)


# ------------------------------------------------------------------------------------------------ image compose (no clamp) + rescale
@pytest.mark.parametrize("channels", [3, 4])
def test_image_compose_rescale_extreme_in_last_pixel(hl, channels):
    """One sample of 257 pixels: two workgroups, the second with the last pixel alone.  The maximum sits in the last pixel, the minimum in
    pixel 255 -- the last lane of the last wave of the first workgroup."""
    gen = torch.Generator().manual_seed(5 + channels)
    noise = torch.rand((1, channels, 1, 257), generator=gen) * 2.0 - 1.0
    image = torch.rand((1, 1, 257, channels), generator=gen)
    noise[0, 0, 0, 256], noise[0, channels - 1, 0, 255] = BIG, -BIG
    out, part_min, part_max = hl.image_noise_compose(noise.cuda(), image.cuda(), (1, 1, 257, channels), multiplier=1.0, blend_mode="simple_add",
                                                     channel_mask=(1 << channels) - 1, clamp=False)
    composed = out.cpu()
    assert torch.equal(composed, image + noise.movedim(1, -1))
    lo, hi = composed.amin().reshape(1), composed.amax().reshape(1)
    assert lo.item() == composed[0, 0, 255, channels - 1].item() and hi.item() == composed[0, 0, 256, 0].item()
    assert torch.equal(part_min[0, :2].cpu().amin().reshape(1), lo) and torch.equal(part_max[0, :2].cpu().amax().reshape(1), hi)
    want = R.minmax_rescale(composed.reshape(1, -1), lo, hi, 1e-07, 0.0, 1.0).reshape(composed.shape)
    assert torch.equal(hl.image_rescale_(out, part_min, part_max).cpu(), want)


# ------------------------------------------------------------------------------------------------ freeu_hidden_mean: a NaN poisons both
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("hw", [(7, 9), (5, 13), (25, 41)])  # 63, 65 and 1025 positions for 1024 threads
def test_freeu_hidden_extremes(hl, hw, channels):
    n = hw[0] * hw[1]
    x, lo, hi = planted_rows(n)
    maps = x[:, None, :].repeat(1, channels, 1)
    maps[:, 1:] *= 0.001  # the planted positions keep the extremes of the mean
    mean, ext = hl.freeu_hidden_mean(maps.reshape(3, channels, *hw).cuda())
    mean = mean.cpu()
    assert torch.equal(ext.cpu(), torch.stack([mean.amin(dim=1), mean.amax(dim=1)], dim=1))
    assert torch.equal(mean.argmin(dim=1), x.argmin(dim=1)) and torch.equal(mean.argmax(dim=1), x.argmax(dim=1))
    if channels == 1:
        assert torch.equal(mean, x) and torch.equal(ext.cpu(), torch.stack([lo, hi], dim=1))


def test_freeu_hidden_extremes_nan_in_last_position(hl):
    x, lo, hi = planted_rows(1025)
    x[1, 1024] = NAN
    _, ext = hl.freeu_hidden_mean(x.reshape(3, 1, 25, 41).cuda())
    ext = ext.cpu()
    assert bool(torch.isnan(ext[1]).all()) and torch.equal(ext[[0, 2]], torch.stack([lo, hi], dim=1)[[0, 2]])
