"""FreeU Extreme in fp64 numpy, from the recorded fp32 filter: FreeUExtremeConfig.apply (py/nodes/freeu_extreme.py:187-230) stated once,
plus the case table that tests/golden/make_freeu_golden.py records and the tests replay (shapes: the smallest at which each route of
csrc/freeu.hip can go wrong)."""
import numpy as np

FILTERS = {
    "A": dict(alpha=1.0, max_freq=0.7071),
    "B": dict(alpha=-0.5, min_freq=0.05, max_freq=0.5),
    "C": dict(alpha=3.0),
}

# tag -> (shape, config keywords, filter name or None)
CASES = {
    "a": ((2, 8, 8, 8), dict(scale=1.3, hidden_mean=True, filter_norm=1.0), "A"),                                                 # kind 2
    "b": ((2, 8, 16, 16), dict(scale=0.8, hidden_mean=True, blend=0.7, blend_mode="lerp", filter_norm=0.0), "B"),                 # kind 1
    "c": ((2, 8, 6, 10), dict(scale=1.2, hidden_mean=False, blend=0.7, blend_mode="inject", filter_norm=1.0), "A"),               # kind 2, H != W
    "d": ((1, 4, 5, 7), dict(scale=1.5, hidden_mean=True, blend=0.7, blend_mode="subtract_b", filter_norm=1.0), "A"),             # odd: direct passes
    "e": ((2, 5, 8, 8), dict(scale=1.0, hidden_mean=True, slice=0.5, filter_norm=1.0), "B"),                                      # int(2.5) = 2 channels
    "f": ((2, 8, 8, 8), dict(scale=1.4, hidden_mean=True, slice=0.75, slice_offset=0.5), None),                                   # overrun, clamped
    "g": ((2, 8, 8, 8), dict(scale=0.9, hidden_mean=False, slice=0.25, slice_offset=0.25, blend=0.7, blend_mode="lerp"), None),   # channels 2, 3
    "h": ((2, 3, 8, 8), dict(scale=1.3, hidden_mean=True, slice=0.25), None),   # int(0.75) = 0: empty (with a filter the reference's rfft2 raises)
    "i": ((2, 8, 8, 8), dict(scale=1.0, hidden_mean=False, blend=0.7, blend_mode="subtract_b", filter_norm=0.0), "A"),           # scale 1, scalar
}
DTYPES = ("float32", "float16", "bfloat16")

# two stacked non-final configs on one map (applied in this order), and a cache hit: the config says filter C, the cache holds A
STACK = ((2, 8, 8, 8), (dict(scale=1.2, hidden_mean=True, slice=0.5, final=False, filter_norm=1.0), "A"),
         (dict(scale=0.9, hidden_mean=True, slice=0.75, slice_offset=0.25, blend=0.7, blend_mode="lerp", final=False), None))
CACHE_HIT = ((2, 8, 8, 8), dict(scale=1.3, hidden_mean=True, filter_norm=1.0), "C", "A")

# host logic: a chain head -> ... -> tail (frux_config_opt links), queried at (pct, stage, is_skip)
CHAIN = (
    dict(target="backbone", stage_1=True, start=0.0, end=0.5, final=False),
    dict(target="skip", stage_1=True, stage_2=True, start=0.2, end=1.0, final=True),
    dict(target="both", stage_2=True, start=1.0, end=1.0),               # dropped: start >= 1
    dict(target="both", stage_3=True, blend=0.0),                        # dropped: blend == 0
    dict(target="both", start=0.0, end=1.0),                             # dropped: no stage
    dict(target="both", stage_1=True, stage_3=True, start=0.0, end=0.35, final=False),
    dict(target="backbone", stage_1=True, stage_2=True, stage_3=True, start=0.3, end=0.9, final=True),
)
# a head that its own test would drop is kept all the same
CHAIN_BAD_HEAD = (dict(target="both", stage_1=True, start=1.0, end=0.0, blend=0.0), dict(target="both", stage_2=True))
QUERIES = tuple((pct, stage, skip) for pct in (0.0, 0.1, 0.2, 0.3, 0.35, 0.5, 0.75, 0.9, 1.0) for stage in (1, 2, 3) for skip in (False, True))
MODEL_CHANNELS = 4
HANDLER_CHANNELS = (16, 8, 4, 6)   # stages 1, 2, 3 and an unmapped count
HANDLER_SIGMAS = (999.0, 700.0, 650.0, 300.0, 0.0)   # with timestep(s) = s: pct = 1 - s / 999


def make_input(shape, seed):
    """Standard normal with per-sample offsets of order 1 (max - min of the channel mean stays well away from zero)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    offs = np.array([0.7, -1.1, 0.4, 1.6])[: shape[0]].reshape(-1, 1, 1, 1)
    return (x + offs).astype(np.float32)


def slice_of(features, slice_=1.0, slice_offset=0.0):
    size = int(features * slice_)
    offs = int(features * slice_offset)
    return slice(offs, offs + size)


def apply_ref(x, filt, *, scale=1.0, hidden_mean=True, slice=1.0, slice_offset=0.0, blend=1.0, blend_mode=None, **_ignored):  # noqa: A002
    """fp64: the hidden-mean map from ALL channels, the slice, irfft2(rfft2 * filt) (ortho), the scale, the blend.  Returns a new array."""
    x = np.array(x, dtype=np.float64)
    H, W = x.shape[-2:]
    with np.errstate(invalid="ignore", divide="ignore"):
        if hidden_mean:
            m = x.mean(axis=1, keepdims=True)
            lo, hi = m.min(axis=(2, 3), keepdims=True), m.max(axis=(2, 3), keepdims=True)
            s = 1.0 + (scale - 1.0) * ((m - lo) / (hi - lo))
        else:
            s = scale
        sl = slice_of(x.shape[1], slice, slice_offset)
        a = x[:, sl]
        if a.shape[1] == 0:
            return x
        f = a
        if filt is not None:
            f = np.fft.irfft2(np.fft.rfft2(a, norm="ortho") * np.asarray(filt, dtype=np.float64).reshape(H, W // 2 + 1), s=(H, W), norm="ortho")
        v = f * s
        if blend == 1.0:
            out = v
        elif blend_mode == "lerp":
            out = a + blend * (v - a)
        elif blend_mode == "inject":
            out = v * blend + a
        elif blend_mode == "subtract_b":
            out = a - v * blend
        else:
            raise KeyError(blend_mode)
        x[:, sl] = out
    return x


def spread(ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(ref.max() - ref.min())


def distance(got, ref):
    """Largest elementwise distance as a fraction of the reference's range."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / spread(ref))


HALF_EPS = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}


def reference_error(g):
    """E of the issue: the largest distance, over the recorded fp32 cases, between the reference's fp32 output and the fp64 statement."""
    worst = 0.0
    for tag, (shape, kw, fname) in CASES.items():
        filt = None if fname is None else g[f"{tag}_filter"]
        worst = max(worst, distance(np.asarray(g[f"{tag}_out_float32"]), apply_ref(np.asarray(g[f"{tag}_x"]), filt, **kw)))
    return worst
