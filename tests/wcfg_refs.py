"""Plain numpy restatements of the four fused WaveletCFG entry points (``hip_lib.wcfg_bands``, ``hip_lib.wcfg_lowpass``, ``hip_lib.FusedCall``,
``hip_lib.dwt2_forward`` / ``dwt2_inverse``) over oracle/dwt_oracle.py, in float64 (or float32, to MEASURE what fp32 arithmetic costs a case).
tests/test_wcfg_refs_cpu.py pins them to the reference-run fixtures of tests/golden/wavelet_cfg.npz; tests/test_gpu_wcfg_kernel_edges.py then
uses them at the kernel-level parameters the node never produces (``x = None``, ``b = None``, ``ku`` / ``kt`` / ``g`` of any value, zero and
negative scales) and at the shapes where the kernels' plans change route.

Every function works on ``[..., H, W]`` arrays, takes the wavelet by NAME (the taps come from the table the package ships, the same numbers
the tests hand to the kernels) and returns an array of the working dtype at the INPUT's size: the final rounding to fp32 is the caller's.

The case tables of the GPU module live here too, so that the CPU test can run every one of them through the oracle in both precisions.
"""
import numpy as np

from oracle import dwt_oracle as dwo

KU, KT = 0.3, 1.7
TOL_OUT = {True: 2e-6, False: 5e-5}      # WaveletCFG outputs, x max(1, peak): fp64 / fp32 arithmetic (tests/test_gpu_wavelet.py)
TOL_COEF = {True: 1e-11, False: 2e-5}    # single-level coefficients, rtol = atol
# case id -> measured max |fp32 oracle - fp64 oracle| / max(1, peak) of the cases whose fp32 oracle leaves TOL_OUT[False]; the GPU module
# allows those four times the measured value, tests/test_wcfg_refs_cpu.py checks the record.  Empty: every case stays inside.
MEASURED_FP32 = {}


# ------------------------------------------------------------------------------------------------ inputs and tables
def inputs(seed: int, planes: int, H: int, W: int):
    """(cond, uncond, x) float32 [1, planes, H, W]: Gaussians with a mean (no symmetry for an index error to hide behind), cond and
    uncond correlated so that their difference is not one more white plane."""
    rng = np.random.default_rng(seed)
    cond = rng.standard_normal((1, planes, H, W)) + 0.25
    uncond = 0.8 * cond + 0.6 * rng.standard_normal((1, planes, H, W)) - 0.1
    x = 1.5 * rng.standard_normal((1, planes, H, W)) + 0.5
    return cond.astype(np.float32), uncond.astype(np.float32), x.astype(np.float32)


def level_scales(levels: int):
    """[levels][3] (cH, cV, cD), finest level first: no two levels and no two orientations share a value."""
    return [(1.5 + 0.25 * j, 0.5 + 0.1 * j, -0.75 + 0.2 * j) for j in range(levels)]


def level_scales_same_v(levels: int):
    """As ``level_scales`` with cV's scale equal to cD's on every level (the band kernel then keeps no cV plane)."""
    return [(1.5 + 0.25 * j, -0.75 + 0.2 * j, -0.75 + 0.2 * j) for j in range(levels)]


def lowpass_weights(levels: int, yl_scale: float = 0.6):
    """(g, per-level detail scales d) as ``WaveletCFG._lowpass_plan`` builds g: g[0] = d_1, g[j] = d_{j+1} - d_j, g[J] = yl - d_J."""
    d = [1.5 + 0.25 * j * (-1) ** j for j in range(levels)]
    return [d[0], *(d[j] - d[j - 1] for j in range(1, levels)), yl_scale - d[-1]], d


def fused_tables(levels: int):
    """([4] approximation scales, [levels][4][3] detail scales) in FusedCall's order (cond, uncond, diff, final), all distinct."""
    yl = [1.1, 0.9, 2.5, 1.05]
    yh = [[tuple(1.0 + 0.1 * (k + 1) + 0.03 * j for k in range(3)), tuple(0.95 - 0.05 * k + 0.02 * j for k in range(3)),
           level_scales(levels)[j], tuple(0.9 + 0.1 * k - 0.04 * j for k in range(3))] for j in range(levels)]
    return yl, yh


def diff_tables(levels: int, yl_scale: float = 0.6, yh=None):
    """FusedCall tables of a difference-only rule."""
    one = (1.0, 1.0, 1.0)
    yh = level_scales(levels) if yh is None else yh
    return [1.0, 1.0, yl_scale, 1.0], [[one, one, tuple(yh[j]), one] for j in range(levels)]


# ------------------------------------------------------------------------------------------------ the transform-domain pieces
def _crop(t, H, W):
    return t[..., :H, :W]


def phi(v, *, wave, levels, mode, inv_mode=None, yl_scale=1.0, yh_scales=None, inv_wave=None):
    """waverec2 of the scaled wavedec2 of v, cropped to v's size.  ``yh_scales``: [levels][3], finest level first."""
    dt = v.dtype.type
    yl, yh = dwo.wavedec2(v, wave, mode, levels)
    yl = yl * dt(yl_scale)
    if yh_scales is not None:
        yh = [band * np.asarray(yh_scales[j], dtype=v.dtype).reshape(3, 1, 1) for j, band in enumerate(yh)]
    return _crop(dwo.waverec2(yl, yh, inv_wave or wave, inv_mode or mode), *v.shape[-2:])


def ref_bands(a, b, x, *, wave, levels, mode, inv_mode=None, yh_scales, yl_scale, ku=KU, kt=KT, subtract_from_x=True, dtype=np.float64):
    """``hip_lib.wcfg_bands``: [x -] (ku b + kt Phi(a - b)); ``b`` None: v = a and no ku term."""
    a = a.astype(dtype)
    v = a if b is None else a - b.astype(dtype)
    r = dtype(kt) * phi(v, wave=wave, levels=levels, mode=mode, inv_mode=inv_mode, yl_scale=yl_scale, yh_scales=yh_scales)
    if b is not None:
        r = dtype(ku) * b.astype(dtype) + r
    return x.astype(dtype) - r if subtract_from_x else r


def ref_lowpass(cond, uncond, x, *, wave, levels, mode, inv_mode=None, g, ku=KU, kt=KT, subtract_from_x=True, dtype=np.float64):
    """``hip_lib.wcfg_lowpass``: the same form with ONE detail scale per level, handed over as the telescoped weights
    g[0] = d_1, g[j] = d_{j+1} - d_j, g[J] = yl - d_J (finest level first)."""
    if len(g) != levels + 1:
        raise ValueError("g must hold levels + 1 weights")
    d = np.cumsum(np.asarray(g[:levels], dtype=np.float64))
    yl = float(d[-1] + g[levels])
    return ref_bands(cond, uncond, x, wave=wave, levels=levels, mode=mode, inv_mode=inv_mode, yh_scales=[(float(s),) * 3 for s in d], yl_scale=yl,
                     ku=ku, kt=kt, subtract_from_x=subtract_from_x, dtype=dtype)


def _combine(c, u, s_c, s_u, s_d, s_f, blend_mode, t):
    """band_combine: blend(u s_u, (c s_c - u s_u) s_d, t) s_f; a scale that is exactly 1 is skipped, as the reference's ``!= 1.0`` tests do."""
    dt = c.dtype.type
    if s_c != 1.0:
        c = c * dt(s_c)
    if s_u != 1.0:
        u = u * dt(s_u)
    d = c - u
    if s_d != 1.0:
        d = d * dt(s_d)
    r = dwo.BLENDS[blend_mode](u, d, dt(t))
    if s_f != 1.0:
        r = r * dt(s_f)
    return r


def ref_fused(cond, uncond, x, *, wave, levels, mode, inv_mode=None, yl_scales, yh_scales, blend_mode="inject", strength=1.0, subtract_from_x=True,
              inv_wave=None, dtype=np.float64):
    """``hip_lib.FusedCall``: [x -] IDWT(band_combine(DWT cond, DWT uncond)), ``yl_scales`` [4] and ``yh_scales`` [levels][4][3] in the order
    (cond, uncond, diff, final), orientations (cH, cV, cD), finest level first."""
    cl, ch = dwo.wavedec2(cond.astype(dtype), wave, mode, levels)
    ul, uh = dwo.wavedec2(uncond.astype(dtype), wave, mode, levels)
    yl = _combine(cl, ul, *yl_scales, blend_mode, strength)
    yh = []
    for j in range(levels):
        tab = yh_scales[j]
        yh.append(np.stack([_combine(ch[j][..., k, :, :], uh[j][..., k, :, :], *(tab[n][k] for n in range(4)), blend_mode, strength)
                            for k in range(3)], axis=-3))
    r = _crop(dwo.waverec2(yl, yh, inv_wave or wave, inv_mode or mode), *cond.shape[-2:])
    return x.astype(dtype) - r if subtract_from_x else r


def ref_dwt2(x, *, wave, mode):
    """``hip_lib.dwt2_forward``: (ll [..., h, w], hi [..., 3, h, w])."""
    return dwo.dwt2(x, wave, mode)


def ref_idwt2(ll, hi, *, wave, mode, out_hw=None):
    """``hip_lib.dwt2_inverse``: ``ll`` may be one row / column larger than the bands (its leading block is used); ``out_hw`` crops."""
    h, w = hi.shape[-2:]
    out = dwo.idwt2(ll[..., :h, :w], hi, wave, mode)
    return out if out_hw is None else _crop(out, *out_hw)


def blend_coeffs(s_c, s_u, s_d, s_f, blend_mode, t):
    """blend(s_u U, s_d (s_c C - s_u U), t) s_f = A C + B U: (A, B), the two launches of ``WaveletCFG.wavelet_cfg_bands``."""
    sign = -1.0 if blend_mode == "subtract_b" else 1.0
    keep = 1.0 - t if blend_mode == "lerp" else 1.0
    return sign * t * s_d * s_c * s_f, (keep - sign * t * s_d) * s_u * s_f


def plan_sizes(H, W, levels, flen, mode, inv_mode):
    """Coefficient-plane sizes per level, or None where a level's inverse cannot cover the level below (the plans' refusal)."""
    out = []
    for _ in range(levels):
        h, w = dwo.out_len(H, flen, mode), dwo.out_len(W, flen, mode)
        hr, wr = (2 * h, 2 * w) if inv_mode == "periodization" else (2 * h - flen + 2, 2 * w - flen + 2)
        if hr < H or wr < W:
            return None
        out.append((h, w))
        H, W = h, w
    return out


# ------------------------------------------------------------------------------------------------ case tables of the GPU module
WAVES = ("haar", "db2", "db3", "db4", "db5", "db6", "db7", "db8", "db9", "db10", "bior2.2", "sym7")
MODES = dwo.MODES
MODE_CASES = ([(w, m, m, True) for w in ("db4", "db9") for m in MODES]
              + [("db4", "symmetric", "zero", True), ("db4", "reflect", "constant", True), ("db4", "zero", "periodic", True),
                 ("haar", "symmetric", "periodization", True), ("haar", "periodization", "symmetric", True),
                 ("db2", "symmetric", "periodization", False), ("db2", "periodization", "symmetric", False)])  # (wave, mode, inv_mode, accepted)
SHORT_SIZES = ((1, 8), (8, 1), (2, 2), (3, 5), (9, 11), (5, 64))
SHORT_WAVES = ("haar", "db4", "db10")
TILE_HEIGHTS = (15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 42)
TILE_CASES = [(H, 32 + i % 4, wave, mode) for i, H in enumerate(TILE_HEIGHTS) for wave, mode in (("db4", "symmetric"), ("haar", "periodization"))]
BLENDS = (("inject", 0.0), ("inject", 0.35), ("inject", 1.0), ("lerp", 0.0), ("lerp", 0.35), ("lerp", 1.0), ("subtract_b", 0.0),
          ("subtract_b", 0.35), ("subtract_b", 1.0))


def deepest_level(H, W, flen, mode, inv_mode, cap=8):
    """The deepest level count (at most ``cap``) the plans' cover rule accepts; 0: not even one level."""
    best = 0
    for levels in range(1, cap + 1):
        if plan_sizes(H, W, levels, flen, mode, inv_mode) is None:
            break
        best = levels
    return best


def special_tables(levels: int):
    """FusedCall tables holding exact 1.0, 0.0 and negative entries in each of the cond, uncond, diff and final positions: one table
    per (position, value), the other positions keep distinct ordinary values."""
    out = []
    for pos in range(4):
        for val in (1.0, 0.0, -1.25):
            yl, yh = fused_tables(levels)
            yl = list(yl)
            yl[pos] = val
            yh = [[tuple(val if (n == pos and k == (j + pos) % 3) else tab[n][k] for k in range(3)) for n in range(4)] for j, tab in enumerate(yh)]
            out.append((("cond", "uncond", "diff", "final")[pos], val, yl, yh))
    return out


# A case: which entry point, the seed and shape of its inputs, and the entry point's own keyword arguments (wavelet by name).
#   kind "bands":   wave, levels, mode, inv_mode, yh_scales, yl_scale, ku, kt, subtract_from_x, has_b
#   kind "lowpass": wave, levels, mode, inv_mode, g, ku, kt, subtract_from_x
#   kind "fused":   wave, levels, mode, inv_mode, yl_scales, yh_scales, blend_mode, strength, subtract_from_x
#   kind "node":    a difference-only WaveletCFG rule (wave, levels, mode, inv_mode, yl_scale, yh_scales, blend_mode, strength): what a refused
#                   shape falls back to; its reference is ref_fused with the rule's tables
def case(kind, seed, planes, H, W, **kw):
    return dict(kind=kind, seed=seed, planes=planes, H=H, W=W, kw=kw)


def bands_case(seed, planes, H, W, wave, levels, mode, inv_mode=None, *, yh_scales=None, yl_scale=0.6, ku=KU, kt=KT, subtract_from_x=True, has_b=True):
    return case("bands", seed, planes, H, W, wave=wave, levels=levels, mode=mode, inv_mode=inv_mode or mode,
                yh_scales=level_scales(levels) if yh_scales is None else yh_scales, yl_scale=yl_scale, ku=ku, kt=kt, subtract_from_x=subtract_from_x,
                has_b=has_b)


def lowpass_case(seed, planes, H, W, wave, levels, mode, inv_mode=None, *, ku=KU, kt=KT, subtract_from_x=True):
    return case("lowpass", seed, planes, H, W, wave=wave, levels=levels, mode=mode, inv_mode=inv_mode or mode, g=lowpass_weights(levels)[0], ku=ku,
                kt=kt, subtract_from_x=subtract_from_x)


def fused_case(seed, planes, H, W, wave, levels, mode, inv_mode=None, *, tables=None, blend_mode="lerp", strength=0.35, subtract_from_x=True):
    yl, yh = fused_tables(levels) if tables is None else tables
    return case("fused", seed, planes, H, W, wave=wave, levels=levels, mode=mode, inv_mode=inv_mode or mode, yl_scales=yl, yh_scales=yh,
                blend_mode=blend_mode, strength=strength, subtract_from_x=subtract_from_x)


def node_case(seed, planes, H, W, wave, levels, mode, inv_mode=None, *, blend_mode="lerp", strength=0.35):
    return case("node", seed, planes, H, W, wave=wave, levels=levels, mode=mode, inv_mode=inv_mode or mode, yl_scale=0.6,
                yh_scales=level_scales(levels), blend_mode=blend_mode, strength=strength)


def three(seed, planes, H, W, wave, levels, mode, inv_mode=None):
    """The same transform through all three fused entry points: (wcfg_bands, wcfg_lowpass, FusedCall with a difference-only table --
    the single-tensor route -- and FusedCall with all four tables)."""
    return [bands_case(seed, planes, H, W, wave, levels, mode, inv_mode), lowpass_case(seed + 1, planes, H, W, wave, levels, mode, inv_mode),
            fused_case(seed + 2, planes, H, W, wave, levels, mode, inv_mode, tables=diff_tables(levels)),
            fused_case(seed + 3, planes, H, W, wave, levels, mode, inv_mode)]


def reference(c, dtype=np.float64, sel=slice(None)):
    """The case's expected output [1, planes, H, W] in ``dtype`` (before the rounding to fp32); ``sel``: a slice of its planes."""
    cond, uncond, x = (t[:, sel] for t in inputs(c["seed"], c["planes"], c["H"], c["W"]))
    kw = dict(c["kw"])
    if c["kind"] == "bands":
        has_b = kw.pop("has_b")
        return ref_bands(cond, uncond if has_b else None, x, dtype=dtype, **kw)
    if c["kind"] == "lowpass":
        return ref_lowpass(cond, uncond, x, dtype=dtype, **kw)
    if c["kind"] == "fused":
        return ref_fused(cond, uncond, x, dtype=dtype, **kw)
    if c["kind"] == "node":
        yl, yh = diff_tables(kw["levels"], kw.pop("yl_scale"), kw.pop("yh_scales"))
        return ref_fused(cond, uncond, x, dtype=dtype, yl_scales=yl, yh_scales=yh, **kw)
    raise ValueError(c["kind"])


def node_params(c, high_precision):
    """``WCFGRules.build`` parameters of a "node" case."""
    kw = c["kw"]
    return dict(difference=dict(yl_scale=kw["yl_scale"], yh_scales=[list(row) for row in kw["yh_scales"]]), wave=kw["wave"], level=kw["levels"],
                padding_mode=kw["mode"], inv_padding_mode=kw["inv_mode"], difference_blend_mode=kw["blend_mode"],
                difference_blend_strength=kw["strength"], high_precision_mode=high_precision)


def filter_cases():
    """37 x 50, 3 levels, symmetric: every filter length of ``with_taps`` (2 .. 20) plus an asymmetric pair and a long symlet."""
    return {wave: three(100 + 10 * i, 3, 37, 50, wave, 3, "symmetric") for i, wave in enumerate(WAVES)}


def mode_cases():
    """33 x 47, 2 levels.  Accepted pairs go through the three entry points; a refused pair is the node's business -- at ONE level and
    only symmetric -> periodization: the shifted pair's second level reconstructs 20 x 28 for an 18 x 25 band, which the reference's
    inverse cannot take (it drops one row, not two), and periodization -> symmetric reconstructs 32 x 46 for a 33 x 47 latent, which
    the reference cannot subtract from x.  Neither has a reference result; the refusal of the LDS kernels is asserted for both."""
    out = {}
    for i, (wave, mode, inv_mode, ok) in enumerate(MODE_CASES):
        key = f"{wave}-{mode}-{inv_mode}"
        if ok:
            out[key] = three(300 + 10 * i, 3, 33, 47, wave, 2, mode, inv_mode)
        else:
            out[key] = [node_case(300 + 10 * i, 3, 33, 47, wave, 1, mode, inv_mode)] if inv_mode == "periodization" else []
    return out


def short_cases():
    """Planes shorter than the filter: the extension wraps more than once.  Per (size, wavelet): every mode at 1 level and at 8 levels,
    the deepest count the plans take (the cover rule ``Hr >= H[j-1]`` holds at every depth when both directions use one mode)."""
    out = {}
    for si, (H, W) in enumerate(SHORT_SIZES):
        for wi, wave in enumerate(SHORT_WAVES):
            flen = len(dwo.taps(wave)[0])
            cases = []
            for mi, mode in enumerate(MODES):
                deep = deepest_level(H, W, flen, mode, mode)
                for levels in sorted({1, deep}):
                    cases += three(1000 + 400 * si + 100 * wi + 10 * mi + levels, 3, H, W, wave, levels, mode)
            out[f"{H}x{W}-{wave}"] = cases
    return out


def tile_cases():
    """Heights one and two rows either side of the tile heights (8, 16, 24, 32, 40), widths with W % 4 in {0, 1, 2, 3}."""
    return {f"{H}x{W}-{wave}-{mode}": three(3000 + 10 * i, 3, H, W, wave, 2, mode) for i, (H, W, wave, mode) in enumerate(TILE_CASES)}


def level_cases():
    """haar / periodization on 256 x 128: 8 levels through all three entry points; FusedCall also at 9 (its resident deeper-levels call
    at kDeepMaxLevels = 8) and 10 levels (one beyond: the per-level tile launches)."""
    out = {"8": three(4000, 3, 256, 128, "haar", 8, "periodization")}
    for levels in (9, 10):
        out[str(levels)] = [fused_case(4000 + levels, 3, 256, 128, "haar", levels, "periodization", tables=diff_tables(levels)),
                            fused_case(4010 + levels, 3, 256, 128, "haar", levels, "periodization")]
    return out


def scale_cases():
    """The scale-table forms: cV kept or not, no second tensor, no x, special values, every blend at three strengths."""
    H, W, wave, levels, mode = 40, 36, "db4", 3, "symmetric"
    out = {"same_v": [bands_case(5000, 3, H, W, wave, levels, mode, yh_scales=level_scales_same_v(levels))],
           "any_v": [bands_case(5001, 3, H, W, wave, levels, mode)],
           "no_b": [bands_case(5002, 3, H, W, wave, levels, mode, has_b=False, ku=0.0, kt=1.0),
                    bands_case(5003, 3, H, W, wave, levels, mode, has_b=False, ku=0.0, kt=-0.8, yh_scales=level_scales_same_v(levels))],
           "no_x": [bands_case(5004, 3, H, W, wave, levels, mode, subtract_from_x=False),
                    bands_case(5005, 3, H, W, wave, levels, mode, subtract_from_x=False, has_b=False),
                    lowpass_case(5006, 3, H, W, wave, levels, mode, subtract_from_x=False),
                    fused_case(5007, 3, H, W, wave, levels, mode, subtract_from_x=False),
                    fused_case(5008, 3, H, W, wave, levels, mode, subtract_from_x=False, tables=diff_tables(levels))],
           "unit_zero_negative": [bands_case(5010, 3, H, W, wave, levels, mode, yh_scales=[(1.0, 0.0, -1.5), (0.0, -2.0, 1.0), (-0.5, 1.0, 0.0)], yl_scale=1.0),
                                  bands_case(5011, 3, H, W, wave, levels, mode, yl_scale=0.0, ku=1.0, kt=-1.0),
                                  bands_case(5012, 3, H, W, wave, levels, mode, yl_scale=-1.0, ku=0.0, kt=1.0),
                                  case("lowpass", 5013, 3, H, W, wave=wave, levels=levels, mode=mode, inv_mode=mode, g=[1.0, 0.0, -1.0, 1.0], ku=1.0, kt=1.0,
                                       subtract_from_x=True),
                                  case("lowpass", 5014, 3, H, W, wave=wave, levels=levels, mode=mode, inv_mode=mode, g=[0.0, 1.0, 0.0, -2.0], ku=0.0, kt=-1.0,
                                       subtract_from_x=True)]}
    for i, (name, val, yl, yh) in enumerate(special_tables(levels)):
        out[f"fused-{name}-{val}"] = [fused_case(5100 + i, 3, H, W, wave, levels, mode, tables=(yl, yh))]
    for i, (blend, t) in enumerate(BLENDS):
        out[f"blend-{blend}-{t}"] = [fused_case(5200 + i, 3, H, W, wave, levels, mode, blend_mode=blend, strength=t),
                                     fused_case(5300 + i, 3, H, W, wave, levels, mode, blend_mode=blend, strength=t, tables=diff_tables(levels))]
    return out


ALIGN_SHAPE = (24, 36)


def align_cases():
    H, W = ALIGN_SHAPE
    return {"bands": bands_case(6000, 3, H, W, "db4", 2, "symmetric"), "lowpass": lowpass_case(6001, 3, H, W, "db4", 2, "symmetric"),
            "bands-odd-w": bands_case(6002, 3, H, W - 1, "db4", 2, "symmetric"), "lowpass-odd-w": lowpass_case(6003, 3, H, W - 1, "db4", 2, "symmetric")}


LOOP_SMALL = dict(H=8, W=10, planes=2048 + 37, wave="haar", levels=2, mode="periodization")

# ---- LDS budget: the issue's four series, and a 12-tap one for the far side of the band kernel's ``FT <= 10`` rule; (wave, mode, levels, H)
BUDGET_SERIES = (("haar", "periodization", 1, 24), ("db4", "symmetric", 5, 24), ("db4", "symmetric", 3, 16), ("db4", "symmetric", 1, 16),
                 ("db6", "symmetric", 2, 16))
BUDGET_SMALL_W = 40  # a plane far inside the budget: three or more workgroups per CU
MODE_IDS = {"zero": 0, "symmetric": 1, "reflect": 2, "periodization": 3, "periodic": 4, "constant": 5}


def budget_boundary(query, H, levels, flen, mode, *extra):
    """(largest accepted W, smallest refused W) in 8 .. 4097 for ``query(H, W, levels, flen, mode, mode, *extra) >= 0``; the byte count
    grows with W, so the first refusal is found by bisection and confirmed on both sides.  Widths above 4096 are refused by the plans."""
    m = MODE_IDS[mode]
    ok = lambda W: query(H, W, levels, flen, m, m, *extra) >= 0  # noqa: E731
    lo, hi = 8, 4097
    assert ok(lo) and not ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo, hi


def budget_cases(lib):
    """Both sides of an LDS boundary of the two single-launch kernels for every series, element size and cV form, from the library's own
    plan queries (host functions: they pick the SHAPE, never the expected value), plus one small plane per series.
    -> list of dict(id, case, kernel, elem, lds: bytes of an accepted plane or -1, flen, node: the WaveletCFG rule of a refused plane)."""
    out = []

    def add(ident, c, kernel, elem, lds, flen, node=None):
        out.append(dict(id=ident, case=c, kernel=kernel, elem=elem, lds=int(lds), flen=flen, node=node))

    for si, (wave, mode, levels, H) in enumerate(BUDGET_SERIES):
        flen = len(dwo.taps(wave)[0])
        m = MODE_IDS[mode]
        one_per_level = [(s,) * 3 for s in lowpass_weights(levels)[1]]
        for elem in (4, 8):
            seed = 7000 + 100 * si + 10 * elem
            wa, wr = budget_boundary(lib.sonar_wcfg_lowpass_lds_bytes, H, levels, flen, mode, elem)
            add(f"low-{wave}-{levels}-e{elem}-fits", lowpass_case(seed, 2, H, wa, wave, levels, mode), "lowpass", elem,
                lib.sonar_wcfg_lowpass_lds_bytes(H, wa, levels, flen, m, m, elem), flen)
            if wr <= 4096:
                node = node_case(seed + 1, 2, H, wr, wave, levels, mode)
                node["kw"]["yh_scales"] = one_per_level  # a rule the low-pass kernel would take if the plane fitted
                add(f"low-{wave}-{levels}-e{elem}-refused", lowpass_case(seed + 1, 2, H, wr, wave, levels, mode), "lowpass", elem, -1, flen, node)
            for any_v in (0, 1):
                wa, wr = budget_boundary(lib.sonar_wcfg_bands_lds_bytes, H, levels, flen, mode, elem, any_v)
                yh = level_scales(levels) if any_v else level_scales_same_v(levels)
                add(f"bands-{wave}-{levels}-e{elem}-v{any_v}-fits", bands_case(seed + 2 + 2 * any_v, 2, H, wa, wave, levels, mode, yh_scales=yh), "bands",
                    elem, lib.sonar_wcfg_bands_lds_bytes(H, wa, levels, flen, m, m, elem, any_v), flen)
                if wr <= 4096:
                    node = node_case(seed + 3 + 2 * any_v, 2, H, wr, wave, levels, mode)
                    node["kw"]["yh_scales"] = yh
                    add(f"bands-{wave}-{levels}-e{elem}-v{any_v}-refused", bands_case(seed + 3 + 2 * any_v, 2, H, wr, wave, levels, mode, yh_scales=yh),
                        "bands", elem, -1, flen, node)
            add(f"bands-{wave}-{levels}-e{elem}-small", bands_case(seed + 8, 2, H, BUDGET_SMALL_W, wave, levels, mode), "bands", elem,
                lib.sonar_wcfg_bands_lds_bytes(H, BUDGET_SMALL_W, levels, flen, m, m, elem, 1), flen)
    return out
