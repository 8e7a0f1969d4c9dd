"""Shared by tests/test_elementwise_refs_cpu.py and tests/test_gpu_elementwise.py: plain torch restatements of the operations that
the step kernels (csrc/sampler_steps.hip) and the noise-type helpers (csrc/elementwise.hip, rows.hip, spectral_ops.hip) implement, the seeded inputs the GPU tests feed them, and the
comparison helpers.

Every restatement is dtype-generic: it computes in the dtype of its tensor arguments.  The GPU tests hand it float64 copies of the
float32 inputs the kernel receives and round the result once to float32; the CPU tests also run it in float32, next to its sibling in
oracle/sonar_oracle.py or a committed golden, so that a GPU test cannot pass or fail for the restatement's own reasons.  The op order
of each is the one in the comment above its kernel.

Momentum is not restated: the step references drive ``oracle.sonar_oracle.MomentumState`` (py/sonar.py:169-320, pinned to the
reference by tests/test_oracle_golden.py) on the tensors they are given, with the kernels' scalars as arguments.
"""
import math
import os
import warnings

import numpy as np
import torch

from oracle import sonar_oracle as orc

RTOL, ATOL = 1e-5, 1e-6                    # the project's elementwise tolerance (tests/test_gpu_kernels.py)
TINY32 = float(torch.finfo(torch.float32).tiny)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def f32(v) -> float:
    """The value a C `float` argument takes: scalars go to the kernel and to the reference as the same number."""
    return float(np.float32(float(v)))


# ------------------------------------------------------------------------------------------------ comparison
def within(got, want64, *, floor=0.0, exclude=None):
    """got (float32, rounded results of a kernel) against want64 (float64 reference): |got - want| <= max(ATOL + RTOL |want|, floor)
    at every element.  Positions where the reference is NaN or infinite (``exclude``: the mask the test chose IN ADVANCE, which must be
    exactly those positions and fewer than 1 % of the elements) are compared in kind instead."""
    got = got.detach().cpu()
    want64 = want64.detach().cpu()
    assert got.shape == want64.shape, (tuple(got.shape), tuple(want64.shape))
    special = ~torch.isfinite(want64)
    if exclude is None:
        assert not bool(special.any()), "the reference has NaN / inf where the test planned none"
    else:
        exclude = exclude.cpu()
        assert torch.equal(special, exclude), "NaN / inf of the reference are not where the test placed them"
        assert int(exclude.sum()) * 100 < exclude.numel(), "more than 1 % of the elements excluded"
        g, w = got[exclude].double(), want64[exclude]
        assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(g[~torch.isnan(g)], w[~torch.isnan(w)]), "NaN / inf differ in kind"
    ok = ~special
    err = (got.double() - want64).abs()[ok]
    allow = (ATOL + RTOL * want64.abs()[ok]).clamp(min=float(floor))
    bad = err > allow
    assert not bool(bad.any()), f"{int(bad.sum())} of {err.numel()} elements off; worst |err| {float(err.max()):.3e} (allowed {float(allow[err.argmax()]):.3e})"


def ref32_error(fn, *args64, **kw) -> float:
    """max |fn in float32 - fn in float64| on the given float64 inputs (tensors cast down, everything else passed as is): the error
    of the same restatement computed in float32 on the host.  Transcendental kernels are allowed four times that (``floor`` of
    ``within``), never less than the project tolerance; the bound comes from the reference alone."""
    def down(a):
        if isinstance(a, torch.Tensor) and a.dtype == torch.float64:
            return a.float()
        if isinstance(a, torch.Tensor) and a.dtype == torch.complex128:
            return a.to(torch.complex64)
        return a

    def flat(o):
        o = o if isinstance(o, (tuple, list)) else (o,)
        return [torch.view_as_real(t) if t.is_complex() else t for t in o if isinstance(t, torch.Tensor)]

    hi, lo = flat(fn(*args64, **kw)), flat(fn(*[down(a) for a in args64], **kw))
    worst = 0.0
    for a, b in zip(hi, lo):
        d = (a.double() - b.double()).abs()
        d = d[torch.isfinite(d)]
        worst = max(worst, float(d.max()) if d.numel() else 0.0)
    return worst


# ------------------------------------------------------------------------------------------------ launch_ew family
def scalar_op(op, a, b, s):
    return a * s if op == 0 else a / s if op == 1 else (a - b) / s


def affine(x, sub, mul, add):
    return (x - sub) * mul + add


def sq_acc(acc, z, mul, first):
    return (torch.zeros_like(acc) if first else acc) + mul * (z * z)


def axpby(y, ymul, x, xmul):
    """y*ymul + x*xmul and the (sum, sum of squares) of the result."""
    v = y * ymul + x * xmul
    return v, v.sum(), (v * v).sum()


def powerlaw(x, alpha, use_sign):
    """py/noise_generation.py:775-786: (sign(x) or x) * |x|^alpha."""
    return (torch.sign(x) if use_sign else x) * torch.abs(x) ** alpha


def laplace_add(x, u, div_fac, loc, scale):
    """py/noise_generation.py:789-802: x / div_fac + (loc - scale * sign(u) * log1p(-max(|u|, tiny)))."""
    return x / div_fac + (loc - scale * torch.sign(u) * torch.log1p(-u.abs().clamp(min=TINY32)))


def studentt(x, g, loc, scale, df):
    """py/noise_generation.py:652-677: loc + scale * (x * rsqrt(max(g / 0.5, tiny) / df))."""
    z = (g / 0.5).clamp(min=TINY32)
    return loc + scale * (x * (1.0 / torch.sqrt(z / df)))


def norm_decision(x, factor, thr_sd=2.5):
    """py/utils.py:100-105 on the statistics of x: (mean, unbiased std, subtract?, divide?)."""
    n = x.numel()
    mean, sd = float(x.mean()), float(x.std())
    thr = thr_sd / math.sqrt(n)
    return mean, sd, abs(mean) > thr, abs(1.0 - sd) > thr, float(factor)


def apply_norm(x, dec):
    mean, sd, sub, div, factor = dec
    if sub:
        x = x - mean
    if div:
        x = x / sd
    return x * factor if factor != 1.0 else x


def norm_noise(case, shape, seed=12):
    """The noise of test_step_kernels_apply_a_pending_normalisation_like_scale_noise (tests/test_gpu_round2.py) at a given shape, and
    the factor that goes with it: 'shift_and_scale' 1.7 z + 0.4, 'scale_only' 0.6 z, 'as_is' z standardised (factor 1).  The draw z is
    centred first: at a hundred elements its own mean would otherwise decide on which side of the threshold a case falls."""
    z = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    z = z - z.mean()
    if case == "shift_and_scale":
        return z * 1.7 + 0.4, 1.3
    if case == "scale_only":
        return z * 0.6, 1.3
    assert case == "as_is"
    z = z.double()
    return ((z - z.mean()) / z.std()).float(), 1.0


NORM_OUTCOMES = {"shift_and_scale": (True, True), "scale_only": (False, True), "as_is": (False, False)}


# ------------------------------------------------------------------------------------------------ the sampler steps
def _state(cfg, h, h_fresh):
    if h_fresh:
        assert cfg.init == "RAND" and h is not None and cfg.rand_init_noise_multiplier == 1
        return orc.MomentumState(cfg, rand_init=lambda: h)
    st = orc.MomentumState(cfg)
    st.h = h
    return st


def _with_noise(x, noise, noise_scale, norm):
    if noise is None:
        return x
    return x + (noise if norm is None else apply_norm(noise, norm)) * noise_scale


def euler_step(cfg, step, x, den, h, sigma, dt, *, noise=None, noise_scale=0.0, norm=None, h_fresh=False):
    """sonar_momentum_euler_f32: py/sonar.py:309-320 with dt given, then x += norm(noise) * noise_scale.  Returns (x_out, h or None)."""
    st = _state(cfg, h, h_fresh)
    den_m = st.momentum_denoised(x, den, sigma, step)
    md = st.momentum_d(x, den_m, sigma, step)
    return _with_noise(md * dt + x, noise, noise_scale, norm), st.h


def dpmpp_stage1(cfg, step, x, den, h, sigma, expm1_a, ratio_a, adj_is_one, *, noise=None, noise_scale=0.0, norm=None, h_fresh=False):
    """sonar_dpmpp_stage1_f32: the first half step of oracle.sonar_dpmpp_sde (md1 ... x_2 += noise).  Returns (x2, md1, h or None)."""
    st = _state(cfg, h, h_fresh)
    md1 = st.momentum_denoised(x, den, sigma, step)
    diff_2 = expm1_a * md1
    m_d = st.momentum_d(x, md1, sigma, step, gate_momentum=1 if adj_is_one else 0.5, d=diff_2)
    return _with_noise(ratio_a * x - m_d, noise, noise_scale, norm), md1, st.h


def dpmpp_stage2(cfg, step, x, den2, md1, h, sigma_s, expm1_b, ratio_b, fac, adj_is_one, *, noise=None, noise_scale=0.0, norm=None):
    """sonar_dpmpp_stage2_f32: the second half step (md2 ... x += noise).  Returns (x_out, dd, h or None)."""
    st = _state(cfg, h, False)
    md2 = st.momentum_denoised(x, den2, sigma_s, step)
    dd = (1 - fac) * md1 + fac * md2
    diff_1 = expm1_b * dd
    m_d = st.momentum_d(x, md2, sigma_s, step, gate_momentum=1 if adj_is_one else 0.5, d=diff_1)
    return _with_noise(ratio_b * x - m_d, noise, noise_scale, norm), dd, st.h


def dpmpp_scalars(sigma, sigma_next, eta, s_noise):
    """The scalars the host hands the two stage kernels for one step of oracle.sonar_dpmpp_sde (r = 1/2), from tensors of any dtype."""
    tf = lambda s: s.log().neg()  # noqa: E731
    sig = lambda t: t.neg().exp()  # noqa: E731
    t, t_next = tf(sigma), tf(sigma_next)
    s = t + (t_next - t) * 0.5
    s_t, s_s, s_t_next = sig(t), sig(s), sig(t_next)
    sd, su = orc.ancestral_step(s_t, s_s, eta)
    s_ = tf(sd)
    out = dict(sigma=sigma, sigma_s=s_s, fac=1.0, expm1_a=(t - s_).expm1(), ratio_a=sig(s_) / s_t, noise_scale_a=s_noise * su)
    sd, su = orc.ancestral_step(s_t, s_t_next, eta)
    t_down = tf(sd)
    out.update(expm1_b=(t - t_down).expm1(), ratio_b=sig(t_down) / s_t, noise_scale_b=s_noise * su)
    return out


# ------------------------------------------------------------------------------------------------ reductions over a middle axis
def std_mid(x):
    """x [outer, mid, inner] -> unbiased std over mid, [outer, inner]; mid == 1 gives NaN like torch.std."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch warns about the degrees of freedom at mid == 1; the NaN is the point)
        return x.std(dim=1, unbiased=True)


def amax_mid(x, use_abs):
    return (x.abs() if use_abs else x).amax(dim=1)


def div_mid(x, d):
    return x / d[:, None, :]


def mul_table(x, table, inner, follow_sign):
    """x flat; x[i] *= table[(i // inner) % len]; with follow_sign the result takes the sign of 1 - table (py/noise.py:1134-1202)."""
    s = table[(torch.arange(x.numel()) // inner) % table.numel()].reshape(x.shape)
    v = x * s
    return torch.copysign(v, 1.0 - s) if follow_sign else v


def row_affine(op, x, a, b):
    """x [rows, inner], a / b [rows]: op 0 (x - a) / b, op 1 x * b + a."""
    return (x - a[:, None]) / b[:, None] if op == 0 else x * b[:, None] + a[:, None]


def clamp_signpow_rows(x, limit, mul, p):
    """x [rows, inner]: copysign(|clamp(x, -lim, lim)|^p, x) with lim = limit[row] * mul."""
    lim = (limit * mul)[:, None]
    v = torch.minimum(torch.maximum(x, -lim), lim)
    return torch.copysign(v.abs() ** p, v)


# ------------------------------------------------------------------------------------------------ ModulatedNoise helpers
def bcast_std_view(stdv, outer, mid, inner, bcast):
    """The [outer, mid, inner]-broadcastable view of the std vector of bcast mode 0 (per outer), 1 (per outer, mid), 2 (per outer, inner)."""
    return stdv.reshape((outer, 1, 1) if bcast == 0 else (outer, mid, 1) if bcast == 1 else (outer, 1, inner))


def bcast_gain(x, stdv, bcast, abs_strength, k):
    """py/noise.py:799-803: plain = x k; v = plain * (1 / (std |strength| + 1)) + plain.  Returns (v, sum x^2, sum v^2)."""
    outer, mid, inner = x.shape
    plain = x * k
    v = plain * (1.0 / (bcast_std_view(stdv, outer, mid, inner, bcast) * abs_strength + 1.0)) + plain
    return v, (x * x).sum(), (v * v).sum()


def ratio_mix(a, a_mul, x, x_mul, num_sum, num_mul, den_sum):
    """py/noise.py:805-810: a * (a_mul * sqrt(num_mul * num / den)) + x * x_mul."""
    return a * (a_mul * math.sqrt(num_mul * float(num_sum) / float(den_sum))) + x * x_mul


# ------------------------------------------------------------------------------------------------ rescales
def minmax_rescale(x, lo, hi, eps, tmin, tmax):
    """normalize_to_scale's tail (py/utils.py:462-469), x [rows, inner], lo / hi [rows], one tensor op per reference tensor op (the
    targets are Python floats there, so their difference is formed in double and meets the tensor once)."""
    out = x - lo[:, None]
    out /= (hi - lo)[:, None].clone().add_(eps)
    return out.mul_(tmax - tmin).add_(tmin).clamp_(tmin, tmax)


def normalize_to_scale(x, tmin, tmax, eps=1e-07):
    """py/utils.py:452-470 over each row of x [rows, inner]."""
    return minmax_rescale(x, x.amin(dim=1), x.amax(dim=1), eps, tmin, tmax)


def signed_rescale(x, min_neg, max_neg, min_pos, max_pos):
    """normalize_to_scale_adv (py/utils.py:473-510) over each row of x [rows, inner]: negatives and positives rescaled separately,
    each between its own extremes; a target that is out of range on the inside comes from the data; a skipped sign is copied; zeros
    (and NaN, which is neither < 0 nor > 0) come out 0."""
    skip_pos = max_pos <= 0 or min_pos >= max_pos
    skip_neg = min_neg >= 0 or min_neg >= max_neg
    out = torch.zeros_like(x)
    for r in range(x.shape[0]):
        t = x[r]
        neg, pos = t < 0.0, t > 0.0
        if skip_neg:
            out[r][neg] = t[neg]
        elif bool(neg.any()):
            v = t[neg]
            hi = v.max().item() if max_neg >= 0 else max_neg
            out[r][neg] = normalize_to_scale(v[None], min_neg, hi)[0]
        if skip_pos:
            out[r][pos] = t[pos]
        elif bool(pos.any()):
            v = t[pos]
            lo = v.min().item() if min_pos < 0 else min_pos
            out[r][pos] = normalize_to_scale(v[None], lo, max_pos)[0]
    return out


def load_signed_rescale_golden():
    """tests/golden/signed_rescale.npz (make_signed_rescale_golden.py): rows [8, 12] and, per case, the four targets and the REAL
    reference's normalize_to_scale_adv of every row."""
    data = np.load(os.path.join(GOLDEN, "signed_rescale.npz"), allow_pickle=False)
    rows = torch.from_numpy(data["rows"])
    names = [str(n) for n in data["row_names"]]
    cases = {str(n): (tuple(float(v) for v in data[f"{n}_targets"]), torch.from_numpy(data[f"{n}_out"])) for n in data["case_names"]}
    return rows, names, cases


# ------------------------------------------------------------------------------------------------ spectral helpers
def cdft_mid(z, inverse, real_out):
    """z [outer, C, inner] real or complex: DFT along C; the inverse without its 1 / C."""
    out = torch.fft.ifft(z, dim=1) * z.shape[1] if inverse else torch.fft.fft(z, dim=1)
    return out.real if real_out else out


def spectrum_of(x, channel_dft):
    """x real [B, C, H, W] -> its spectrum over (H, W), or over (C, H, W) with channel_dft."""
    return torch.fft.fftn(x, dim=(-3, -2, -1)) if channel_dft else torch.fft.fft2(x)


def logamp(z):
    """la = log|z| of the spectrum handed to the kernel (half or full)."""
    return torch.log(torch.sqrt(z.real * z.real + z.imag * z.imag))


def full_abs_logamp(x, channel_dft):
    """|log|F x|| at every bin of the FULL spectrum of the real input: what the kernel rebuilds from a half spectrum's Hermitian partners."""
    return logamp(spectrum_of(x, channel_dft)).abs()


def signum_mult(a, q, intensity):
    """py/noise.py:975-1003 for log-amplitudes a and quantiles q = (low, high, max), all broadcastable."""
    ql, qh, qm = q
    one = torch.ones_like(a)
    hi = torch.where(a > qh, 1.0 - torch.minimum((a - qh) / (qm - qh), 0.5 * one), one)
    lo = torch.where(a < ql, 1.0 + torch.minimum(1.0 - a / ql, 0.5 * one), one)
    return (lo * hi) ** intensity


def spectral_signum_mask(z, la, q, C, intensity, gain, channel_sym):
    """z complex [B * C, elems], la [B * C, elems], q [nq, 3] (nq 1 or C): z * gain * mask, the quantile row of a plane being its
    channel's (nq == C) or row 0; channel_sym averages the masks of channel c and (C - c) % C."""
    planes = z.shape[0]
    c = torch.arange(planes) % C
    nq = q.shape[0]
    pick = lambda idx: tuple(q[idx, j][:, None] for j in range(3))  # noqa: E731
    m = signum_mult(la, pick(torch.zeros_like(c) if nq == 1 else c), intensity)
    if channel_sym and nq != 1:
        m = 0.5 * (m + signum_mult(la, pick((C - c) % C), intensity))
    return z * (m * gain)
