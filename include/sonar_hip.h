/*
 * sonar_hip.h — C ABI of libsonar_hip.so (MI355X / gfx950 only).
 *
 * This is the drop-in boundary for the procedural-noise + momentum-step + wavelet-split hot
 * path of blepping/ComfyUI-sonar (last row).  The reference is 100 % Python over
 * torch ops, so it has no FFI of its own; every entry point below replaces one torch-op
 * sequence of the reference, cited as `file:line` relative to the reference root.
 *
 * Conventions (all entry points):
 *   - returns 0 on success, SONAR_ERR_* (<0) on failure; sonar_last_error() gives the text
 *   - every buffer is a caller-owned DEVICE pointer (PyTorch-ROCm tensor.data_ptr()),
 *     contiguous NCHW, fp32 unless the name says f64; sizes are int64_t; scalars by value
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no device sync, no allocation
 *   - workspace, when needed, is passed in by the caller (sonar_*_ws_bytes gives the size)
 *   - "partials" = array of `npart` (sum, sum-of-squares) fp64 pairs produced by a producing
 *     kernel and consumed by sonar_scale_noise_f32 (which reduces them in a fixed order on
 *     device, so normalisation needs no host sync and no atomics)
 */
#ifndef SONAR_HIP_H
#define SONAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SONAR_OK 0
#define SONAR_ERR_ARG (-1)         /* null pointer / negative size / bad enum */
#define SONAR_ERR_UNSUPPORTED (-2) /* shape the kernel does not handle */
#define SONAR_ERR_HIP (-3)         /* HIP runtime error, see sonar_last_error() */

/* blend modes: py/utils.py:17-21 (BLENDING_MODES) */
#define SONAR_BLEND_LERP 0       /* torch.lerp(a, b, t) */
#define SONAR_BLEND_INJECT 1     /* a + b*t */
#define SONAR_BLEND_SUBTRACT_B 2 /* a - b*t */

/* momentum modes: py/sonar.py:40-43 */
#define SONAR_MODE_CLASSIC 0
#define SONAR_MODE_NEW 1
#define SONAR_MODE_DENOISED 2

/* history init applied inside the step when no history exists yet: py/sonar.py:169-206 */
#define SONAR_INIT_NONE 0        /* ZERO (history stays unset) or history already present */
#define SONAR_INIT_SAMPLE 1      /* history = x (denoised in DENOISED mode) */
#define SONAR_INIT_SAMPLE_NORM 2 /* history = x / sigma (denoised / sigma in DENOISED mode) */

/* number of (sum,sumsq) partial pairs every stats-producing kernel writes */
#define SONAR_NPART 1024

int sonar_abi_version(void);
const char* sonar_last_error(void);
/* Version of the GENERATE-mode value streams (device draws, cpu = False): the number changes whenever a seed gives other values than the
 * build before did -- saved seeds and workflows that use device draws are reproducible only within one version.  Replay mode (the
 * reference's host-generator draws handed in, cpu = True: the parity mode) is not versioned, its values are the reference's.
 *   3: round 3 (xoshiro128 bursts seeded by Philox4x32-10 at three depths)
 *   5: round 5 (MWC64X bursts; power-law spectra: filter weight under the radius' square root, 23 radius / 16 angle bits)
 *   6: round 6 (Brownian noise only: node bursts seeded by hashing a per-sub-tile Philox state with the node id, the power-law draw's
 *      conversions; every other generator's values are version 5's).  Version 6 has TWO Brownian families: the node bursts for one
 *      seed and latents of a multiple of 4096 elements with the call on whole latents, one Philox4x32-10 block per 4 values (counter =
 *      (element / 4, node id), key = seed) for per-latent seeds and every other shape -- a function of the shape and the seed kind,
 *      never of buffer addresses (sonar_brownian_f32).
 *   7: Distro noise's vonmises (formed from r - 1 and half-angle terms: no cancellation at large concentration) and poisson at rate >= 10
 *      (k and the slow-path inequality in double); every other value is version 6's.
 * oracle/device_streams.py states every generate-mode stream in numpy; a change of values bumps this number and that file together. */
int sonar_noise_stream_version(void);

/* ---------------------------------------------------------------- normalisation (row N) */
/* py/utils.py:100 — whole-tensor mean/std inputs: writes SONAR_NPART fp64 (sum,sumsq) pairs */
int sonar_stats_f32(const float* x, int64_t n, double* partials, void* stream);
/* reduce partials -> out3 = {sum, sumsq, n} (device fp64[3]); used for the optional cross-rank
 * all-reduce and by tests */
int sonar_stats_finalize(const double* partials, int64_t npart, int64_t n, double* out3, void* stream);
/* py/utils.py:93-106 — scale_noise: normalized=0 -> x*=factor; normalized=1 -> data-dependent
 * (x-mean)/std with thresholds threshold_std_devs/sqrt(n_total) evaluated ON DEVICE, then *factor.
 * partials/npart: from any producing kernel; n_total: element count the stats cover (may exceed
 * n when the stats were all-reduced over ranks).  In place. */
int sonar_scale_noise_f32(float* x, int64_t n, float factor, int normalized, float threshold_std_devs,
                          const double* partials, int64_t npart, int64_t n_total, void* stream);
/* sonar_scale_noise_f32(normalized = 1) that also writes the (sum, sumsq) of the RESULT into out_partials (1024 pairs; derived from the
 * input statistics and the decision, no extra pass), so a wrapper that normalises the same tensor again (chain -> scheduled -> chain,
 * py/noise.py:194,676,1405) needs no statistics sweep; when the decision is "leave as is" the kernel returns without touching x. */
int sonar_scale_noise_stats_f32(float* x, int64_t n, float factor, float threshold_std_devs, const double* partials,
                                int64_t npart, int64_t n_total, double* out_partials, void* stream);
/* py/utils.py:96-99 — normalize_dims variant: rows = groups, each of `inner` contiguous elements:
 * y = x/std_row; y -= mean_row(y); y *= factor.  (dims must be trailing & contiguous) */
int sonar_scale_noise_rows_f32(float* x, int64_t rows, int64_t inner, float factor, void* stream);

/* ---------------------------------------------------------------- elementwise (rows U, C, S, L) */
/* out = blend(a, b, t) — py/utils.py:17-21; out may alias a or b */
int sonar_blend_f32(int mode, const float* a, const float* b, float t, float* out, int64_t n, void* stream);
/* out = blend(a, b, t[i % tn]) with per-element/broadcast weights (BlendedNoise mask, py/noise.py:1364-1379) */
int sonar_blend_tensor_f32(int mode, const float* a, const float* b, const float* t, int64_t tn, float* out,
                           int64_t n, void* stream);
/* y = y*ymul + x*xmul  (chain accumulate py/noise.py:192; ancestral noise add py/sonar.py:565) */
int sonar_axpby_f32(float* y, float ymul, const float* x, float xmul, int64_t n, void* stream);
/* the same, and the (sum, sumsq) partials of the result (1024 fp64 pairs): the last accumulation of a chain feeds its scale_noise */
int sonar_axpby_stats_f32(float* y, float ymul, const float* x, float xmul, int64_t n, double* partials, void* stream);
/* ModulatedNoise spectral_signum (py/noise.py:938-1015): fftn over the modulation dims -> log amplitude -> per-sample quantiles of its
 * absolute value (sonar_abs_quantile_rows_f32 on `full`) -> soft clamp of the bins outside the 5 % / 95 % quantiles -> inverse.
 *  sonar_rfft2_f32                 z_out[planes][H][W/2+1] (complex64) = rfft2(x) unscaled, LDS-resident (power-of-two planes)
 *  sonar_cdft_mid_f32              DFT along the middle axis of complex z[outer][C][inner] (the channel axis), out of place; real_in:
 *                                  float input; real_out: real part only, float output; inverse without the 1/C
 *  sonar_spectral_logamp_f32       la = log(sqrt(re^2 + im^2)); full[planes][H][W] = |la| over the whole spectrum (dropped rfft2 columns
 *                                  from their Hermitian partners; C = channels when a channel DFT was applied, else 1)
 *  sonar_spectral_signum_mask_f32  z *= gain * (mult_low * mult_high)^intensity, q[nq][3] = (low, high, max) quantile rows: row 0 when
 *                                  nq == 1, the bin's CHANNEL index when nq == C (how the reference's expand() lines the vector up);
 *                                  channel_sym: z is a HALF spectrum under a channel DFT -> the mask is averaged with its Hermitian
 *                                  partner's (row (C - c) % C), which is what the real part of the reference's complex inverse keeps */
int sonar_rfft2_f32(const float* x, float* z_out, int64_t planes, int64_t H, int64_t W, void* stream);
int sonar_cdft_mid_f32(const float* z_in, float* z_out, int64_t outer, int64_t C, int64_t inner, int inverse, int real_in,
                       int real_out, void* stream);
int sonar_spectral_logamp_f32(const float* z, float* la, float* full, int64_t planes, int64_t C, int64_t H, int64_t W, int64_t Wz,
                              void* stream);
int sonar_spectral_signum_mask_f32(float* z, const float* la, const float* q, int64_t nq, int64_t planes, int64_t C,
                                   int64_t plane_elems, float intensity, float gain, int channel_sym, void* stream);
/* CompositeNoise py/noise.py:524-531: out = dst*(1-mask) + src*mask; mask is [mask_n] broadcast over n/mask_n */
int sonar_mask_mix_f32(const float* dst, const float* src, const float* mask, int64_t mask_n, float* out,
                       int64_t n, void* stream);
/* x = (x - sub)*mul + add in place (UniformNoiseGenerator, py/noise_generation.py:508-514) */
int sonar_affine_f32(float* x, float sub, float mul, float add, int64_t n, void* stream);
/* out = a*s (op 0) | a/s (op 1, true division) | (a-b)/s (op 2: k-diffusion to_d, py/sonar.py:300) */
int sonar_scalar_op_f32(int op, const float* a, const float* b, float s, float* out, int64_t n, void* stream);
/* per-row mean and unbiased std over `inner` contiguous elements (guidance_shift / prepare_ref_latent,
 * py/sonar.py:336-341,372-377) */
int sonar_rowstats_f32(const float* x, int64_t rows, int64_t inner, float* mean, float* stdv, void* stream);
/* op 0: out = (x - a[row]) / b[row]   op 1: out = x * b[row] + a[row]   (same call sites) */
int sonar_row_affine_f32(int op, const float* x, int64_t rows, int64_t inner, const float* a, const float* b,
                         float* out, void* stream);
/* StudentTNoiseGenerator.generate, py/noise_generation.py:667-677, in three steps:
 *  sonar_studentt_f32            x (a standard-normal draw) -> loc + scale * x * rsqrt(max(gamma/0.5, tiny) / df), gamma = the
 *                                torch._standard_gamma(df/2) draw of torch.distributions.StudentT.rsample (Chi2 = Gamma(df/2, 1/2)); in place
 *  sonar_abs_quantile_rows_f32   out[row] = torch.quantile(|x[row]|, q) with linear interpolation; the caller passes the fp32 rank
 *                                q*(inner-1) split into rank_lo + rank_frac (radix select on bit patterns, one workgroup per row)
 *  sonar_clamp_signpow_rows_f32  x = copysign(|clamp(x, -lim, lim)|^p, x), lim = limit[row] * mul; in place */
/* acc = (first ? 0 : acc) + mul*z*z -- the chi-square of an integer df as a sum of squared normals (on-device StudentT draws) */
int sonar_sq_acc_f32(float* acc, const float* z, float mul, int first, int64_t n, void* stream);
int sonar_studentt_f32(float* x, const float* gamma, float loc, float scale, float df, int64_t n, void* stream);
int sonar_abs_quantile_rows_f32(const float* x, int64_t rows, int64_t inner, int64_t rank_lo, float rank_frac, float* out,
                                void* stream);
int sonar_clamp_signpow_rows_f32(float* x, int64_t rows, int64_t inner, const float* limit, float mul, float p, void* stream);
/* Quantile filtering (utils.quantile_normalize, py/utils.py:123-449).  Rows are `inner` contiguous values.
 *  sonar_quantile_rows_ws_bytes  bytes of workspace sonar_quantile_rows_f32 needs for this shape and strategy (0: none)
 *  sonar_quantile_rows_f32   per row: nq = quantile(|p|, q) * nq_fac + eps (linear interpolation, the caller passes the fp32 rank
 *                            q*(inner-1) as rank_lo + rank_frac), p = x, or sign(x) * (max|x| - |x|) when centered = 1; then the
 *                            strategy `op` (SONAR_Q_*, the wave strategies as SONAR_Q_WAVE | SONAR_Q_WAVE_* flags), the centered
 *                            back-mapping sign(o) * (max|x| - |o|) and copysign(|o|^pow_fac, o) unless pow_fac is 0 or 1.  out (may be
 *                            NULL: statistics only) must not alias x.  stats receives [rows][3] = (nq, max|x|, second statistic: nq / max|p|
 *                            for scale_down, the mean, the lower median or the mode).  Rows of up to 65536 values are read once, one
 *                            workgroup per row; longer rows are split across workgroups (per-pass global histograms in `ws`), except
 *                            for the mode.  The mode is taken over the row's finite values.
 *  sonar_quantile_replace_ws_elems     int64 elements of the `counts` workspace for n values
 *  sonar_quantile_replace_compact_f32  the replace* candidates: the values p with |p| <= nq of their row, over the whole tensor in
 *                            memory order, into cand[n]; counts[ws - 1] = their number.  Value i belongs to statistics row
 *                            (i / (len * stride)) * stride + i % stride (stats as written by sonar_quantile_rows_f32)
 *  sonar_quantile_replace_apply_f32    out[j] = p[j] where |p[j]| <= nq, else the mean over k < count of
 *                            cand[((j - s_k) mod n) mod n_cand], s_k = k (-k for odd k when flip), then copysign toward p (sign_mode 1)
 *                            or -p (2), the centered back-mapping and the power.  Writes nothing when n_cand is 0. */
#define SONAR_Q_CLAMP 0
#define SONAR_Q_TANH 1
#define SONAR_Q_TANH_OUTLIERS 2
#define SONAR_Q_SIGMOID 3
#define SONAR_Q_SIGMOID_KEEPSIGN 4
#define SONAR_Q_SIGMOID_OUTLIERS 5
#define SONAR_Q_ATAN 6
#define SONAR_Q_TENTH 7
#define SONAR_Q_HALF 8
#define SONAR_Q_ZERO 9
#define SONAR_Q_REVERSE_ZERO 10
#define SONAR_Q_SCALE_DOWN 11
#define SONAR_Q_MEAN 12
#define SONAR_Q_MEDIAN 13
#define SONAR_Q_MODE_1DEC 14
#define SONAR_Q_MODE_2DEC 15
#define SONAR_Q_WAVE 16
#define SONAR_Q_WAVE_COS 0x100
#define SONAR_Q_WAVE_WHOLEPI 0x200
#define SONAR_Q_WAVE_WRONG 0x400
#define SONAR_Q_WAVE_KEEPSIGN 0x800
int64_t sonar_quantile_rows_ws_bytes(int64_t rows, int64_t inner, int op);
int sonar_quantile_rows_f32(const float* x, int64_t rows, int64_t inner, int64_t rank_lo, float rank_frac, float nq_fac, float eps, int op,
                            int centered, float pow_fac, float* out, float* stats, void* ws, void* stream);
int64_t sonar_quantile_replace_ws_elems(int64_t n);
int sonar_quantile_replace_compact_f32(const float* x, const float* stats, int64_t n, int64_t len, int64_t stride, int centered,
                                       float* cand, int64_t* counts, void* stream);
int sonar_quantile_replace_apply_f32(const float* x, const float* stats, int64_t n, int64_t len, int64_t stride, int centered,
                                     const float* cand, const int64_t* counts, int count, int flip, int sign_mode, float pow_fac, float* out,
                                     void* stream);
/* Distro noise (DistroNoiseGenerator, py/noise_generation.py:805-1256), generate mode.  sonar_distro_fill_f32 writes out[i], i < n, as
 * the selected component of one draw of `family` (SONAR_DISTRO_*) for global element elem_offset + i: the host has already applied
 * result_index and passes the selected component's parameters in `p`.  Every value is a pure function of (seed, stream_id, global element
 * index): Philox4x32-10 blocks with key (seed_lo, seed_hi ^ SONAR_DISTRO_DOMAIN) and counter (idx_lo, idx_hi | stream_hi << 16, block,
 * stream_lo), so idx and stream_id must be below 2^48.  Block allotment and word conversions: INTEGRATION.md 3b.  Rejection samplers stop
 * after SONAR_DISTRO_MAX_PROPOSALS proposals with a finite fallback.  Parameters must be finite and inside the family's support (the
 * host validates them through torch).  Event families take k <= 16; lkjcholesky and wishart take d = k in 2..8.
 * Fields of sonar_distro_params per family (a, b, c; v; k; row, col):
 *   exponential (lambd)  cauchy (median, sigma)  geometric (p)  log_normal / normal (mean, std)  beta (concentration1, concentration0)
 *   continuous_bernoulli (probs)  dirichlet (v = concentrations, k, row = component)  fisher_snedecor (df1, df2)
 *   gamma / inverse_gamma (concentration, rate)  gumbel / laplacian (loc, scale)  kumaraswamy (concentration1, concentration0)
 *   lkjcholesky (concentration; k = d; row, col)  lrmvariate_normal (loc, sqrt(cov_diag); v = cov_factor row, k = rank)
 *   mvariate_normal (loc, sqrt(cov_multiplier))  pareto (scale, alpha)  poisson (rate)  relaxed_bernoulli (logit, temperature)
 *   relaxed_onehotcategorical (temperature; v = logits, k, row = component)  studentt (loc, scale, df)  uniform (low, high)
 *   vonmises (loc, concentration, proposal_r - 1)  weibull (scale, concentration)  wishart (df, cov_multiplier; k = d; row, col) */
#define SONAR_DISTRO_EXPONENTIAL 0
#define SONAR_DISTRO_CAUCHY 1
#define SONAR_DISTRO_GEOMETRIC 2
#define SONAR_DISTRO_LOG_NORMAL 3
#define SONAR_DISTRO_NORMAL 4
#define SONAR_DISTRO_BETA 5
#define SONAR_DISTRO_CONTINUOUS_BERNOULLI 6
#define SONAR_DISTRO_DIRICHLET 7
#define SONAR_DISTRO_FISHER_SNEDECOR 8
#define SONAR_DISTRO_GAMMA 9
#define SONAR_DISTRO_GUMBEL 10
#define SONAR_DISTRO_INVERSE_GAMMA 11
#define SONAR_DISTRO_KUMARASWAMY 12
#define SONAR_DISTRO_LAPLACIAN 13
#define SONAR_DISTRO_LKJCHOLESKY 14
#define SONAR_DISTRO_LRMVARIATE_NORMAL 15
#define SONAR_DISTRO_MVARIATE_NORMAL 16
#define SONAR_DISTRO_PARETO 17
#define SONAR_DISTRO_POISSON 18
#define SONAR_DISTRO_RELAXED_BERNOULLI 19
#define SONAR_DISTRO_RELAXED_ONEHOTCATEGORICAL 20
#define SONAR_DISTRO_STUDENTT 21
#define SONAR_DISTRO_UNIFORM 22
#define SONAR_DISTRO_VONMISES 23
#define SONAR_DISTRO_WEIBULL 24
#define SONAR_DISTRO_WISHART 25
#define SONAR_DISTRO_MAX_EVENT 16
#define SONAR_DISTRO_MAX_PROPOSALS 64
#define SONAR_DISTRO_DOMAIN 0x44495354u
typedef struct sonar_distro_params {
    int32_t family;
    int32_t k;
    int32_t row, col;
    float a, b, c;
    float v[SONAR_DISTRO_MAX_EVENT];
} sonar_distro_params;
int sonar_distro_fill_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset, const sonar_distro_params* p,
                          void* stream);
/* SonarNoiseImage (py/nodes/misc.py:158-357): noise composed into a ComfyUI IMAGE.  noise is NCHW ([batch][channels][plane], or
 * [batch][1][plane] with greyscale != 0: the one plane serves every channel), image and out are NHWC ([batch][plane][channels]).
 *  sonar_image_channel_mean_f32   out[b][p] = mean over c of noise[b][c][p] (channels added in order, true division): the greyscale fold
 *                                 (:340), written as a plane so that its extremes can be reduced (sonar_minmax_rows_f32)
 *  sonar_image_noise_compose_f32  per value, each step rounded on its own, in the reference's order (:341-352):
 *                                   n = noise; with noise_lo / noise_hi (per-sample extremes, [batch]; both NULL: skipped)
 *                                   n = clamp(((n - lo) / ((hi - lo) + eps)) * (noise_max - noise_min) + noise_min, noise_min, noise_max);
 *                                   n *= multiplier; v = image (0 when image is NULL: pure noise);
 *                                   bit c of channel_mask set: v = blend(v, n, blend_strength) (SONAR_BLEND_*, or SONAR_IMAGE_BLEND_ADD: v + n);
 *                                   clamp != 0: out = clip(v, 0, 1); clamp == 0: out = v, and the (min, max) of every block's values go to
 *                                   part_min / part_max ([batch][SONAR_IMAGE_NPART] each; slots no block owns are not written)
 *                                 image must not overlap out.  One lane owns one pixel for 3 and 4 channels; any other count (<= 64) takes a plain
 *                                 strided loop.
 *  sonar_image_rescale_f32        normalize_to_scale(image, 0, 1) per sample (:350), in place on the NHWC image, the extremes taken from the
 *                                 partial slots a clamp == 0 compose launch of the same (plane) wrote */
#define SONAR_IMAGE_BLEND_ADD 3
#define SONAR_IMAGE_NPART 1024
#define SONAR_IMAGE_MAX_CHANNELS 64
int sonar_image_channel_mean_f32(const float* noise, int64_t batch, int64_t channels, int64_t plane, float* out, void* stream);
int sonar_image_noise_compose_f32(const float* noise, const float* noise_lo, const float* noise_hi, double noise_min, double noise_max,
                                  float eps, float multiplier, int greyscale, int blend_mode, float blend_strength, uint64_t channel_mask,
                                  const float* image, float* out, int64_t batch, int64_t channels, int64_t plane, int clamp,
                                  float* part_min, float* part_max, void* stream);
int sonar_image_rescale_f32(float* image, int64_t batch, int64_t channels, int64_t plane, const float* part_min, const float* part_max,
                            float eps, void* stream);
/* Filter previews of SonarPowerNoise / SonarPowerFilterNoise (py/nodes/powernoise.py:268-294, 410-468): two or three panels side by side,
 * one launch per image, every roll / flip / concatenation done in the addressing.  Per plane: filter [H][W/2+1] (the normalised real
 * half-spectrum), kernel [H][W] (its irfft2, NOT rolled), noise [H][W] or NULL (then noise_h = noise_w = 0; with a plane they must be H, W).
 * out is [planes][H][FW + W (+ W with noise)]:
 *   columns 0 .. FW-1      tanh(filter_gain * F) * 256, F = rfft2_to_fft2(filter) (:457-468): with Wh = W/2+1 and L = Wh-2 (Wh odd) or
 *                          Wh-1 (Wh even), F[r][c] = filter[(r - H/2) mod H][c - L] for c >= L, and for c < L the mirror image
 *                          filter[(H-1 - r' - H/2) mod H][L - c], r' = (r-1) mod H for an even H, r for an odd one.  FW = L + Wh, which is
 *                          not always W (W = 6: 7 columns, W = 9: 8) -- the reference's widths
 *   the next W columns     (tanh(kernel_gain * k) + 1) * 128, k = kernel[(r - H/2) mod H][(c - W/2) mod W]
 *   the last W columns     (tanh(noise * (1/3)) + 1) * 128
 * each step rounded on its own.  sonar_preview_panels_f32 writes the values as fp32; with gain == 0 it writes F, the rolled kernel and the
 * noise as they are (data movement only), and may then be given kernel = NULL and no noise: out is [planes][H][FW], rfft2_to_fft2 itself.
 * sonar_preview_compose_u8 writes clamp(value, 0, 255) truncated to uint8.  H, W >= 2. */
int sonar_preview_panels_f32(const float* filter, const float* kernel, const float* noise, int64_t planes, int64_t H, int64_t W, int64_t noise_h,
                             int64_t noise_w, float filter_gain, float kernel_gain, int gain, float* out, void* stream);
int sonar_preview_compose_u8(const float* filter, const float* kernel, const float* noise, int64_t planes, int64_t H, int64_t W, int64_t noise_h,
                             int64_t noise_w, float filter_gain, float kernel_gain, uint8_t* out, void* stream);
/* RippleFilteredNoise, py/noise.py:1197-1200: x[i] *= table[(i / inner) % len] (a sin / cos gain profile along one dimension, or along
 * the flattened trailing dimensions with inner = 1); follow_sign: the result takes the sign of 1 - table[..] (torch.copysign). In place. */
int sonar_mul_table_f32(float* x, const float* table, int64_t n, int64_t inner, int64_t len, int follow_sign, void* stream);
/* LaplacianNoiseGenerator.generate, py/noise_generation.py:796-802: x = x/div_fac + Laplace(loc, scale), the variate built from a
 * uniform u in (eps-1, 1) the way torch.distributions.Laplace.rsample does: loc - scale*sign(u)*log1p(-max(|u|, tiny)).  In place. */
int sonar_laplace_add_f32(float* x, const float* u, float div_fac, float loc, float scale, int64_t n, void* stream);
/* ModulatedNoise (py/noise.py:784-866), three steps that never read a scalar back to the host:
 *  sonar_std_mid_f32   unbiased std over the middle axis of x[outer][mid][inner] -> stdv[outer][inner]
 *                      (torch.std(dim=-3, keepdim=True), :795-799; the other two modulation_dims use sonar_rowstats_f32)
 *  sonar_bcast_gain_f32  v = x*k*(1/(std*|strength|+1) + 1) (:800-803), std broadcast by `bcast`: 0 = stdv[outer],
 *                      1 = stdv[outer][mid], 2 = stdv[outer][inner]; `out` and/or `partials` may be NULL; each partial slot pair
 *                      holds (sum x^2, sum v^2) of its block (1024 pairs, same layout as the statistics kernels)
 *  sonar_ratio_mix_f32   out = a*(a_mul*rho) + x*x_mul, rho = sqrt(num_mul * sum num[2i] / sum den[2i+1]): the L2-norm ratio
 *                      "noise_norm / scaled_noise_norm" (:805-810, :860-866) taken from partial slots */
int sonar_std_mid_f32(const float* x, int64_t outer, int64_t mid, int64_t inner, float* stdv, void* stream);
int sonar_bcast_gain_f32(const float* x, const float* stdv, int64_t outer, int64_t mid, int64_t inner, int bcast,
                         float abs_strength, float k, float* out, double* partials, void* stream);
int sonar_ratio_mix_f32(const float* a, float a_mul, const float* x, float x_mul, const double* num_partials,
                        double num_mul, const double* den_partials, float* out, int64_t n, void* stream);
/* PowerLawNoiseGenerator, py/noise_generation.py:775-779: x = (use_sign ? sign(x) : x) * |x|^alpha, in place */
int sonar_powerlaw_f32(float* x, float alpha, int use_sign, int64_t n, void* stream);
/* x viewed as [outer, mid, inner]: amax over `mid` of x (use_abs 0) or |x| (use_abs 1) -> peak[outer, inner]
 * (torch.amax over one non-trailing dim, py/noise_generation.py:780-785) */
int sonar_amax_mid_f32(const float* x, int64_t outer, int64_t mid, int64_t inner, int use_abs, float* peak, void* stream);
/* x[o, m, i] /= d[o, i], in place, true division (same call site) */
int sonar_div_mid_f32(float* x, int64_t outer, int64_t mid, int64_t inner, const float* d, void* stream);
/* py/utils.py:452-470 normalize_to_scale: per row min/max rescale to [lo,hi] */
int sonar_minmax_rows_f32(const float* x, int64_t rows, int64_t inner, float* out_min, float* out_max, void* stream);
/* the rest of normalize_to_scale (py/utils.py:462-469): out = clamp(((x - lo[r]) / ((hi[r] - lo[r]) + eps)) * (target_max - target_min)
 * + target_min, target_min, target_max), one (lo, hi) per row, every step rounded separately as the reference's tensor ops are; the
 * targets arrive as doubles (Python floats in the reference): their difference is rounded to fp32 once */
int sonar_minmax_rescale_f32(const float* x, int64_t rows, int64_t inner, const float* lo, const float* hi, float eps,
                             double target_min, double target_max, float* out, void* stream);

/* ---------------------------------------------------------------- statistics over any subset of dimensions (csrc/group_stats.hip)
 * torch.mean / torch.std / amin / amax with dim = any tuple and keepdim = True (NormalizeToScaleNoise, py/noise.py:1287-1296;
 * normalize_to_scale, py/utils.py:452-470) on the contiguous tensor as it lies.  The caller collapses (shape, reduced dims) into
 * `nseg` <= SONAR_GROUP_MAX_SEGMENTS alternating segments s0.., outermost first (adjacent dimensions of one kind merged, size-1 dimensions
 * dropped; the sizes beyond nseg are ignored); segment k is reduced when (k odd) != first_reduced.  A group is one coordinate of the kept
 * segments, numbered row-major over them: the flattened keepdim layout.
 *  sonar_group_stats_f32           per group mean and unbiased std (one member: NaN, like torch) and / or min and max; the pair not wanted
 *                                  is NULL.  fp64 sums of x and x^2 as sonar_rowstats_f32; long reductions over few groups are split over
 *                                  workgroups, the parts left in `ws` and added in a fixed order by a second launch (same bits every run).
 *                                  ws: sonar_group_stats_ws_doubles(...) doubles (0: not split, ws may be NULL).
 *  sonar_group_affine_f32          sonar_row_affine_f32's operations with a[g], b[g] of the element's group; a NULL a is 0, a NULL b is 1
 *                                  (not both); out may be x
 *  sonar_group_minmax_rescale_f32  sonar_minmax_rescale_f32's arithmetic with lo[g], hi[g]; out may be x
 *  sonar_group_adjust_f32          NormalizeToScaleNoise's per-group scalars, n values: op 0 out = v * k; op 1 t = (v - 1) * k + 1,
 *                                  out = 1e-07 where t == 0 (NaN stays NaN); out may be v
 *  sonar_group_peak_f32            per group amax of x (use_abs 0) or |x| (use_abs 1), NaN where a member is NaN (torch.amax over any tuple of
 *                                  dims: PowerLawNoiseGenerator's div_max_dims, py/noise_generation.py:780-785).  Split like
 *                                  sonar_group_stats_f32; ws: sonar_group_stats_ws_doubles(..., 0, 1) doubles
 *  sonar_group_div_f32             x /= d[g] in place, a true division (a zero d gives torch's inf / NaN)
 *  sonar_group_divided_mean_f32    per group mean of x / d[g], every quotient rounded to fp32 and added in fp64 (the second statistic of
 *                                  sonar_scale_noise_rows_f32: py/utils.py:97-99).  ws: sonar_group_stats_ws_doubles(..., 1, 0) doubles
 *  sonar_group_scale_noise_f32     x = (x / sd[g] - mean[g]) * factor in place, each step rounded on its own: the last pass of
 *                                  sonar_scale_noise_rows_f32 with the operands of the element's group
 * SONAR_ERR_ARG: nseg outside 1..6, a negative size, a required pointer NULL, a result of sonar_group_stats_f32 (or ws) equal to x, an
 * operand table equal to out, a split shape without ws.  SONAR_ERR_UNSUPPORTED: 2^31 elements or more.  A size of 0 launches nothing. */
#define SONAR_GROUP_MAX_SEGMENTS 6
int64_t sonar_group_stats_ws_doubles(int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4, int64_t s5,
                                     int want_mean_std, int want_min_max);
int sonar_group_stats_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                          int64_t s5, float* mean, float* stdv, float* lo, float* hi, double* ws, void* stream);
int sonar_group_affine_f32(int op, const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                           int64_t s5, const float* a, const float* b, float* out, void* stream);
int sonar_group_minmax_rescale_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                   int64_t s5, const float* lo, const float* hi, float eps, double target_min, double target_max,
                                   float* out, void* stream);
int sonar_group_adjust_f32(int op, const float* v, int64_t n, float k, float* out, void* stream);
int sonar_group_peak_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                         int64_t s5, int use_abs, float* peak, double* ws, void* stream);
int sonar_group_div_f32(float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4, int64_t s5,
                        const float* d, void* stream);
int sonar_group_divided_mean_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                 int64_t s5, const float* d, float* mean, double* ws, void* stream);
int sonar_group_scale_noise_f32(float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                int64_t s5, const float* sd, const float* mean, float factor, void* stream);

/* ---------------------------------------------------------------- latent operations under CFG */
/* SonarApplyLatentOperationCFG (py/nodes/latent_operations.py:246-300): the arithmetic on either side of the latent operations, one launch
 * each.  x, t1, t2, t1_orig and out are n contiguous values of `dtype` (SONAR_DTYPE_*: widened to fp32 at load, `out` rounded once, to
 * nearest even); result, t2_out / t2 and sigma are fp32.  sigma (device, nullable): NULL = no prediction flip, else sigma_n = 1 value or one
 * per sample of `inner` consecutive elements (sigma_n = n / inner; inner must divide n and need not be a multiple of the vector width).
 * Every operation is rounded on its own, in the reference's order, and the division is a true division.
 *  sonar_cfg_op_prepare  f(t) = (x - t) / sigma[i / inner] with a flip, f(t) = t without;  t2_out = f(t2) (t2, t2_out nullable together);
 *                        result = f(t1) - f(t2), or f(t1) without t2.  x may be NULL without a flip.
 *  sonar_cfg_op_finish   r = result + t2 (t2 nullable: the buffer prepare wrote);  with a flip r = x - sigma[i / inner] * r;
 *                        out = blend(t1_orig, r, w) (SONAR_BLEND_*, evaluated as sonar_blend_f32 does) or out = r for SONAR_CFG_BLEND_NONE
 *                        (t1_orig may then be NULL).  out must not overlap an input.
 * 16-byte aligned buffers take 4 elements per lane and access; any other alignment takes the one-element route.
 * SONAR_ERR_ARG: n < 0, inner <= 0 or not a divisor of n, sigma_n neither 1 nor n / inner, an unknown dtype or blend mode, and for n > 0 a
 * required pointer NULL.  n == 0 launches nothing (and asks for no buffer: an empty tensor has none). */
#define SONAR_DTYPE_F32 0
#define SONAR_DTYPE_F16 1
#define SONAR_DTYPE_BF16 2
#define SONAR_CFG_BLEND_NONE (-1)
int sonar_cfg_op_prepare(int dtype, const void* x, const void* t1, const void* t2, const float* sigma, int64_t sigma_n, float* result,
                         float* t2_out, int64_t n, int64_t inner, void* stream);
int sonar_cfg_op_finish(int dtype, const float* result, const float* t2, const void* x, const float* sigma, int64_t sigma_n,
                        const void* t1_orig, int blend_mode, float w, void* out, int64_t n, int64_t inner, void* stream);

/* ---------------------------------------------------------------- SonarCustomNoiseParameters */
/* The tail of CustomNoiseParametersNoise (py/noise.py:2172-2185): fix_invalid, the crop back from a squared plane, the conversion to the
 * latent's dtype and scale_noise, as two launches without a host synchronisation.  src is `planes` planes of plane_in values of src_dtype
 * (SONAR_DTYPE_*), of which the first plane_out of each are kept; out is planes * plane_out values of dst_dtype.  Arithmetic is fp32,
 * statistics are fp64, the result is rounded once (to nearest even).
 *  sonar_noise_params_scan   one sweep over src -> partials ([SONAR_NOISE_PARAMS_NPART][SONAR_NOISE_PARAMS_SLOT] doubles; only the slots of
 *                            the launch's blocks are written, and the apply launch of the SAME src / planes / plane_in / plane_out /
 *                            fix_invalid reads exactly those).  fix_invalid != 0: finite maximum and minimum over ALL values (padding
 *                            included; two floats in one word), and over the kept values the sum and sum of squares of the finite ones
 *                            and the counts of +inf, -inf and NaN.  fix_invalid == 0: sum and sum of squares of the kept values as they are.
 *  sonar_noise_params_apply  per kept value, in this order: with fix_invalid NaN -> 0, +inf -> max(finite maximum, 0), -inf ->
 *                            min(finite minimum, 0) (nan_to_num_'s extremes are those of the tensor whose non-finite values are 0
 *                            already); with normalized the two thresholded corrections of scale_noise (mean and unbiased std of the
 *                            fixed, kept values, derived from the partials; the mean is subtracted as two floats, high part then low
 *                            part); * factor when factor != 1; written at p * plane_out + i.
 *                            partials may be NULL when both flags are 0 (a crop / conversion / multiply alone).  out must not be src.
 * Both plane lengths multiples of 4 and 16-byte aligned buffers: 4 values per lane and access; anything else: one value, per launch.
 * SONAR_ERR_ARG: an unknown dtype, planes < 0, plane_out <= 0 or > plane_in, more than 2^31 tiles, for planes > 0 a required pointer NULL.
 * planes == 0 launches nothing. */
#define SONAR_NOISE_PARAMS_NPART 1024
#define SONAR_NOISE_PARAMS_SLOT 6
int64_t sonar_noise_params_ws_doubles(void); /* doubles the partials buffer of the two entry points below must hold */
int sonar_noise_params_scan(int src_dtype, const void* src, int64_t planes, int64_t plane_in, int64_t plane_out, int fix_invalid,
                            double* partials, void* stream);
int sonar_noise_params_apply(int src_dtype, const void* src, int dst_dtype, void* out, int64_t planes, int64_t plane_in, int64_t plane_out,
                             int fix_invalid, int normalized, float factor, float threshold_std_devs, const double* partials, void* stream);

/* ---------------------------------------------------------------- ShuffledNoise */
/* utils.elementwise_shuffle_by_dim (py/utils.py:599-657): every row of a contiguous fp32 tensor of `ndim` <= 5 dimensions s0.. permuted
 * along dimension `dim` on its own, on the tensor as it lies (no transposed copy).  n = the size of `dim`, rows = the other sizes'
 * product, row r = the row-major position of the other dimensions: with inner = the product of the sizes behind `dim`, value j of row r
 * lies at ((r / inner) * n + j) * inner + r % inner -- the strides follow from the shape.  Every output value is an input value.
 *  sonar_shuffle_gather_f32    replay mode, the permutation from the host: out[r, j] = src[r, idx[r * n + j]] (idx_is_offset 0: an int32
 *                              table [rows][n], entries in [0, n) -- not checked) or out[r, j] = src[r, (j + idx[r]) % n] (idx_is_offset 1:
 *                              one int32 per row in [0, n); a negative entry copies the row).
 *  sonar_shuffle_generate_f32  generate mode, the permutation drawn in the kernel from (seed, stream_id, row_offset + r) -- the stream
 *                              contract is INTEGRATION.md 3b: row r is shuffled when prob >= 1 or its mask variate (stream_id) is below
 *                              prob and copied otherwise; with no_identity a shuffled row is rotated by an offset in [1, n) (stream_id + 1),
 *                              otherwise value j moves to the rank of its key among the row's n keys (stream_id + 2), ranked in LDS by
 *                              (key, j).  No table reaches memory.  Keys: n <= SONAR_SHUFFLE_MAX_N.
 * SONAR_ERR_ARG: a NULL pointer, out == src, ndim outside 1..5, dim outside [0, ndim), a negative size, n < 1 (n < 2 with offsets or
 * no_identity), more than 2^31 rows, prob NaN, row_offset < 0, row_offset + rows or stream_id + 2 not below 2^48.  SONAR_ERR_UNSUPPORTED:
 * keys with n > SONAR_SHUFFLE_MAX_N.  All checked before anything is launched; rows == 0 launches nothing. */
#define SONAR_SHUFFLE_MAX_N 4096
#define SONAR_SHUFFLE_DOMAIN 0x53484646u
int sonar_shuffle_gather_f32(const float* src, float* out, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4, int dim,
                             const int32_t* idx, int idx_is_offset, void* stream);
int sonar_shuffle_generate_f32(const float* src, float* out, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4, int dim,
                               float prob, int no_identity, uint64_t seed, uint64_t stream_id, int64_t row_offset, void* stream);

/* ---------------------------------------------------------------- CollatzNoiseGenerator */
/* One iteration of CollatzNoiseGenerator (py/noise_generation.py:2330-2615) over the view [outer][len][inner] of a contiguous fp32 latent
 * (not flattened: len = the size of `dim`, inner = the product of the sizes behind it; flattened: len = the product from `dim` on,
 * inner = 1).  cl = min(len, chain_length), n_chunks = ceil(len / cl), chains = outer * n_chunks * inner, len_p = n_chunks * cl.
 *  sonar_collatz_chain_f32  seeds [outer][n_chunks][inner] -> out [outer][len_p][inner].  Per chain: noise = seed * span + rmin (the scalars
 *                           rounded to fp32), an exact zero replaced by (*seed_ext * span + rmin) / chains -- seed_ext a device scalar, the
 *                           seed that gives the largest noise (the largest seed for span >= 0, else the smallest), so the value is
 *                           noise.max() / noise.numel() without a read on the host -- then the seed_mode parity fix and cl + chain_offset
 *                           links of the recurrence in registers.  Kept per link past chain_offset: result / noise (OUT_RATIOS), muls
 *                           (OUT_MULTS) or adds / noise (OUT_ADDS).  The shortcuts for even / odd multipliers of 1 and additions of 0 are
 *                           decided on the doubles as given.  Every step is one correctly rounded fp32 operation.
 *  sonar_collatz_mix_f32    acc[o][j][i] += (out1[o][j][i] * second) * scale for j < len (out1 in the padded layout); second is 1
 *                           (SECOND_ONE, `second` may be NULL), seeds[o][j / cl][i] (SECOND_SEEDS) or second[o][j][i] (SECOND_MIX).
 * SONAR_ERR_ARG: a NULL pointer, out == seeds (acc == an input), a negative size or one beyond 2^31, chain_length < 1, chain_offset < 0,
 * more than 2^31 chains, an unknown flag, mode or output.  All checked before anything is launched; an empty view launches nothing. */
#define SONAR_COLLATZ_INTEGER_MATH 1
#define SONAR_COLLATZ_BREAK_LOOPS 2
#define SONAR_COLLATZ_KEEP_SIGN 4
#define SONAR_COLLATZ_SEED_DEFAULT 0
#define SONAR_COLLATZ_SEED_FORCE_ODD 1
#define SONAR_COLLATZ_SEED_FORCE_EVEN 2
#define SONAR_COLLATZ_OUT_RATIOS 0
#define SONAR_COLLATZ_OUT_MULTS 1
#define SONAR_COLLATZ_OUT_ADDS 2
#define SONAR_COLLATZ_SECOND_ONE 0
#define SONAR_COLLATZ_SECOND_SEEDS 1
#define SONAR_COLLATZ_SECOND_MIX 2
int sonar_collatz_chain_f32(const float* seeds, const float* seed_ext, float* out, int64_t outer, int64_t len, int64_t inner,
                            int64_t chain_length, int64_t chain_offset, double span, double rmin, double emul, double eadd, double omul,
                            double oadd, int flags, int seed_mode, int output, void* stream);
int sonar_collatz_mix_f32(float* acc, const float* out1, const float* second, int second_mode, int64_t outer, int64_t len, int64_t inner,
                          int64_t chain_length, float scale, void* stream);

/* ---------------------------------------------------------------- VoronoiNoiseGenerator */
/* One octave of VoronoiNoiseGenerator.generate_octave (py/noise_generation.py:1847-1869) as one launch, accumulated into the output:
 * out[b][c][y][x] = out + result * amplitude, and with SONAR_VORONOI_FINAL_DIV the sum is then divided by final_div (the generator's
 * total amplitude).  fp [B][C][N][3] are the plane's feature points in [0, 1]; the grid (y / H, x / W, z_norm), the two `(v * scale) % 1`
 * and the toroidal difference d = (g - f + 0.5) % 1 - 0.5 are the reference's own fp32 operations, one rounding each, `%` as
 * torch.remainder.  One thread per pixel, a workgroup inside one (b, c) plane, the plane's points staged through LDS
 * SONAR_VORONOI_CHUNK at a time; per pixel one pass over the points keeps the four smallest distances and the index of the smallest
 * (and the online-softmax sums of `softmin`) in registers.
 * The program is the parsed distance_mode / result_mode of the octave (the host flattens the strings):
 *   distance = sum over n_d terms of metric(xform_k(... xform_1(d))) * scale; a transform is WEIGHT (d * (a, b, c)) or FRACTAL_SIN /
 *              FRACTAL_COS (d + a * fun(d * b)); the metrics are the reference's (MANHATTEN is its euclidean), ANGLE* read component idx
 *              of F.normalize(d) (eps 1e-12).
 *   result   = sum over n_r terms of ridge_k(... ridge_1(op(e))) * scale with e = fn_k(... fn_1(distance)), fn = a * fun(distance * b)
 *              (the result fractal_norm: the selection runs on e), ridge = 1 - a * v.  Ops: F (the idx1-th smallest), INV_F
 *              (1 / (F + eps)), DIFF (F[idx2] - F[idx1]), DIFF2 ((v2 - v1) / (v2 + v1 + 1e-6)), SOFTMIN (sum e * softmax(-|d| * temperature)),
 *              CELLID (index of the smallest / aux[term] + 1, aux a device array of SONAR_VORONOI_MAX_TERMS floats: the whole tensor's
 *              largest index, reduced from a CELLID_RAW pass) and CELLID_RAW (the index of the smallest as a float).
 * SONAR_ERR_ARG: a NULL pointer (aux only with a CELLID term), out == fp, a negative size, a size of 2^31 or more, N < 2 (with pixels to
 * compute), a term count outside 1..SONAR_VORONOI_MAX_TERMS, a chain longer than SONAR_VORONOI_MAX_CHAIN, an unknown metric, transform, op
 * or flag, idx outside its range.  SONAR_ERR_UNSUPPORTED: N > SONAR_VORONOI_MAX_POINTS.  All checked before anything touches the HIP
 * runtime; an empty output launches nothing. */
#define SONAR_VORONOI_MAX_TERMS 4
#define SONAR_VORONOI_MAX_CHAIN 4
#define SONAR_VORONOI_MAX_POINTS 4096
#define SONAR_VORONOI_CHUNK 256
#define SONAR_VORONOI_FINAL_DIV 1
#define SONAR_VORONOI_D_EUCLIDEAN 0
#define SONAR_VORONOI_D_MANHATTEN 1
#define SONAR_VORONOI_D_CHEBYSHEV 2
#define SONAR_VORONOI_D_MINKOWSKI 3
#define SONAR_VORONOI_D_QUADRATIC 4
#define SONAR_VORONOI_D_ANGLE 5
#define SONAR_VORONOI_D_ANGLE_TANH 6
#define SONAR_VORONOI_D_ANGLE_SIGMOID 7
#define SONAR_VORONOI_X_WEIGHT 0
#define SONAR_VORONOI_X_FRACTAL_SIN 1
#define SONAR_VORONOI_X_FRACTAL_COS 2
#define SONAR_VORONOI_R_F 0
#define SONAR_VORONOI_R_INV_F 1
#define SONAR_VORONOI_R_DIFF 2
#define SONAR_VORONOI_R_DIFF2 3
#define SONAR_VORONOI_R_SOFTMIN 4
#define SONAR_VORONOI_R_CELLID 5
#define SONAR_VORONOI_R_CELLID_RAW 6
#define SONAR_VORONOI_R_SOFTMIN_SORTED 7 /* sonar_voronoi_rank_octave_f32 only */
#define SONAR_VORONOI_RANK_ROW_N 256     /* the longest row SOFTMIN_SORTED is built for: 64 lanes' rows and the staged points in LDS */
typedef struct sonar_voronoi_dterm {
    int32_t metric, idx, n_xform;
    int32_t xform[SONAR_VORONOI_MAX_CHAIN];
    float xa[SONAR_VORONOI_MAX_CHAIN], xb[SONAR_VORONOI_MAX_CHAIN], xc[SONAR_VORONOI_MAX_CHAIN];
    float p, inv_p /* minkowski: p and 1 / p, the latter formed in double */, scale;
} sonar_voronoi_dterm;
typedef struct sonar_voronoi_rterm {
    int32_t op, idx1, idx2, n_fn, n_ridge;
    int32_t fn[SONAR_VORONOI_MAX_CHAIN] /* SONAR_VORONOI_X_FRACTAL_SIN / _COS */;
    float fa[SONAR_VORONOI_MAX_CHAIN], fb[SONAR_VORONOI_MAX_CHAIN];
    float ridge[SONAR_VORONOI_MAX_CHAIN] /* innermost first */;
    float eps, temperature, scale;
} sonar_voronoi_rterm;
typedef struct sonar_voronoi_program {
    int32_t n_d, n_r;
    sonar_voronoi_dterm d[SONAR_VORONOI_MAX_TERMS];
    sonar_voronoi_rterm r[SONAR_VORONOI_MAX_TERMS];
} sonar_voronoi_program;
int sonar_voronoi_octave_f32(const float* fp, float* out, const float* aux, int64_t B, int64_t C, int64_t H, int64_t W, int64_t N,
                             float scale, float z_norm, float amplitude, float final_div, int flags, const sonar_voronoi_program* prog,
                             void* stream);

/* The fuzz distance mode (py/noise_generation.py:1586-1603) as three launches of the octave kernel; distance term `fuzz_term` of the
 * program is the fuzzed one, its chain and metric the inner mode.  `stats` is a device array of 2 + 2 B C H words holding floats as
 * unsigned integers of the same order (a negative float's bits inverted, a positive one's sign bit set): [0] / [1] the minimum / maximum
 * of the inner distance over the whole tensor, [2 + 2 r] / [3 + 2 r] those of the fuzzed distance over (W, N) of row r = (b C + c) H + y;
 * the caller fills the minimum slots with 0xFFFFFFFF and the maximum slots with 0 before pass 0.
 *   pass 0  reduces the inner distance into stats[0..1] (rmin, rmax = result.aminmax()); writes nothing else, out may be NULL
 *   pass 1  reduces inner + (u * 2 f - f), f = max(|rmin|, |rmax|) * fuzz formed in double from the device values, into the row slots
 *           (normalize_to_scale(dim=(-2, -1)) on [B, C, H, W, N] groups over (W, N)); out may be NULL
 *   pass 2  the real pass: the fuzzed distance rescaled with sonar_minmax_rescale_f32's device function between its row's extremes to
 *           [rmin, rmax] (eps 1e-7), then the term's scale, the other terms, the selection and the result as in sonar_voronoi_octave_f32
 * No value is read on the host and no [B, C, H, W, N] tensor is written.  The uniforms: `u` [B][C][H][W][N] when given (replay mode),
 * else the element elem_offset + flat index of the stream (seed, stream_id) that sonar_philox_uniform_f32 fills -- the same values
 * hip_lib.philox_uniform gives for that shape, so all three passes see one draw.
 * SONAR_ERR_ARG beyond sonar_voronoi_octave_f32's: NULL stats, stats or u equal to another buffer, pass outside 0..2, fuzz_term outside
 * the program's distance terms, fuzz NaN, elem_offset or stream_id outside [0, 2^48). */
int sonar_voronoi_fuzz_octave_f32(const float* fp, float* out, const float* aux, const float* u, uint32_t* stats, int64_t B, int64_t C,
                                  int64_t H, int64_t W, int64_t N, float scale, float z_norm, float amplitude, float final_div, int flags,
                                  const sonar_voronoi_program* prog, int pass, int fuzz_term, double fuzz, uint64_t seed, uint64_t stream_id,
                                  int64_t elem_offset, void* stream);

/* The rank route: the same octave with idx1 / idx2 anywhere in [0, N) -- `f:idx=k` past f4, the median (the host passes rank
 * (N - 1) / 2, torch.median's lower middle) -- and SOFTMIN_SORTED (softmin:use_sorted: the weight of point j multiplies the j-th smallest
 * value).  The k-th smallest value of a pixel's row is found exactly, bit by bit on the floats' ordered-integer image: 32 sweeps over the
 * points that count, for both ranks of every term at once, the values below the candidate; one more sweep in front serves SOFTMIN,
 * SOFTMIN_SORTED and the CELLID ops.  With ranks inside 0..3 the output has sonar_voronoi_octave_f32's bits.  SOFTMIN_SORTED runs in
 * workgroups of one wave that hold each pixel's row in LDS (N <= SONAR_VORONOI_RANK_ROW_N) and ranks every value in it.
 * fuzz_term -1: no fuzz distance term (u and stats NULL); else the arguments of sonar_voronoi_fuzz_octave_f32's pass 2, after its passes
 * 0 and 1 have filled `stats`.
 * Every term is a value here: the write-through of the reference's bare `f` views into the sorted row their sum shares is restated by
 * sonar_voronoi_octave_f32 alone, and the host keeps such sums there (the median is no view).
 * SONAR_ERR_ARG beyond the entry points' above: a rank below 0 or not below N, u or stats without a fuzz term.  SONAR_ERR_UNSUPPORTED:
 * SOFTMIN_SORTED with N > SONAR_VORONOI_RANK_ROW_N. */
int sonar_voronoi_rank_octave_f32(const float* fp, float* out, const float* aux, const float* u, uint32_t* stats, int64_t B, int64_t C,
                                  int64_t H, int64_t W, int64_t N, float scale, float z_norm, float amplitude, float final_div, int flags,
                                  const sonar_voronoi_program* prog, int fuzz_term, double fuzz, uint64_t seed, uint64_t stream_id,
                                  int64_t elem_offset, void* stream);

/* The result modes that work on whole planes of inner results (each inner term one sonar_voronoi_octave_f32 launch into a temporary):
 *  sonar_voronoi_gradient_f32  gradient_magnitude with replicate padding (clamped indices): acc[p][y][x] += sqrt(dx^2 + dy^2) * scale,
 *                              dx = r1[y][x + 1] - r2[y][x - 1], dy = r1[y + 1][x] - r2[y - 1][x]; r2 may be r1.
 *  sonar_voronoi_fuzz_add_f32  the result fuzz's x += u * twice_fuzz - fuzz, each step rounded (the rescale around it is the existing
 *                              min / max reduction and sonar_minmax_rescale_f32).
 *  sonar_voronoi_acc_f32       acc = acc + x * scale, then / final_div with SONAR_VORONOI_FINAL_DIV.
 * SONAR_ERR_ARG: a NULL pointer, an output equal to an input, a negative size, 2^31 values or more, an unknown flag; a size of 0 launches
 * nothing. */
int sonar_voronoi_gradient_f32(const float* r1, const float* r2, float* acc, int64_t planes, int64_t H, int64_t W, float scale, void* stream);
int sonar_voronoi_fuzz_add_f32(float* x, const float* u, int64_t n, float twice_fuzz, float fuzz, void* stream);
int sonar_voronoi_acc_f32(float* acc, const float* x, int64_t n, float scale, float final_div, int flags, void* stream);

/* ---------------------------------------------------------------- PatternBreakNoise */
/* utils.pattern_break (py/utils.py:575-596) on a contiguous fp32 tensor of n values, out != x:
 *   v = clamp(((x - lo) / ((hi - lo) + 1e-7)) * 2 - 1, -1, 1)           lo, hi = min, max of x (a NaN never wins)
 *   a = 2 * (fmod(|v| * 1e6, 11) / 11) - 1                              every step one fp32 rounding, fmod exact
 *   result = clamp(((detail_scale * erfinv(a)) * sqrt(2)) * 0.2, -1, 1) erfinv(-1) = -inf reaches the clamp; NaN stays NaN
 *   restore_scale: result = clamp(((result - rlo) / ((rhi - rlo) + 1e-7)) * (hi - lo) + lo, lo, hi), rlo, rhi = min, max of result,
 *                  hi - lo formed in double and rounded once (the reference takes them through .item())
 *   out = blend(blend_mode, x, result, percentage)                      SONAR_BLEND_*
 * detail_scale is 1 + detail_level / 10, formed in double by the caller.  Nothing is read on the host.  `route` SONAR_PATTERN_BREAK_THREE:
 * three launches (extremes of x; extremes of the result, only with restore_scale; apply) through (lo, hi) partials in `ws`;
 * SONAR_PATTERN_BREAK_ONE: one workgroup runs the three phases in one launch; SONAR_PATTERN_BREAK_AUTO: ONE up to
 * SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX values (sonar_pattern_break_route(n) tells which).  Both routes give the same bits in `out`.
 * ws: SONAR_PATTERN_BREAK_WS floats (ws_floats says how many there are).  stats (nullable): SONAR_NPART (sum, sumsq) pairs of `out`, as
 * sonar_stats_f32 writes them (the summation order depends on the route).
 * SONAR_ERR_ARG: x, out or ws NULL, a pointer not aligned to its element, out == x, ws == x or out, n <= 0, an unknown blend mode or route,
 * ws_floats < SONAR_PATTERN_BREAK_WS.  All checked before anything touches the HIP runtime. */
#define SONAR_PATTERN_BREAK_NPART 512
#define SONAR_PATTERN_BREAK_WS (4 * SONAR_PATTERN_BREAK_NPART)
#define SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX 4096
#define SONAR_PATTERN_BREAK_AUTO 0
#define SONAR_PATTERN_BREAK_ONE 1
#define SONAR_PATTERN_BREAK_THREE 2
int sonar_pattern_break_route(int64_t n);
int sonar_pattern_break_f32(const float* x, float* out, int64_t n, float detail_scale, float percentage, int blend_mode, int restore_scale,
                            int route, float* ws, int64_t ws_floats, double* stats, void* stream);

/* A pending global normalisation of a noise tensor (py/utils.py:100-105): the decision scale_noise(normalized=True) would take,
 * computed ON THE DEVICE from the tensor's (sum, sumsq) partials and left in device memory, so that the kernel that consumes the
 * noise (the sampler-step kernels below take it as `noise_norm`, nullable) applies `((v - mean) / std) * factor` -- only the parts
 * the thresholds ask for, in scale_noise's own order: same bits -- while it reads the noise, instead of a separate read + write of
 * the tensor.  sonar_apply_norm_f32 materialises it in place for any other consumer. */
typedef struct sonar_noise_norm {
    float mean, stdv, inv_std /* correctly rounded 1 / stdv */, factor;
    int32_t do_sub, do_div;
} sonar_noise_norm;
int sonar_norm_decision_f32(const double* partials, int64_t npart, int64_t n_total, float factor, float threshold_std_devs,
                            sonar_noise_norm* out /* device */, void* stream);
int sonar_apply_norm_f32(float* x, int64_t n, const sonar_noise_norm* norm /* device */, void* stream);

/* ---------------------------------------------------------------- momentum step (rows M, M2) */
typedef struct sonar_momentum_cfg {
    float momentum;      /* SonarConfig.momentum             py/sonar.py:47 */
    float hist_ratio;    /* history_ratios[0] = momentum_hist py/sonar.py:208-219 */
    float hist_scale;    /* history_ratios[1] */
    float md_scale;      /* history_ratios[2] = direction */
    int32_t mode;        /* SONAR_MODE_* */
    int32_t momentum_blend; /* SONAR_BLEND_* for momentum_mix  py/sonar.py:256-260 */
    int32_t history_blend;  /* SONAR_BLEND_* for update_hist   py/sonar.py:231-236 */
    int32_t use_momentum;   /* check_step(step)                py/sonar.py:221-225 */
    int32_t update_hist;    /* momentum_hist != 1 && check_step(step, is_history=True) */
    int32_t init_kind;      /* SONAR_INIT_* (applies only when h_in == NULL) */
    int32_t h_in_fresh;     /* 1: h_in was created by RAND init in this very step -> not used by the
                               denoised-mix of this step (py/sonar.py:273-283 reads hd before init) */
    int32_t reserved;
} sonar_momentum_cfg;

/* One Sonar Euler step, fused (py/sonar.py:262-320): x_out = momentum_d*(sigma_down-sigma) + x and
 * the twice-updated history.  h_in may be NULL (no history yet); h_out must be valid whenever the
 * step can create/update history; *h_out_present (host int, may be NULL) tells whether h_out holds
 * a history afterwards.  noise (nullable) adds noise*noise_scale (ancestral, py/sonar.py:563-566).
 * x_out may alias x; h_out may alias h_in. */
int sonar_momentum_euler_f32(const float* x, const float* denoised, const float* h_in, float* x_out,
                             float* h_out, const float* noise, float noise_scale, float sigma, float dt,
                             const sonar_momentum_cfg* cfg, int64_t n, int* h_out_present, const sonar_noise_norm* noise_norm,
                             void* stream);

/* DPM-Solver++(SDE) half steps, py/sonar.py:649-735.  Stage 1:
 *   md1 = MD(den, sigma); m_d = D(expm1_a * md1); x2 = ratio_a*x - m_d + noise*noise_scale
 * Stage 2 (den2 = model(x2, sigma_s)):
 *   md2 = MD(den2, sigma_s); dd = (1-fac)*md1 + fac*md2; m_d = D(expm1_b * dd);
 *   x_out = ratio_b*x - m_d (+ noise*noise_scale when noise != NULL)
 * `adj_is_one` reproduces the `adjusted_momentum == 1` early-out of get_momentum_d while the
 * blend weight stays cfg->momentum (py/sonar.py:298-303). */
int sonar_dpmpp_stage1_f32(const float* x, const float* denoised, const float* h_in, float* x2_out, float* md1_out,
                           float* h_out, const float* noise, float noise_scale, float sigma, float expm1_a,
                           float ratio_a, int adj_is_one, const sonar_momentum_cfg* cfg, int64_t n,
                           int* h_out_present, const sonar_noise_norm* noise_norm, void* stream);
int sonar_dpmpp_stage2_f32(const float* x, const float* denoised2, const float* md1, const float* h_in,
                           float* x_out, float* dd_out, float* h_out, const float* noise, float noise_scale,
                           float sigma_s, float expm1_b, float ratio_b, float fac, int adj_is_one,
                           const sonar_momentum_cfg* cfg, int64_t n, int* h_out_present, const sonar_noise_norm* noise_norm,
                           void* stream);

/* ---------------------------------------------------------------- base generators (rows G1, G2) */
/* On-device counter RNG.  Philox4x32-10 (key = seed) seeds one xoshiro128++ burst per (stream id, tile, lane);
 * a flat buffer is drawn in tiles of 4096 elements, so the value of element e depends only on
 * (seed, stream_id, elem_offset + e) -> independent of how a batch is sharded over GPUs. */
int sonar_philox_normal_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                            double* partials /*nullable*/, void* stream);
/* out = (u - sub)*mul + add, u~U[0,1)  (py/noise_generation.py:508-514) */
int sonar_philox_uniform_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                             float sub, float mul, float add, double* partials /*nullable*/, void* stream);
/* The same draws followed by scale_noise(factor, normalized = 1) with the tensor written ONCE: a statistics pass re-draws the
 * values without storing them, the final pass re-draws, normalises and stores (uniform = 0: N(0,1); 1: (U[0,1) - sub)*mul + add).
 * N(0,1) with factor 1 passes both thresholds 98.7 % of the time: that case stores the draws with their statistics in one pass and
 * lets sonar_scale_noise_f32 decide on the device (it returns without touching the tensor when there is nothing to do).
 * partials: 1024 fp64 pairs of workspace. */
int sonar_philox_noise_f32(int uniform, float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                           float sub, float mul, float add, float factor, float threshold_std_devs, double* partials,
                           void* stream);
/* The same call in a sampler's steady state, for prepared plans (round 6): ONE launch runs this call's final pass (statistics in
 * `partials`: left there by the previous call's launch when `have_stats`, else computed first by the ordinary statistics pass) and the
 * statistics pass of the call that will draw with `next_stream_id`, into `partials_next` (another 1024 fp64 pairs) -- the final pass is
 * store-bound, the statistics pass pure vector-ALU work, one wave does both for its tiles.  Output bits and `partials_next` are those of
 * sonar_philox_noise_f32 (N(0,1) with factor 1 included: with the decision known before the first store the raw draws go out as they
 * are 98.7 % of the time, and otherwise with scale_noise's own subtract / divide sequence -- no second launch either way).
 * sonar_philox_noise_ahead_ok(): whether the form pays for the shape -- n > 0, and for N(0,1) with factor 1 (whose ordinary route draws
 * every value once) only up to 8 Mi elements, where the call is launch-bound; the entry point itself takes every shape. */
int sonar_philox_noise_ahead_ok(int uniform, int64_t n, float factor);
int sonar_philox_noise_ahead_f32(int uniform, float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                 float sub, float mul, float add, float factor, float threshold_std_devs, double* partials,
                                 int have_stats, uint64_t next_stream_id, double* partials_next, void* stream);
/* `rows` independent latents of `inner` contiguous elements from ONE launch (csrc/noise_rows.hip; the batch_index form of
 * CustomNOISE.generate_noise).  Row r is, bit for bit, what a call on a 16-byte aligned tensor of its own gives:
 *   sonar_philox_normal_f32 / sonar_philox_uniform_f32(x_r, inner, row_seed[r], stream_id + row_stream[r], 0, partials_r), then
 *   SONAR_ROWS_NORM_NONE         x_r *= factor (skipped for a factor of exactly 1)
 *   SONAR_ROWS_NORM_SCALE_NOISE  sonar_scale_noise_f32(x_r, inner, factor, 1, threshold_std_devs, partials_r, SONAR_NPART, inner)
 *   SONAR_ROWS_NORM_FUSED        the final pass of sonar_philox_noise_f32's two-pass route (uniform draws, and normal draws with a factor
 *                                other than 1): the same statistics and decision, the quotient as a multiply by 1 / std
 * -- mean, unbiased std and both thresholds (threshold_std_devs / sqrt(inner)) are the row's own, from the fp64 (sum, sumsq) partials in the
 * order the per-call fill reduces `inner` elements.  row_seed, row_stream: DEVICE arrays of `rows` values; row_stream may be NULL (every row
 * draws with stream_id).  sub, mul, add: sonar_philox_uniform_f32's affine map, ignored for normal draws.  One workgroup per row, no
 * workspace, no atomics.
 * SONAR_ERR_UNSUPPORTED, nothing launched: rows < 0, inner <= 0, inner > sonar_philox_rows_max_inner() (SONAR_NPART * 4 tiles of 4096),
 * row_seed NULL with rows > 0.  SONAR_ERR_ARG: an unknown normalisation, out NULL or not aligned to a float.  rows == 0: success, nothing
 * launched. */
#define SONAR_ROWS_NORM_NONE 0
#define SONAR_ROWS_NORM_SCALE_NOISE 1
#define SONAR_ROWS_NORM_FUSED 2
int64_t sonar_philox_rows_max_inner(void);
int sonar_philox_rows_f32(float* out, int64_t rows, int64_t inner, const uint64_t* row_seed, const uint64_t* row_stream /*nullable*/,
                          int uniform, uint64_t stream_id, float sub, float mul, float add, float factor, int normalized,
                          float threshold_std_devs, void* stream);
/* The same for generate-mode Perlin noise: `rows` latents of C * H * W elements, every row with its OWN lattice.  Row r is, bit for bit,
 * what these calls give on 16-byte aligned tensors of their own, with s_r = stream_id + row_stream[r]:
 *   sonar_perlin_lattice_f32(terms_r, iters, C, H, W, blend_mode, row_seed[r], s_r + 1), then
 *   SONAR_ROWS_NORM_NONE   sonar_perlin_generate_f32(terms_r, x_r, 1, C * H * W, 1, div_fac, row_seed[r], s_r, 0, ...), x_r *= factor (skipped
 *                          for a factor of exactly 1)
 *   SONAR_ROWS_NORM_FUSED  sonar_perlin_noise_f32(terms_r, x_r, 1, C * H * W, 1, div_fac, row_seed[r], s_r, 0, factor, threshold_std_devs, ...)
 * -- the launch route (scalar, vector, fast, tile-aligned), the word-to-value converter and the order of the (sum, sumsq) partials are
 * those of a batch of ONE latent of C * H * W elements, whatever the address of the row inside `out`.  lattice: workspace of rows * C * H * W
 * floats, 16-byte aligned; row r's summed lattice is left in its slice.  One workgroup per row, no atomics.
 * SONAR_ERR_UNSUPPORTED, nothing launched: rows < 0, H or W >= 2^20, C * H * W > sonar_philox_rows_max_inner(), row_seed NULL with rows > 0.
 * SONAR_ERR_ARG: C, H or W <= 0, iters < 0 or >= 2^20, an unknown blend mode, a normalisation other than the two above, out NULL or not
 * aligned to a float, lattice NULL or not 16-byte aligned, lattice == out.  rows == 0: success, nothing launched. */
int sonar_perlin_rows_f32(float* out, float* lattice, int64_t rows, int64_t C, int64_t H, int64_t W, int64_t iters, int blend_mode,
                          float div_fac, const uint64_t* row_seed, const uint64_t* row_stream /*nullable*/, uint64_t stream_id,
                          float factor, int normalized, float threshold_std_devs, void* stream);

/* Brownian-interval noise (the reference wraps ComfyUI's BrownianTreeNoiseSampler -> torchsde, un-vendored:
 * py/noise_generation.py:262-286, py/nodes/powernoise.py:383-393).  out[e] = sum_k coefs[k] * z(node_ids[k], e) with
 * z a counter-based N(0,1) keyed by (seed, node id (48 bits), global element index elem_offset + e).  node_ids / coefs are
 * HOST arrays (<= 96 entries): the expansion of the queried increment / point over the node normals, kept by the host in fp64
 * (each queried time is a Brownian bridge between the nearest times known before it).  latent_elems =
 * elements per latent (0 if unknown): when it is a multiple of 4096, there is one seed and the call covers whole latents, z(node, .)
 * is a node burst: per 1024-element sub-tile and lane ONE base state rng_stream(seed, 0xB0B000000001, sub-tile, lane), per node a
 * multiply-with-carry burst seeded with fmix32(base.x ^ hx), fmix32(base.c ^ hc), (hx, hc) = splitmix64(node id), 12 words per lane
 * (23 radius bits, 16 angle bits per value); otherwise one Philox4x32-10 block per 4 values (counter (element / 4, node id), key seed).
 * The family never depends on buffer alignment (4-byte-aligned buffers take the same values).  latent_seeds (device, nullable): one
 * seed per latent (the sampler's batched-seed mode), replacing `seed` (always the Philox family). */
int sonar_brownian_f32(float* out, int64_t n, int64_t elem_offset, const uint64_t* node_ids, const float* coefs, int nnodes,
                       uint64_t seed, const uint64_t* latent_seeds, int64_t latent_elems, void* stream);
/* One path point instead of an increment: W = sum_k coefs[k] z(node_ids[k], e) with the coefficients of W(t) itself;
 * w_out = W (nullable) and out = scale * (W - prev) (out, prev nullable; prev = a W(t') kept from an earlier call). */
int sonar_brownian_point_f32(float* out, float* w_out, const float* prev, float scale, int64_t n, int64_t elem_offset,
                             const uint64_t* node_ids, const float* coefs, int nnodes, uint64_t seed,
                             const uint64_t* latent_seeds, int64_t latent_elems, void* stream);
/* The bridge form of a path point: W = fa * base_a + fb * base_b + sum_k coefs[k] z(node_ids[k], e), base_a / base_b (nullable) =
 * the cached W tensors of the two times the new one was bridged between -- ONE fresh normal per element instead of the point's
 * whole expansion.  Also accumulates an expansion longer than 96 terms in chunks (base_a = the partial sum, fa = 1). */
int sonar_brownian_bridge_f32(float* out, float* w_out, const float* prev, float scale, const float* base_a, float fa,
                              const float* base_b, float fb, int64_t n, int64_t elem_offset, const uint64_t* node_ids,
                              const float* coefs, int nnodes, uint64_t seed, const uint64_t* latent_seeds, int64_t latent_elems,
                              double* partials /* nullable: (sum, sumsq) of `out`, SONAR_NPART pairs */, void* stream);
/* Two points of the same path from one launch, both differenced against the same kept W (DPM++ SDE asks (t, s) and (t, t') per step):
 *   W_i = fa_i * base_a_i + fb_i * base_b_i + sum over point i's nodes of coef * z(node, e),   out_i = scale_i * (W_i - prev),
 * w_out_i = W_i (nullable).  Point i's nodes are the shared list (ONE coefficient, the same for both points) and its private list; a
 * node may be on both private lists with a coefficient each.  Every list has strictly ascending 48-bit ids, the shared list is disjoint
 * from the private ones.  z(node, .) is drawn once per node whichever points hold it, and each W_i is accumulated in ascending id order:
 * out_i, w_out_i and partials_i are bit for bit what sonar_brownian_bridge_f32 gives for point i alone (same routes, same value
 * families).  SONAR_ERR_ARG before any launch: a NULL output, two outputs sharing a buffer, an output aliasing a base or prev, n < 0 or
 * n >= 2^31, an unsorted list.  SONAR_ERR_UNSUPPORTED (make two single-point queries): more than 96 terms over the three lists;
 * statistics asked for while one expansion has fewer than 4 terms and the other has not (the single-point launches would differ in
 * block size, and with it in the statistics' summation order). */
int sonar_brownian_pair_f32(float* out_1, float* out_2, float* w_out_1, float* w_out_2, const float* prev, float scale_1, float scale_2,
                            const float* base_a_1, float fa_1, const float* base_b_1, float fb_1, const float* base_a_2, float fa_2,
                            const float* base_b_2, float fb_2, int64_t n, int64_t elem_offset, const uint64_t* shared_ids,
                            const float* shared_coefs, int nshared, const uint64_t* ids_1, const float* coefs_1, int n_1,
                            const uint64_t* ids_2, const float* coefs_2, int n_2, uint64_t seed, const uint64_t* latent_seeds,
                            int64_t latent_elems, double* partials_1, double* partials_2, void* stream);

/* Accumulating forms of the generators (noise chains: result = sum_i item_i * factor_i, py/noise.py:188-194).  Instead of writing
 * a fresh tensor that sonar_axpby_f32 then folds into the running sum (read 8N + write 4N more), the generator reads the sum and
 * writes it back: y <- y * y_mul + x * x_mul with x the values the plain form would have stored (products rounded separately and
 * skipped for a multiplier of exactly 1: bit-identical to plain form + sonar_axpby_f32).  partials (nullable, SONAR_NPART pairs)
 * receives (sum, sumsq) of the new y, which is what a following scale_noise needs. */
typedef struct sonar_accumulate {
    float* y;         /* running sum, updated in place */
    float y_mul;
    float x_mul;
    double* partials; /* nullable */
} sonar_accumulate;
int sonar_philox_normal_acc_f32(const sonar_accumulate* acc, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                void* stream);
int sonar_perlin_generate_acc_f32(const sonar_accumulate* acc, const float* terms, int64_t B, int64_t chw, int64_t iters, float div_fac,
                                  uint64_t seed, uint64_t stream_id, int64_t elem_offset, void* stream);
int sonar_brownian_bridge_acc_f32(const sonar_accumulate* acc, float* w_out, const float* prev, float scale, const float* base_a, float fa,
                                  const float* base_b, float fb, int64_t n, int64_t elem_offset, const uint64_t* node_ids,
                                  const float* coefs, int nnodes, uint64_t seed, const uint64_t* latent_seeds, int64_t latent_elems,
                                  void* stream);
/* Two chain items in ONE pass over the running sum (py/noise.py:188-194 with a Gaussian or Perlin item followed by a Brownian one):
 * `pre` describes the fold the PREVIOUS item would have made with its own entry point (kind NORMAL: sonar_philox_normal_acc_f32 with
 * that seed / stream_id; kind PERLIN: sonar_perlin_generate_acc_f32 with iters == 1, that summed lattice, chw == latent_elems); the
 * Brownian kernel evaluates it per element, applies y1 = y * pre.y_mul + x * pre.x_mul and then its own fold on y1 -- the same
 * operations as the two launches, so the same bits, with one read + write of the sum instead of two.  Requires the tile route of the
 * Brownian kernel (one seed, latents of whole 4096-element tiles, 16-byte aligned tensors; the two items share elem_offset):
 * SONAR_ERR_UNSUPPORTED otherwise, and the caller applies `pre` with its own entry point first. */
#define SONAR_PREFIX_NORMAL 1
#define SONAR_PREFIX_PERLIN 2
typedef struct sonar_fold_prefix {
    int32_t kind;
    float y_mul;      /* y1 = y * y_mul + x * x_mul */
    float x_mul;
    float div_fac;    /* PERLIN */
    uint64_t seed;
    uint64_t stream_id;
    const float* terms; /* PERLIN: the summed lattice [chw] */
    int64_t chw;        /* PERLIN */
    int32_t fresh;      /* 1: the item is the chain's FIRST -- the sum holds nothing yet, y1 = x (y is not read; x_mul must be 1 and the
                           hosting fold's y_mul carries the item's factor, as sonar_axpby_f32 would) */
} sonar_fold_prefix;
int sonar_brownian_bridge_chain_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, float* w_out, const float* prev, float scale,
                                    const float* base_a, float fa, const float* base_b, float fb, int64_t n, int64_t elem_offset,
                                    const uint64_t* node_ids, const float* coefs, int nnodes, uint64_t seed, int64_t latent_elems,
                                    void* stream);
/* sonar_philox_normal_acc_f32 / sonar_perlin_generate_acc_f32 (iters == 1: `terms` is the summed lattice) with `pre` riding along.
 * Whole 4-element groups only (n, elem_offset, chw multiples of 4; 16-byte aligned tensors): SONAR_ERR_UNSUPPORTED otherwise. */
int sonar_philox_normal_chain_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t n, uint64_t seed, uint64_t stream_id,
                                  int64_t elem_offset, void* stream);
int sonar_perlin_generate_chain_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, const float* terms, int64_t B, int64_t chw,
                                    float div_fac, uint64_t seed, uint64_t stream_id, int64_t elem_offset, void* stream);
/* Pyramid noise (sonar_pyramid_generate_f32's values, levels drawn in the kernel or passed in) folded into the running sum, `pre`
 * (nullable) as above: the plane kernel's generator shares the tile keying of the Gaussian / Perlin generators, so any whole-plane
 * shape it can run can host them.  SONAR_ERR_UNSUPPORTED when the plane kernel cannot run the shape (nothing was done). */
int sonar_pyramid_generate_acc_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t planes, int64_t H, int64_t W,
                                   int64_t nlevels, const float* const* level_ptrs, const int64_t* level_h, const int64_t* level_w,
                                   const float* level_weight, int mode, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                   void* stream);
/* sonar_pyramid_generate_acc_f32 hosting a Perlin item (`pre`, kind PERLIN) for a chain that is called step after step with stream ids it
 * can foresee (the prepared plans): extra leading workgroups of the same launch compute the summed lattice [lattice_channels][H][W] of a
 * LATER call's Perlin item into `lattice_out` (as sonar_perlin_lattice_f32 with `seed`, `lattice_stream_id` would) -- independent of the
 * rest of the launch, and one launch less on that later call's critical path. */
int sonar_pyramid_generate_acc_ahead_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t planes, int64_t H, int64_t W,
                                         int64_t nlevels, const float* const* level_ptrs, const int64_t* level_h, const int64_t* level_w,
                                         const float* level_weight, int mode, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                         float* lattice_out, int64_t lattice_iters, int64_t lattice_channels, int blend_mode,
                                         uint64_t lattice_stream_id, void* stream);

/* ---------------------------------------------------------------- Perlin (row P) */
/* py/noise_generation.py:465-476,388-405 at the only position generate() uses (grid == output,
 * block 1x1, pos (0.5,0.5)): angles[iters][C][H+1][W+1] -> terms[iters][C][H][W] evaluating the
 * reference's blend tree.  blend_mode: SONAR_BLEND_* */
int sonar_perlin_terms_f32(const float* angles, float* terms, int64_t iters, int64_t C, int64_t H, int64_t W,
                           int blend_mode, void* stream);
/* generate mode: the same terms with the lattice angles drawn where they are used (counter-based, keyed by seed / stream_id /
 * lattice point / iteration; shared by every latent and every rank), summed over the iterations: terms_sum[C][H][W] */
int sonar_perlin_lattice_f32(float* terms_sum, int64_t iters, int64_t C, int64_t H, int64_t W, int blend_mode, uint64_t seed,
                             uint64_t stream_id, void* stream);
/* replay mode, py/noise_generation.py:478-493: out = base/div_fac (+ terms[i] broadcast over B, in order) */
int sonar_perlin_apply_f32(const float* base, const float* terms, float* out, int64_t B, int64_t chw,
                           int64_t iters, float div_fac, double* partials /*nullable*/, void* stream);
/* generate mode: base u~U[0,1) from Philox(seed, stream_id, elem_offset+e) fused with the above */
int sonar_perlin_generate_f32(const float* terms, float* out, int64_t B, int64_t chw, int64_t iters, float div_fac,
                              uint64_t seed, uint64_t stream_id, int64_t elem_offset, double* partials /*nullable*/,
                              void* stream);

/* generate mode + scale_noise(factor, normalized=True) without a second sweep over the tensor (SURVEY.md §8d
 * "stats-before-write"): pass 1 re-draws the values and only reduces (sum, sumsq) -> partials; pass 2 re-draws,
 * applies the on-device normalisation decision and writes the final tensor once. */
int sonar_perlin_noise_f32(const float* terms, float* out, int64_t B, int64_t chw, int64_t iters, float div_fac,
                           uint64_t seed, uint64_t stream_id, int64_t elem_offset, float factor, float threshold_std_devs,
                           double* partials /*workspace, SONAR_NPART pairs*/, void* stream);
/* sonar_perlin_lattice_f32 + sonar_perlin_noise_f32 for a sampler that is called step after step with stream ids it can foresee (the
 * prepared plans, below): ONE launch per call in the steady state.  The launch runs this call's final pass (`terms`: its summed lattice,
 * `partials` + have_stats: its statistics, both left by the previous launches; have_stats == 0: the statistics pass is launched first),
 * then the statistics pass of the NEXT call (tile stream `next_stream_id` against `terms_next`, nullable) into `partials_next`, and in
 * extra blocks the lattice of a LATER call (`lattice_out`, nullable; `lattice_iters`, C, H, W, `blend_mode`, `lattice_stream_id` as
 * sonar_perlin_lattice_f32 takes them) -- nothing inside the launch depends on anything else inside it.  The output bits are those of the
 * two entry points it replaces.  Only where sonar_perlin_noise_ahead_ok() says 1 (whole 4096-element tiles per latent, at most 4096
 * tiles: the launch-bound sizes); SONAR_ERR_UNSUPPORTED otherwise. */
int sonar_perlin_noise_ahead_ok(int64_t B, int64_t chw, int64_t elem_offset);
int sonar_perlin_noise_ahead_f32(const float* terms, float* out, int64_t B, int64_t chw, float div_fac, uint64_t seed, uint64_t stream_id,
                                 int64_t elem_offset, float factor, float threshold_std_devs, double* partials, int have_stats,
                                 uint64_t next_stream_id, const float* terms_next, double* partials_next, float* lattice_out,
                                 int64_t lattice_iters, int64_t C, int64_t H, int64_t W, int blend_mode, uint64_t lattice_stream_id,
                                 void* stream);

/* ---------------------------------------------------------------- Pyramid (row Y) */
/* dst[B*C][H][W] += bilinear_upsample(src[B*C][h][w]) * scale   (F.interpolate(mode="bilinear",
 * align_corners=False), py/utils.py:58-67 <- py/noise_generation.py:629-646).  mode: 0 bilinear,
 * 1 nearest-exact, 2 area (adaptive average, used when downscaling), 3 nearest (legacy floor(dst * in / out)), 4 bicubic
 * (A = -0.75, clamped taps), 5 bicubic with align_corners=True (py/noise.py:583-588, GuidedNoise's reference latent),
 * 6 bilinear with align_corners=True (py/nodes/powernoise.py:133, the filter's gain curve) */
int sonar_resample_acc_f32(float* dst, const float* src, int64_t planes, int64_t H, int64_t W, int64_t h, int64_t w,
                           float scale, int mode, int accumulate, double* partials /*nullable*/, void* stream);
/* generate mode: out = N(0,1) * base_scale + sum_l upsample(levels[l]) * weights[l].  level_ptrs[l]: device pointer to a
 * [planes][h_l][w_l] grid, or NULL = drawn on device: a NULL level of the latent's own size is folded into the base draw
 * (sum of two independent normals: base_scale = sqrt(1 + w^2)); a smaller NULL level is drawn by the plane kernel (stream
 * id stream_id + 2 + l, keyed by global plane) -- SONAR_ERR_UNSUPPORTED if that kernel cannot run this shape. */
int sonar_pyramid_generate_f32(float* out, int64_t planes, int64_t H, int64_t W, int64_t nlevels,
                               const float* const* level_ptrs /*host array of device ptrs*/, const int64_t* level_h,
                               const int64_t* level_w, const float* level_weight, int mode, uint64_t seed,
                               uint64_t stream_id, int64_t elem_offset, double* partials /*nullable*/, void* stream);
/* Host only, no GPU work: which kernel the pyramid entry points give a level list, by the arithmetic the launch itself uses (the LDS the
 * grids, the coordinate tables and the stretched rows take against the 64 KB budget, W % 4, whole planes): 0 = the flat kernel (supplied
 * grids only: a level drawn in the kernel is refused there), 1 = the plane kernel, 2 = the plane kernel with stretched rows.  level_h /
 * level_w are the caller's list; its first level of the latent's own size counts as drawn (folded into the base draw: it takes no LDS).
 * The kernel route only: the 16-byte alignment and the argument checks stay with the entry points.  SONAR_ERR_UNSUPPORTED for more than
 * 12 grids. */
int sonar_pyramid_route(int64_t H, int64_t W, int64_t nlevels, const int64_t* level_h, const int64_t* level_w, int mode, int64_t elem_offset);

/* same, with the normaliser folded in (see sonar_perlin_noise_f32) */
int sonar_pyramid_noise_f32(float* out, int64_t planes, int64_t H, int64_t W, int64_t nlevels,
                            const float* const* level_ptrs, const int64_t* level_h, const int64_t* level_w,
                            const float* level_weight, int mode, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                            float factor, float threshold_std_devs, double* partials, void* stream);
/* The same call (every level drawn in the kernel, bilinear: the generate-mode call of PyramidNoiseGenerator) in a sampler's steady state,
 * for prepared plans (round 6): ONE launch.  Half of its workgroups run this call's planes and store them normalised -- with the
 * statistics in `partials` (left there by the previous call's launch when `have_stats`; else a launch of this call's planes without
 * stores computes them first) and scale_noise's own operation sequence: the output bits are sonar_pyramid_noise_f32's -- the other half
 * run the planes of the call that will draw with `next_stream_id` and the `next_*` level table without storing anything and leave its
 * (sum, sumsq) partials in `partials_next`, the ones its own generating launch would leave.  SONAR_ERR_UNSUPPORTED (nothing launched) when
 * a level table is beyond the plane kernel's stretched-rows form. */
int sonar_pyramid_noise_ahead_f32(float* out, int64_t planes, int64_t H, int64_t W, int64_t nlevels, const int64_t* level_h,
                                  const int64_t* level_w, const float* level_weight, int mode, uint64_t seed, uint64_t stream_id,
                                  int64_t elem_offset, float factor, float threshold_std_devs, double* partials, int have_stats,
                                  uint64_t next_stream_id, int64_t next_nlevels, const int64_t* next_level_h, const int64_t* next_level_w,
                                  const float* next_level_weight, double* partials_next, void* stream);

/* Levels that are drawn only to be shrunk, with on-device draws: PyramidOld (py/noise_generation.py:567-606: noise = sum_i discount^i *
 * F.interpolate(normal(std = 0.5^i) at (2^(i+1) H) x (2^(i+1) W), size = (H, W), mode)) and HighresPyramid (:517-564: levels of up to 15 x
 * the latent's sides).  The levels are never materialised: level l's value at (global plane, ys, xs) is a counter-based normal keyed by
 * its global element index (Philox4x32-10 of group e / 4, Box-Muller, slot e % 4; stream stream_id + l) times level_sd[l], and the kernel
 * draws exactly the taps the interpolation reads -- mode 1 nearest-exact / 3 nearest one, 0 bilinear 2 x 2, 4 bicubic 4 x 4 per level and
 * output, by the index and weight rules of sonar_resample_acc_f32 (same ids):
 *     out[p][y][x] (+)= sum_l level_weight[l] * interpolate(level_l)[p][y][x]        (accumulate != 0: added to out)
 * Mode 2 (area) only for levels of whole multiples of the output size: the mean of a block of independent normals is itself a normal of
 * std level_sd / sqrt(block size), independent from block to block, and is drawn as such (keyed by the output element; the same joint
 * distribution as drawing the level and pooling it); any other ratio: SONAR_ERR_UNSUPPORTED (the windows overlap: draw the level with
 * sonar_level_normal_f32 and resample it).  At most 16 levels.  sonar_level_normal_f32 writes one whole level [planes][h][w] from the same
 * keys: resampling those levels with sonar_resample_acc_f32 gives the sampled kernel's values (the tests do). */
int sonar_levels_sampled_f32(float* out, int64_t planes, int64_t H, int64_t W, int nlevels, const int64_t* level_h, const int64_t* level_w,
                             const float* level_weight, const float* level_sd, int mode, uint64_t seed, uint64_t stream_id,
                             int64_t plane_offset, int accumulate, void* stream);
int sonar_level_normal_f32(float* level, int64_t planes, int64_t h, int64_t w, float sd, uint64_t seed, uint64_t stream_id,
                           int64_t plane_offset, void* stream);

/* dst[N][C][H][W] (+)= bislerp(src[N][C][h][w]) * scale: ComfyUI's comfy.utils.bislerp (the reference's common_upscale(..., "bislerp"),
 * py/utils.py:58-67; not vendored by the reference: parity unpinned, the definition is restated in DESIGN.md).  The C-vector of a pixel is
 * interpolated spherically, along the width and then along the height, in one launch:
 *     T[n][:][y][X] = slerp(S[n][:][y][c1w[X]], S[n][:][y][c2w[X]], rw[X]),   O[n][:][Y][X] = slerp(T[n][:][c1h[Y]][X], T[n][:][c2h[Y]][X], rh[Y])
 * with slerp(b1, b2, r) over the channel axis: unit vectors u = b / |b| (0 for a zero vector), dot = sum(u1 u2), om = acos(dot),
 * (sin((1 - r) om) u1 + sin(r om) u2) / sin(om) * (|b1| (1 - r) + |b2| r); b1 where dot > 1 - 1e-5, b1 (1 - r) + b2 r where dot < 1e-5 - 1
 * (the jumps at the two thresholds are the definition's).  c1w / c2w / rw [W] and c1h / c2h / rh [H] are device tables (indices into the
 * source axis and the interpolation ratio), built on the host from torch's bilinear coordinates; an index outside the axis is clamped.  Any
 * C > 0.  accumulate != 0: added to dst; partials (nullable): the (sum, sumsq) partials of the finished dst, as sonar_resample_acc_f32
 * leaves them.  Conventions of sonar_resample_acc_f32: error codes, no allocation, asynchronous on `stream`. */
int sonar_bislerp_acc_f32(float* dst, const float* src, int64_t N, int64_t C, int64_t H, int64_t W, int64_t h, int64_t w, float scale,
                          int accumulate, const int32_t* c1w, const int32_t* c2w, const float* rw, const int32_t* c1h, const int32_t* c2h,
                          const float* rh, double* partials /*nullable*/, void* stream);

/* ---------------------------------------------------------------- power-law rFFT noise (row PW) */
/* Which kernel family serves an H x W plane of the power-noise path: 1 = the fixed-size LDS FFT kernels (powers of two, 16..256),
 * 2 = the general-size kernels (any even H <= 512, even W <= 1024 with H*(W/2+1) + H + W <= 20224 complex values: two-factor table-twiddle DFTs in LDS;
 * e.g. 104 x 152 for 832 x 1216 px), 4 = half-spectrum beyond LDS (even H <= 512, even W <= 2048: 256 x 256 for 2048 px): GENERATED noise runs
 * in column blocks through a complex workspace (sonar_power_block_f32); a supplied spectrum and the spectral filter take the
 * sonar_dft_* passes as for kind 0, 0 = unsupported by the LDS kernels (the sonar_power_* / sonar_spectral_filter_f32 calls return -2 for
 * kinds 0 and 4). */
int sonar_power_plane_kind(int64_t H, int64_t W);
/* Host only, no GPU work: the plan of the general-size kernels (kind 2) for an H x W plane, as the launch itself forms it.
 *   family  -1: as the launch routes the size; 0 / 1: the factor pairs of that family's codelet set whatever the route (what best_split
 *           gives an SDXL bucket's size over all codelet lengths, say)
 *   out[12] family (0 = run-time sizes with the codelets 2 .. 12, 1 = with every codelet length, 2 = an SDXL bucket's compile-time pairs),
 *           hn1, hn2 (H = hn1 x hn2), mn1, mn2 (W / 2 = mn1 x mn2), whether the inverse rows fold the c2r pre-twiddle into their first pass,
 *           threads per workgroup (512 or 1024), row batches of that folded pass (0 when it is not folded), then how the passes of
 *           length hn1, hn2, mn1, mn2 run: 1 = a register codelet of that length, 0 = direct sums, 2 = absent (a second pass of length 1)
 * SONAR_ERR_UNSUPPORTED where sonar_power_plane_kind(H, W) != 2. */
int sonar_power_any_plan(int64_t H, int64_t W, int family, int32_t* out);
/* Kind-4 planes, spectrum drawn on device (py/nodes/powernoise.py:338-366 -- the reference filters the rfft2 of white noise, which IS
 * a complex-normal half-spectrum: drawn directly, no forward transform):
 *   mode 0: out = irfft2(drawn * filter, norm="ortho"); statistics of out into `partials` when given
 *   mode 1: the same, normalised like sonar_power_noise_f32 (the column pass sums the Parseval statistics of the filtered spectrum it holds
 *           into `partials`, the row pass writes normalised values): two launches, the tensor written once, the workspace written and read
 *           once (3 x the tensor of HBM traffic)
 *   mode 2: the drawn spectrum itself into `ws` as [planes][H][W/2+1] complex64 (filter, out unused): what modes 0 / 1 transform
 *   ws      [planes][H][W/2+1] complex64 scratch, sonar_power_block_ws_bytes(planes, H, W) bytes (-1: not a kind-4 plane)
 * Streams are keyed by (rng_group of global planes, block of <= 32 spectrum columns, thread slot): shards of a batch agree; the values
 * differ from the white-noise route round 3 used for these planes. */
int64_t sonar_power_block_ws_bytes(int64_t planes, int64_t H, int64_t W);
int sonar_power_block_f32(const float* filter, float* ws, float* out, int64_t planes, int64_t H, int64_t W, uint64_t seed, uint64_t stream_id,
                          int64_t plane_offset, int rng_group, int mode, float factor, float threshold_std_devs, double* partials /*mode 1: required*/,
                          void* stream);
/* py/nodes/powernoise.py:366-377: out = irfft2(z * filter, s=(H,W), norm="ortho").
 *   z      [planes][H][W/2+1] complex64 (interleaved re,im) or NULL -> drawn on device: complex normal
 *          (a+ib)*sqrt(1/2); plane p of this call is global plane plane_offset + p of the logical batch.
 *   rng_group  device draws are keyed per group of `rng_group` consecutive global planes (the Philox seeding of the
 *          xoshiro bursts is paid once per group); planes and plane_offset must be multiples of it.  It is part of
 *          the stream definition: every shard of a batch must pass the same value (the host uses 4 when C % 4 == 0,
 *          else 1).  Ignored when z is supplied.
 *   filter [H][W/2+1] fp32 (broadcast over planes)
 * Supported: H, W powers of two in 16..256 with the half-spectrum LDS-resident (else SONAR_ERR_UNSUPPORTED). */
int sonar_power_irfft2_f32(const float* z, const float* filter, float* out, int64_t planes, int64_t H, int64_t W,
                           uint64_t seed, uint64_t stream_id, int64_t plane_offset, int rng_group,
                           double* partials /*nullable*/, void* stream);
/* draw + filter + irfft2 + scale_noise(factor, normalized=True) writing the tensor ONCE: the output statistics are
 * obtained from the spectrum by Parseval's identity in a first RNG-only pass (no FFT, no stores; only the radius
 * uniforms of the interior columns and the two edge columns are drawn there). */
int sonar_power_noise_f32(const float* filter, float* out, int64_t planes, int64_t H, int64_t W, uint64_t seed,
                          uint64_t stream_id, int64_t plane_offset, int rng_group, float factor, float threshold_std_devs,
                          double* partials /*workspace*/, void* stream);

/* sonar_power_noise_f32 with a look-ahead for samplers that call the same generator step after step (consecutive stream ids).
 * have_stats != 0: `partials` already holds THIS call's statistics (what an earlier call left in its partials_next for exactly this
 * filter / shape / seed / stream_id / plane_offset / rng_group): the statistics launch is skipped.  partials_next (may be NULL):
 * receives the statistics of the same call with stream id next_stream_id, computed by the final pass's otherwise idle waves -- pass it
 * as `partials` with have_stats = 1 if the next call turns out to be that one, ignore it otherwise.  Output bits are those of
 * sonar_power_noise_f32 either way.  Only where sonar_power_noise_ahead_ok() says 1: the pipelined 128 x 128 path with at most 512 work
 * units (idle waves of the final pass), and -- as extra workgroups of the final pass's launch -- every fixed-size or general-size
 * LDS-resident plane with at most 256 work units (the launch-bound batch sizes: one launch per call); SONAR_ERR_UNSUPPORTED elsewhere.  Same call site: py/nodes/powernoise.py:338-408 followed by py/utils.py:85-106. */
int sonar_power_noise_ahead_ok(int64_t planes, int64_t H, int64_t W, int rng_group);
/* process-wide switch between the two generate kernels for 128 x 128 planes: 1 (default) the pipelined kernel where it applies (more than
 * 256 planes), 0 the phase-serial kernel everywhere; < 0 only asks.  Same stream definition, the same bits either way
 * (tests/test_gpu_round3.py); returns the previous setting.  For A/B timing and that test -- not a per-call option. */
int sonar_power_pipeline(int enable);
int sonar_power_noise_ahead_f32(const float* filter, float* out, int64_t planes, int64_t H, int64_t W, uint64_t seed,
                                uint64_t stream_id, int64_t plane_offset, int rng_group, float factor, float threshold_std_devs,
                                double* partials, int have_stats, uint64_t next_stream_id, double* partials_next, void* stream);
/* the spectrum the two entry points above draw for (seed, stream_id, plane_offset, rng_group):
 * z_out[planes][H][W/2+1] complex64 (tests / replaying a device draw) */
int sonar_power_spectrum_f32(float* z_out, int64_t planes, int64_t H, int64_t W, uint64_t seed, uint64_t stream_id,
                             int64_t plane_offset, int rng_group, void* stream);
/* spectral filter of real planes: out = irfft2(rfft2(x, norm="ortho") * filter, s=(H,W), norm="ortho") with
 * filter[H][W/2+1] real; forward and inverse FFT both LDS-resident, x read once, out written once (x != out).
 * PowerFilterNoiseItem / time_brownian path (py/nodes/powernoise.py:356-366,471-522) and, with a symmetrised
 * filter, Re(ifft2(fft2(x) * F)) of OneF / GreenTest (py/noise_generation.py:680-759).  partials: optional (sum, sumsq). */
int sonar_spectral_filter_f32(const float* x, const float* filter, float* out, int64_t planes, int64_t H, int64_t W,
                              double* partials, void* stream);
/* x *= mul / std, std = unbiased standard deviation from the (sum, sumsq) partials of n_total elements
 * (GreenTestNoiseGenerator, py/noise_generation.py:702: noise *= scale / noise.std()); no host sync */
int sonar_std_scale_f32(float* x, int64_t n, float mul, const double* partials, int64_t npart, int64_t n_total, void* stream);
/* py/nodes/powernoise.py:96-101 ChannelMixer.apply: out[b][i] = sum_j mixer[i][j] * in[b][j] over planes of hw */
int sonar_channel_mix_f32(const float* in, const float* mixer, float* out, int64_t B, int64_t C, int64_t hw,
                          double* partials /*nullable*/, void* stream);

/* ---------------------------------------------------------------- 2-D DWT / IDWT (rows W, WC, WF) */
/* pytorch_wavelets DWTForward/DWTInverse semantics == pywt.dwt2/idwt2 per level
 * (py/wavelet_functions.py:56-105).  One level per call; the host loops levels.
 *   mode: 0 zero, 1 symmetric, 2 reflect, 3 periodization, 4 periodic(ppd), 5 constant(replicate)
 *   dec_lo/dec_hi (rec_lo/rec_hi): HOST arrays of `flen` (1 .. 102: every wavelet of the table, db38 and coif17 included)
 *             taps in pywt order; more is SONAR_ERR_ARG "1..102 filter taps required".  Even lengths up to 20 on planes
 *             that fit a 64 KiB LDS tile run in one LDS-staged launch, everything else as a row pass and a column pass.
 *   forward : x[planes][H][W] -> ll[planes][h][w], hi[planes][3][h][w]  (orientations LH,HL,HH == pywt cH,cV,cD;
 *             h = sonar_dwt_out_len(H), w = sonar_dwt_out_len(W))
 *   inverse : ll[planes][ll_h][ll_w] (only its leading h x w block is used: pytorch_wavelets drops the extra
 *             row/column of a coarser ll), hi[planes][3][h][w] -> out[planes][Ho][Wo], Ho/Wo <= full size
 *             (2h - flen + 2, or 2h for periodization)
 *   ws      : caller-provided workspace of sonar_dwt2_ws_bytes(...) bytes (row/column pass intermediate)
 */
int64_t sonar_dwt_out_len(int64_t n, int64_t flen, int mode);
int64_t sonar_dwt2_ws_bytes(int64_t planes, int64_t H, int64_t W, int flen, int mode, int elem_size, int inverse);
int sonar_dwt2_fwd_f32(const float* x, float* ll, float* hi, int64_t planes, int64_t H, int64_t W,
                       const double* dec_lo, const double* dec_hi, int flen, int mode, void* ws, void* stream);
int sonar_dwt2_fwd_f64(const double* x, double* ll, double* hi, int64_t planes, int64_t H, int64_t W,
                       const double* dec_lo, const double* dec_hi, int flen, int mode, void* ws, void* stream);
int sonar_dwt2_inv_f32(const float* ll, int64_t ll_h, int64_t ll_w, const float* hi, float* out, int64_t planes,
                       int64_t h, int64_t w, int64_t Ho, int64_t Wo, const double* rec_lo, const double* rec_hi,
                       int flen, int mode, void* ws, void* stream);
int sonar_dwt2_inv_f64(const double* ll, int64_t ll_h, int64_t ll_w, const double* hi, double* out, int64_t planes,
                       int64_t h, int64_t w, int64_t Ho, int64_t Wo, const double* rec_lo, const double* rec_hi,
                       int flen, int mode, void* ws, void* stream);
/* 1-D DWT / IDWT of flattened latents, one level per call (replaces pytorch_wavelets DWT1DForward / DWT1DInverse behind
 * Wavelet(use_1d_dwt=True), py/wavelet_functions.py:56-57; the callers flatten [B,C,H,W] to [B,C,H*W],
 * py/wavelet_cfg.py:713-715, py/noise_generation.py:1982-1986).  x[rows][L] -> lo[rows][n], hi[rows][n] with
 * n = sonar_dwt_out_len(L, flen, mode); the inverse reads the leading n samples of each lo row (row pitch lo_len >= n:
 * a coarser approximation may be one sample longer than its band) and writes out[rows][Lo], Lo <= 2n - flen + 2
 * (2n in periodization mode).  Same taps / mode conventions as the 2-D entry points; no workspace. */
int sonar_dwt1_fwd_f32(const float* x, float* lo, float* hi, int64_t rows, int64_t L, const double* dec_lo,
                       const double* dec_hi, int flen, int mode, void* stream);
int sonar_dwt1_fwd_f64(const double* x, double* lo, double* hi, int64_t rows, int64_t L, const double* dec_lo,
                       const double* dec_hi, int flen, int mode, void* stream);
int sonar_dwt1_inv_f32(const float* lo, int64_t lo_len, const float* hi, float* out, int64_t rows, int64_t n, int64_t Lo,
                       const double* rec_lo, const double* rec_hi, int flen, int mode, void* stream);
int sonar_dwt1_inv_f64(const double* lo, int64_t lo_len, const double* hi, double* out, int64_t rows, int64_t n, int64_t Lo,
                       const double* rec_lo, const double* rec_hi, int flen, int mode, void* stream);
/* WaveletCFG band arithmetic, py/wavelet_cfg.py:750-791, for one band tensor of n elements whose element i
 * belongs to orientation group g = (i / group_size) % groups (groups = 3 for yh[B,C,3,h,w], 6 for the dual-tree transform's [B,C,6,h,w,2] with group_size = 2 h w, 1 for yl):
 *   c = cond*s_cond[g]; u = uncond*s_uncond[g]; d = (c-u)*s_diff[g]; out = blend(u, d, strength)*s_final[g]
 * s_* are HOST arrays of `groups` (<= 8) doubles; multiplications by exactly 1 are skipped like the reference. */
int sonar_wcfg_band_f32(const float* cond, const float* uncond, float* out, int64_t n, int64_t group_size,
                        int64_t groups, const double* s_cond, const double* s_uncond, const double* s_diff,
                        const double* s_final, int blend_mode, double strength, void* stream);
int sonar_wcfg_band_f64(const double* cond, const double* uncond, double* out, int64_t n, int64_t group_size,
                        int64_t groups, const double* s_cond, const double* s_uncond, const double* s_diff,
                        const double* s_final, int blend_mode, double strength, void* stream);
/* The same arithmetic on a band of the 1-D transform ([B, C, l] rows of row_len coefficients, use_1d_dwt).  The reference's
 * wavelet_scaling (py/wavelet_functions.py:208-215) indexes axis 2 of every band: the orientation axis of a 2-D band, but the
 * COEFFICIENT axis of a 1-D band, whose scale table has one entry -- so only the first coefficient of each row is scaled.
 * s_* are HOST pointers to ONE double each (NULL = 1): applied where i % row_len == 0; every other element uses unit scales. */
int sonar_wcfg_band_head_f32(const float* cond, const float* uncond, float* out, int64_t n, int64_t row_len,
                             const double* s_cond, const double* s_uncond, const double* s_diff, const double* s_final,
                             int blend_mode, double strength, void* stream);
int sonar_wcfg_band_head_f64(const double* cond, const double* uncond, double* out, int64_t n, int64_t row_len,
                             const double* s_cond, const double* s_uncond, const double* s_diff, const double* s_final,
                             int blend_mode, double strength, void* stream);
/* The whole transform-domain step of WaveletCFG in `2 * levels` launches (py/wavelet_cfg.py:750-791,729-748), LDS-staged:
 * each level's analysis handles cond and uncond together (fp32 inputs cast in registers), applies
 * blend(u*s_u, (c*s_c - u*s_u)*s_d, strength)*s_f per band before storing; each level's synthesis is one launch; the last
 * one writes out = x - result (subtract_from_x) or result, cropped to H x W, as fp32.  _f32 / _f64 = arithmetic type
 * (high_precision_mode).  yl_scales[4] = {cond, uncond, diff, final}; yh_scales[levels][4][3] = the same per level
 * (finest first) and orientation (cH, cV, cD).  ws: sonar_wcfg_fused_ws_bytes(...) bytes; returns
 * SONAR_ERR_UNSUPPORTED (nothing launched) when a level does not fit the LDS tile.
 * perfect_reconstruction != 0: the caller vouches that (dec, mode_fwd) / (rec, mode_inv) reconstruct exactly (one wavelet both
 * ways).  Rules that then only scale the difference bands (every cond / uncond / final scale 1, any per-level, per-orientation
 * diff scales) take the single-tensor route: IDWT(blend(U, D (C - U), t)) = ku u + kt IDWT(D DWT(c - u)) -- c - u is formed on
 * load, ONE transform runs instead of two, and the last synthesis adds ku * uncond. */
int64_t sonar_wcfg_fused_ws_bytes(int64_t planes, int64_t H, int64_t W, int levels, int dec_len, int mode_fwd, int rec_len,
                                  int mode_inv, int elem_size);
int sonar_wcfg_fused_f32(const float* cond, const float* uncond, const float* x, float* out, int64_t planes, int64_t H, int64_t W,
                         int levels, const double* dec_lo, const double* dec_hi, int dec_len, int mode_fwd, const double* rec_lo,
                         const double* rec_hi, int rec_len, int mode_inv, const double* yl_scales, const double* yh_scales,
                         int blend_mode, double strength, int subtract_from_x, int perfect_reconstruction, void* ws, int64_t ws_bytes,
                         void* stream);
/* sonar_wcfg_fused_f64 keeps level 1's three detail bands -- 3/4 of that level's coefficients, written once and read once -- in fp32 in
 * its workspace (arithmetic on both sides and every other band stay fp64; the result is an fp32 tensor): 110 MB less HBM traffic per 256 SDXL
 * latents.  sonar_wcfg_hi_storage(0) stores them in fp64 (1: fp32, the default; -1: query); returns the previous setting.  Process-wide. */
int sonar_wcfg_hi_storage(int fp32);
int sonar_wcfg_fused_f64(const float* cond, const float* uncond, const float* x, float* out, int64_t planes, int64_t H, int64_t W,
                         int levels, const double* dec_lo, const double* dec_hi, int dec_len, int mode_fwd, const double* rec_lo,
                         const double* rec_hi, int rec_len, int mode_inv, const double* yl_scales, const double* yh_scales,
                         int blend_mode, double strength, int subtract_from_x, int perfect_reconstruction, void* ws, int64_t ws_bytes,
                         void* stream);
/* ---------------------------------------------------------------- DTCWT (row 8f-4)
 * The dual-tree complex wavelet transform the reference reaches through pytorch_wavelets' DTCWTForward / DTCWTInverse
 * (py/wavelet_functions.py:56-73; Kingsbury's dtwavexfm2 / dtwaveifm2).  Each of its stages (odd-length filters with symmetric
 * extension, decimating / interpolating dual-tree filters) is a sparse linear map along one axis with `taps` terms per output row:
 *   out[o][j][i] (+)= sum_k coef[j][k] * x[o][idx[j][k]][i],  o < outer, j < n_out, i < inner
 * idx [n_out][taps] (int32) / coef [n_out][taps]: DEVICE tables built once per length by the host (py/dtcwt.py).  x != out. */
int sonar_axis_taps_f32(const float* x, float* out, int64_t outer, int64_t n_in, int64_t n_out, int64_t inner, const int* idx,
                        const float* coef, int taps, int accumulate, void* stream);
int sonar_axis_taps_f64(const double* x, double* out, int64_t outer, int64_t n_in, int64_t n_out, int64_t inner, const int* idx,
                        const double* coef, int taps, int accumulate, void* stream);
/* q2c / c2q: three real planes lh, hh, hl [planes][2h][2w] <-> bands [planes][6][h][w][2] (orientations 15, 45, 75, 105, 135, 165
 * degrees, last axis re / im): quad (a b / c d) <-> ((a - d) + i (b + c)) / sqrt 2 and ((a + d) + i (b - c)) / sqrt 2; lh feeds
 * orientations (0, 5), hh (1, 4), hl (2, 3). */
int sonar_dtcwt_q2c_f32(const float* lh, const float* hh, const float* hl, float* bands, int64_t planes, int64_t h, int64_t w, void* stream);
int sonar_dtcwt_c2q_f32(const float* bands, float* lh, float* hh, float* hl, int64_t planes, int64_t h, int64_t w, void* stream);
int sonar_dtcwt_q2c_f64(const double* lh, const double* hh, const double* hl, double* bands, int64_t planes, int64_t h, int64_t w, void* stream);
int sonar_dtcwt_c2q_f64(const double* bands, double* lh, double* hh, double* hl, int64_t planes, int64_t h, int64_t w, void* stream);
/* ---------------------------------------------------------------- ScatternetFilteredNoise
 * One layer of the dual-tree scattering network (pytorch_wavelets' ScatLayer; py/noise_generation.py:2035-2193), fused
 * (csrc/scatternet.hip).  x [B][C][H][W] fp32, any H, W >= 1: an odd side is extended by repeating its last row / column (He, We: the
 * even sizes).  Level-1 DTCWT analysis with the biorthogonal pair h0 (n0 taps) / h1 (n1 taps) under half-sample symmetric extension
 * (the full modular fold: the halo may be longer than the plane), then
 *   band 0      the 2 x 2 mean of the low-pass plane
 *   bands 1..6  s / (sqrt(s + b^2) + b) = sqrt(re^2 + im^2 + b^2) - b of the orientations 15, 45, 75, 105, 135, 165 degrees, s = re^2 + im^2,
 *               b = magbias, (re, im) the quad combinations of sonar_dtcwt_q2c
 * band-major: channel k = band * C + c of the [B][7 C][He / 2][We / 2] result.  Only the channels k0 .. k0 + nk - 1 are computed and
 * written, into out [B][nk][He / 2][We / 2]; a band outside the window is neither filtered nor stored; k0 need not be a multiple of C.
 * The values of a channel do not depend on the window.  h0 / h1 are HOST arrays (read before the call returns): the lengths 5 / 7
 * (near_sym_a), 5 / 3 (legall) and 9 / 7 (antonini) are built, anything else is SONAR_ERR_UNSUPPORTED.  One launch: a workgroup per tile of
 * SONAR_SCAT_TILE_H x SONAR_SCAT_TILE_W output values, band group ({0}, {1, 6}, {2, 5}, {3, 4}) and plane.
 * SONAR_ERR_ARG: a NULL or misaligned pointer, out == x, C, H or W < 1, B < 0, magbias negative or not finite, a tap not finite, a window
 * outside [0, 7 C).  SONAR_ERR_UNSUPPORTED: a side beyond SONAR_SCAT_MAX_SIDE, 2^31 workgroups or more.  All checked before the launch. */
#define SONAR_SCAT_TILE_H 16
#define SONAR_SCAT_TILE_W 32
#define SONAR_SCAT_MAX_SIDE 1048576
int sonar_scat_layer_f32(const float* x, float* out, int64_t B, int64_t C, int64_t H, int64_t W, const float* h0, int n0, const float* h1,
                         int n1, float magbias, int64_t k0, int64_t nk, void* stream);
/* normalize_to_scale_adv (py/utils.py:473-510; NormalizeToScaleNoise's advanced mode, py/noise.py:1262-1286): per row of `inner` elements the
 * negative values are rescaled between their own extremes to [min_neg, max_neg] (max_neg >= 0: the row's largest negative value) and the
 * positive ones to [min_pos, max_pos] (min_pos < 0: the row's smallest positive value); zeros stay, a sign whose range is degenerate
 * (:482-483) is copied.  stats_ws: 4 floats per row, 16-byte aligned.  Two launches. */
int sonar_signed_rescale_f32(const float* x, int64_t rows, int64_t inner, double min_neg, double max_neg, double min_pos, double max_pos, float eps,
                             float* stats_ws, float* out, void* stream);
/* Direct real 2-D DFT passes for planes the LDS-resident FFT kernels do not take (odd heights / widths -- 1080-line video gives
 * 135-row latents -- or planes beyond the LDS budget): torch.fft.rfft2 / irfft2 (py/nodes/powernoise.py:338-408,
 * py/noise_generation.py:680-759, py/nodes/freeu_extreme.py:10-29) as rows r2c -> columns (optionally x a real filter [H][K] on the
 * way in; inverse: e^{+}) -> rows c2r (x scale; the imaginary parts of the DC / Nyquist columns are ignored, as irfft does), through a
 * caller-owned complex64 workspace [planes][H][W/2+1].  Lines of at most 2048; unscaled except for `scale`.  Rows and columns run the
 * LDS line transforms of the general-size kernels (register codelets, a factor above 19 as direct sums; even widths with the
 * half-length trick, odd widths as full-length complex lines); an odd width that is a prime above 19, or buffers that are not 8-byte
 * aligned, run direct sums, O(N) per output.  sonar_dft_cols_f32: inverse = 0 forward, 1 inverse (the
 * filter multiplies the INPUT), 2 forward, x filter, inverse in one pass (the spectral filter's middle; SONAR_ERR_UNSUPPORTED when the
 * columns cannot go through LDS: run 0 then 1).  partials (nullable): (sum, sumsq) of the real output. */
int sonar_dft_rows_r2c_f32(const float* x, float* y, int64_t rows, int64_t W, void* stream);
int sonar_dft_cols_f32(const float* in, const float* filter /*nullable*/, float* out, int64_t planes, int64_t H, int64_t K, int inverse,
                       void* stream);
int sonar_dft_rows_c2r_f32(const float* y, float* out, int64_t rows, int64_t W, float scale, double* partials /*nullable*/, void* stream);
/* max over a non-empty device vector with torch.max's NaN rule, returned to the host: WaveletCFG's `sigma.max().item()`
 * (py/wavelet_cfg.py:795-796) as one launch that writes into pinned host memory + one wait.  `begin` only launches; `end` BLOCKS
 * until the value has landed (as `.item()` does) -- the host prepares everything that does not depend on the value in between.
 * One request per host thread and device at a time (`begin` twice without `end`: SONAR_ERR_ARG).  `sonar_max_to_host_f32` = both. */
int sonar_max_to_host_begin_f32(const float* x, int64_t n, void* stream);
int sonar_max_to_host_end_f32(float* result, void* stream);
int sonar_max_to_host_f32(const float* x, int64_t n, float* result, void* stream);
/* WaveletCFG for difference-only rules with ONE detail scale per level (py/wavelet_cfg.py:750-791 with `cond` / `uncond` / `final`
 * absent; the node's placeholder rule, BASELINE cfg4).  By linearity and perfect reconstruction
 *   IDWT(blend(DWT u, D (DWT c - DWT u), t)) = ku u + kt (g[0] v + Up_1(g[1] LL_1 + Up_2(... g[J] LL_J))),  v = c - u,
 * LL_j = low-pass analysis chain of v, Up_j = level-j synthesis with zero details, g[0] = d_1, g[j] = d_{j+1} - d_j, g[J] = l - d_J
 * (d_j: the detail scale of level j, l: the approximation scale; (ku, kt) = (1, t) inject, (1 - t, t) lerp, (1, -t) subtract_b).
 * One launch, a workgroup per plane, the LL pyramid stays in LDS: out = x - result (subtract_from_x) or result; fp32 tensors,
 * _f32 / _f64 = arithmetic type.  dec_lo / rec_lo: the `flen` (even, <= 20) low-pass taps of ONE wavelet (perfect-reconstruction
 * pair); g: HOST array of levels + 1 doubles.  SONAR_ERR_UNSUPPORTED when the pyramid does not fit in LDS
 * (sonar_wcfg_lowpass_lds_bytes < 0): callers use sonar_wcfg_fused_* then. */
int64_t sonar_wcfg_lowpass_lds_bytes(int64_t H, int64_t W, int levels, int flen, int mode_fwd, int mode_inv, int elem_size);
int sonar_wcfg_lowpass_f32(const float* cond, const float* uncond, const float* x, float* out, int64_t planes, int64_t H,
                           int64_t W, int levels, const double* dec_lo, const double* rec_lo, int flen, int mode_fwd,
                           int mode_inv, const double* g, double ku, double kt, int subtract_from_x, void* stream);
int sonar_wcfg_lowpass_f64(const float* cond, const float* uncond, const float* x, float* out, int64_t planes, int64_t H,
                           int64_t W, int levels, const double* dec_lo, const double* rec_lo, int flen, int mode_fwd,
                           int mode_inv, const double* g, double ku, double kt, int subtract_from_x, void* stream);
/* WaveletCFG with ANY per-level, per-orientation band scales in one launch, the coefficients resident in LDS (py/wavelet_cfg.py:750-791,
 * py/wavelet_functions.py:193-238).  Phi_D(v) = IDWT(D DWT(v)) with D = (yl_scale for the approximation, yh_scales[levels][3] = (cH, cV,
 * cD) per level, finest first) is linear in v, and with a perfect-reconstruction pair a level needs its approximation and ONE detail band
 * on chip (csrc/dwt_bands.h).  v = a - b (b nullable: v = a);  result = ku * b + kt * Phi_D(v);  out = x - (float)result
 * (subtract_from_x) or (float)result; x may alias out.  Difference-only rules: a = cond, b = uncond, D = the difference scales, (ku, kt)
 * as in sonar_wcfg_lowpass_*.  Any other rule with a linear blend is Phi_A(cond) + Phi_B(uncond): two launches, the second with x = out of
 * the first.  fp32 tensors, _f32 / _f64 = arithmetic type; dec / rec: the four filters (flen taps each, even, <= 20) of ONE wavelet.
 * SONAR_ERR_UNSUPPORTED when the coefficients do not fit in LDS (sonar_wcfg_bands_lds_bytes < 0) or the extension pair does not
 * reconstruct: callers use sonar_wcfg_fused_* then. */
int64_t sonar_wcfg_bands_lds_bytes(int64_t H, int64_t W, int levels, int flen, int mode_fwd, int mode_inv, int elem_size, int per_orientation);
int sonar_wcfg_bands_f32(const float* a, const float* b, const float* x, float* out, int64_t planes, int64_t H, int64_t W, int levels,
                         const double* dec_lo, const double* dec_hi, const double* rec_lo, const double* rec_hi, int flen, int mode_fwd,
                         int mode_inv, const double* yh_scales, double yl_scale, double ku, double kt, int subtract_from_x, void* stream);
int sonar_wcfg_bands_f64(const float* a, const float* b, const float* x, float* out, int64_t planes, int64_t H, int64_t W, int levels,
                         const double* dec_lo, const double* dec_hi, const double* rec_lo, const double* rec_hi, int flen, int mode_fwd,
                         int mode_inv, const double* yh_scales, double yl_scale, double ku, double kt, int subtract_from_x, void* stream);
/* process_output, py/wavelet_cfg.py:729-748: out = x - (float)crop(result)  (subtract_from_x = 1, target DENOISED)
 * or out = (float)crop(result); result is [planes][Hr][Wr] (f64 or f32), x/out are [planes][H][W] fp32 */
int sonar_wcfg_output_f32(const float* x, const void* result, int result_is_f64, float* out, int64_t planes,
                          int64_t H, int64_t W, int64_t Hr, int64_t Wr, int subtract_from_x, void* stream);
/* fp32 -> fp64 conversion of a contiguous buffer (get_context cast, py/wavelet_cfg.py:707,764-765) */
int sonar_cast_f32_f64(const float* in, double* out, int64_t n, void* stream);

/* ---------------------------------------------------------------- FreeU Extreme (csrc/freeu.hip) */
/* FreeUExtremeConfig.apply (py/nodes/freeu_extreme.py:187-230) on a UNet feature map x [B][C][H][W] of `dtype` (SONAR_DTYPE_*), addressed
 * in place: stride_b / stride_c are the batch and channel strides in ELEMENTS, every H x W plane is contiguous.  Arithmetic is fp32, the
 * result is rounded once (to nearest even) -- the reference rounds a half tensor after every operation.
 *  sonar_freeu_hidden_mean  get_scale's statistics, two launches, nothing read on the host:
 *                             mean[b][p] = (sum over ALL C channels of x[b][c][p]) / C       (fp32 [B][HW], HW = H * W; lanes walk p)
 *                             extremes[b] = (min, max) of mean[b][:]                           (fp32 [B][2]; a NaN makes both NaN, as torch.min / max)
 *                           ws (fp32, ws_elems values, nullable): with room for G >= 2 copies of mean, G = at most
 *                           sonar_freeu_hidden_mean_groups(B, C, HW) (host arithmetic: few positions and many channels), the channels are split
 *                           over G workgroups per 64 positions; their partial sums meet, in order, in the second launch.
 *  sonar_freeu_apply        the channels c0 .. c0 + cn - 1 of every sample, written in place:
 *                             f = x                                                  SONAR_FREEU_PLAIN (no power filter)
 *                             f = irfft2(rfft2(x, ortho) * filter, ortho)            SONAR_FREEU_FUSED: one workgroup per plane, both transforms in
 *                                                                                    LDS; filter is real [H][W/2+1]; planes of
 *                                                                                    sonar_power_plane_kind 1 and 2 only (else SONAR_ERR_UNSUPPORTED)
 *                             f = filtered[(b * cn + c - c0) * HW + p]                SONAR_FREEU_FILTERED: fp32 [B][cn][H][W], made by the caller
 *                                                                                    (the direct DFT passes for odd / oversized planes)
 *                             s = mean ? 1 + (scale - 1) * ((mean[b][p] - min_b) / (max_b - min_b)) : scale     (0 / 0 is NaN, not guarded;
 *                                                                                    scale - 1 formed in double, rounded to fp32 once)
 *                             v = f * s;  x = blend_mode == SONAR_CFG_BLEND_NONE ? v : blend(x, v, blend)       (SONAR_BLEND_*, as sonar_blend_f32)
 *                           FUSED transforms the whole plane before any of it is stored and reads the original value again (presumably an L2 hit: the
 *                           workgroup loaded the plane microseconds earlier; not measured) instead of keeping a second copy in LDS.  The hidden-mean launch
 *                           must precede this one on the same stream (it reads every channel, the slice's included).
 * SONAR_ERR_ARG: unknown dtype / mode / blend mode, a negative size, a channel window outside [0, C), a stride smaller than the plane, a
 * required pointer NULL or misaligned for its element type, mean without extremes. */
#define SONAR_FREEU_PLAIN 0
#define SONAR_FREEU_FUSED 1
#define SONAR_FREEU_FILTERED 2
int64_t sonar_freeu_hidden_mean_groups(int64_t B, int64_t C, int64_t HW);
int sonar_freeu_hidden_mean(int dtype, const void* x, int64_t B, int64_t C, int64_t HW, int64_t stride_b, int64_t stride_c, float* mean,
                            float* extremes, float* ws, int64_t ws_elems, void* stream);
int sonar_freeu_apply(int dtype, void* x, int64_t B, int64_t C, int64_t H, int64_t W, int64_t stride_b, int64_t stride_c, int64_t c0,
                      int64_t cn, int mode, const float* filter, const float* filtered, const float* mean, const float* extremes, double scale,
                      int blend_mode, float blend, void* stream);

/* ---------------------------------------------------------------- prepared call plans (host floor of rows C, G1, P, Y, PW) */
/* The reference composes a sampler step from Python closures (py/noise.py:137-257, py/noise_generation.py:134-258); at the batch sizes
 * a ComfyUI run uses (1-4, cfg3's 64) the interpreter work per step outweighs the kernels.  A plan is the step resolved once: the entry
 * points of this header it issues, in order, with their arguments.  sonar_plan_run patches the values that change from call to call into
 * the recorded arguments -- tensor addresses (slots), the RNG seed and stream ids, the pyramid's level table -- and calls the same entry
 * points: same launches, same bits, one foreign call per step.  Host-side objects; not thread safe per plan. */
typedef struct sonar_plan sonar_plan;
#define SONAR_PATCH_SLOT 0   /* slots[index] + addend: a device address (or scalar) handed to sonar_plan_run */
#define SONAR_PATCH_STREAM 1 /* stream_base + addend: an RNG stream id */
#define SONAR_PATCH_SEED 2   /* the RNG seed */
#define SONAR_PATCH_BLOB 3   /* address of byte `addend` of the record's blob (array and struct arguments) */
#define SONAR_PATCH_LEVELS 4 /* pyramid level table (sonar_plan_levels at blob offset `index`) recomputed from (seed, stream_base + addend);
                                the level count goes to argument `target` */
typedef struct sonar_plan_patch {
    int32_t source; /* SONAR_PATCH_* */
    int32_t target; /* >= 0: argument index; < 0: byte offset -(target + 1) into the record's blob */
    int32_t index;  /* SLOT: slot number; LEVELS: blob offset of the rule */
    int32_t width;  /* bytes written at a blob target: 4 or 8 */
    int64_t addend;
} sonar_plan_patch;
typedef struct sonar_plan_levels {
    int64_t H, W;
    double discount;
    int32_t iterations;
    int32_t reserved;
    int64_t h_offset, w_offset, weight_offset; /* blob offsets of the int64 / int64 / float tables (`iterations` entries each) */
} sonar_plan_levels;
/* index of a replayable entry point (one that only launches on its last argument, the stream) or -1; its argument count */
int sonar_plan_fn_id(const char* name);
int sonar_plan_fn_nargs(int fn_id);
sonar_plan* sonar_plan_create(int nslots);
void sonar_plan_destroy(sonar_plan* plan);
int sonar_plan_length(const sonar_plan* plan);
/* append one call: `args` = one 64-bit word per argument (integers sign-extended, float / double bit patterns, addresses), `blob` = bytes
 * the arguments point into (copied), `patches` = what sonar_plan_run rewrites before the call (the last argument, the stream, always is) */
int sonar_plan_add(sonar_plan* plan, int fn_id, const uint64_t* args, int nargs, const void* blob, int64_t blob_bytes,
                   const sonar_plan_patch* patches, int npatches);
/* issue every record on `stream`; stops at the first entry point that fails and returns its code (`failed_record`, nullable: its index,
 * -1 when all ran; sonar_last_error() is that entry point's message) */
int sonar_plan_run(sonar_plan* plan, const uint64_t* slots, int nslots, uint64_t seed, uint64_t stream_base, void* stream,
                   int* failed_record);
/* the level sizes and weights of a device-mode pyramid draw (py/noise_generation.py:609-649: r = rand * 2 + 2 per level from a host
 * splitmix64 sequence keyed by (seed, stream_id)); returns the level count.  Pure host arithmetic. */
int sonar_pyramid_levels(int64_t H, int64_t W, int iterations, double discount, uint64_t seed, uint64_t stream_id, int64_t* level_h,
                         int64_t* level_w, float* weight);

#ifdef __cplusplus
}
#endif
#endif /* SONAR_HIP_H */
