// The fused Sonar momentum sampler steps on ew_driver.h's driver: Euler and the two DPM++ stages with the history update in
// registers, and the pending global normalisation of their noise operand (norm_decision, apply_norm), which the step kernels
// apply on the fly.
#include <math.h>

#include "ew_driver.h"

namespace sonar {

// ------------------------------------------------------------------------------------------------
// Momentum building blocks (py/sonar.py:227-307), evaluated per element in registers.
struct HistState {
    float h;
    bool present;
};

// update_hist: h <- v                       when no history yet
//              h <- hblend(v*ms, h*hs, hr)  otherwise          (py/sonar.py:231-236)
__device__ __forceinline__ void hist_update(const sonar_momentum_cfg& c, HistState& hs, float v) {
    if (!c.update_hist) return;
    if (!hs.present) {
        hs.h = v;
        hs.present = true;
    } else {
        hs.h = blend<float>(c.history_blend, v * c.md_scale, hs.h * c.hist_scale, c.hist_ratio);
    }
}

// init_hist_d for SAMPLE / SAMPLE_NORM (py/sonar.py:184-191)
__device__ __forceinline__ void hist_init(const sonar_momentum_cfg& c, HistState& hs, float x, float den, float sigma) {
    if (hs.present || c.init_kind == SONAR_INIT_NONE) return;
    const float src = c.mode == SONAR_MODE_DENOISED ? den : x;
    hs.h = c.init_kind == SONAR_INIT_SAMPLE_NORM ? src / sigma : src;
    hs.present = true;
}

// get_momentum_denoised (py/sonar.py:262-283): returns den_m, updates history with den/sigma
__device__ __forceinline__ float momentum_denoised(const sonar_momentum_cfg& c, HistState& hs, bool h_usable, float x,
                                                   float den, float sigma) {
    float den_m = den;
    if (c.mode == SONAR_MODE_DENOISED && hs.present && h_usable && c.momentum != 1.0f)
        den_m = blend<float>(c.momentum_blend, hs.h * sigma, den, c.momentum);
    hist_init(c, hs, x, den, sigma);
    hist_update(c, hs, den / sigma);
    return c.use_momentum ? den_m : den;
}

// get_momentum_d (py/sonar.py:285-307) for a given d; `early_out` = momentum==1 || DENOISED mode
__device__ __forceinline__ float momentum_d(const sonar_momentum_cfg& c, HistState& hs, bool early_out, float x,
                                            float den, float sigma, float d) {
    if (early_out) return d;
    const float md = hs.present ? blend<float>(c.momentum_blend, hs.h, d, c.momentum) : d;
    hist_init(c, hs, x, den, sigma);
    hist_update(c, hs, c.mode == SONAR_MODE_NEW ? d : md);
    return c.use_momentum ? md : d;
}

// A noise tensor whose global normalisation (py/utils.py:100-105) is still pending: the decision -- taken on the device from the
// tensor's (sum, sumsq) partials by sonar_norm_decision_f32 -- rides along and the step kernel that consumes the noise applies it on
// the fly, with scale_noise_kernel's own operation sequence (subtract, divide, multiply: same bits), instead of a separate read +
// write of the tensor.
// The quotient v / std without the ten-instruction IEEE division sequence per element: std is the same for every element, so its
// correctly rounded reciprocal is taken once (sonar_norm_decision_f32) and one residual step q' = q + (v - std q) / std on q = v / std
// gives the correctly rounded quotient (Markstein: exact remainder by fma, correctly rounded reciprocal) for every v in the normal
// range -- the same bits as scale_noise_kernel's `v / std`, at three instructions.
struct PendingNorm {  // one thread's copy of the decision (read once per item, not once per element)
    float mean, stdv, inv_std, factor;
    bool sub, div, mul;
    __device__ __forceinline__ explicit PendingNorm(const sonar_noise_norm* __restrict__ nn) {
        if (nn) {
            mean = nn->mean; stdv = nn->stdv; inv_std = nn->inv_std; factor = nn->factor;
            sub = nn->do_sub != 0; div = nn->do_div != 0; mul = factor != 1.0f;
        } else {
            mean = 0.0f; stdv = inv_std = factor = 1.0f;
            sub = div = mul = false;
        }
    }
    __device__ __forceinline__ float operator()(float v) const {
        if (sub) v = v - mean;
        if (div) {
            const float q = v * inv_std;
            v = __builtin_fmaf(__builtin_fmaf(-stdv, q, v), inv_std, q);
        }
        if (mul) v = v * factor;
        return v;
    }
};

__global__ void __launch_bounds__(kBlock) norm_decision_kernel(const double* __restrict__ partials, int64_t npart, int64_t n_total, float factor,
                                                                float thr_sd, sonar_noise_norm* out) {
    kernarg_touch_for(partials, npart, n_total, factor, thr_sd, out);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    const NormDecision d = decide_norm<kBlock>(partials, npart, n_total, thr_sd, red, &sh);
    if (threadIdx.x == 0) {
        out->mean = d.mean;
        out->stdv = d.stdv;
        out->inv_std = 1.0f / d.stdv;  // correctly rounded (IEEE division), once
        out->factor = factor;
        out->do_sub = d.do_sub;
        out->do_div = d.do_div;
    }
}

struct ApplyNormOp {
    float* x;
    const sonar_noise_norm* nn;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> p = load<V>(x, i);
        const PendingNorm pending(nn);
#pragma unroll
        for (int k = 0; k < V; ++k) p.v[k] = pending(p.v[k]);
        store<V>(x, i, p);
    }
};

// NT: both outputs stored with the non-temporal hint -- for a streaming kernel with three inputs and two outputs the lines are better off
// not sitting in the L2 (512 SDXL latents: 120 -> 115 us; at 64 latents and below the write-back cache wins by a little)
template <bool NT>
struct EulerOpT {
    const float *x, *den, *h_in;
    float *x_out, *h_out;
    const float* noise;
    const sonar_noise_norm* noise_norm;
    float noise_scale, sigma, dt;
    sonar_momentum_cfg c;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> px = load<V>(x, i), pd = load<V>(den, i);
        Pack<V> ph, pn, rx, rh;
        if (h_in) ph = load<V>(h_in, i);
        if (noise) pn = load<V>(noise, i);
        const bool early = c.momentum == 1.0f || c.mode == SONAR_MODE_DENOISED;
        const PendingNorm pending(noise_norm);
        bool present = false;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            HistState hs{h_in ? ph.v[k] : 0.0f, h_in != nullptr};
            const float den_m = momentum_denoised(c, hs, !c.h_in_fresh, px.v[k], pd.v[k], sigma);
            const float d = (px.v[k] - den_m) / sigma;  // to_d
            const float md = momentum_d(c, hs, early, px.v[k], den_m, sigma, d);
            float xn = md * dt + px.v[k];
            if (noise) xn = xn + pending(pn.v[k]) * noise_scale;
            rx.v[k] = xn;
            rh.v[k] = hs.h;
            present = hs.present;
        }
        store<V, NT>(x_out, i, rx);
        if (present && h_out) store<V, NT>(h_out, i, rh);
    }
};
using EulerOp = EulerOpT<false>;

struct Dpmpp1Op {
    const float *x, *den, *h_in;
    float *x2_out, *md1_out, *h_out;
    const float* noise;
    const sonar_noise_norm* noise_norm;
    float noise_scale, sigma, expm1_a, ratio_a;
    int adj_is_one;
    sonar_momentum_cfg c;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> px = load<V>(x, i), pd = load<V>(den, i);
        Pack<V> ph, pn, rx, rm, rh;
        if (h_in) ph = load<V>(h_in, i);
        if (noise) pn = load<V>(noise, i);
        const bool early = adj_is_one || c.mode == SONAR_MODE_DENOISED;
        const PendingNorm pending(noise_norm);
        bool present = false;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            HistState hs{h_in ? ph.v[k] : 0.0f, h_in != nullptr};
            const float md1 = momentum_denoised(c, hs, !c.h_in_fresh, px.v[k], pd.v[k], sigma);
            const float diff2 = expm1_a * md1;
            const float m_d = momentum_d(c, hs, early, px.v[k], md1, sigma, diff2);
            float x2 = ratio_a * px.v[k] - m_d;
            if (noise) x2 = x2 + pending(pn.v[k]) * noise_scale;
            rx.v[k] = x2;
            rm.v[k] = md1;
            rh.v[k] = hs.h;
            present = hs.present;
        }
        store<V>(x2_out, i, rx);
        store<V>(md1_out, i, rm);
        if (present && h_out) store<V>(h_out, i, rh);
    }
};

struct Dpmpp2Op {
    const float *x, *den2, *md1, *h_in;
    float *x_out, *dd_out, *h_out;
    const float* noise;
    const sonar_noise_norm* noise_norm;
    float noise_scale, sigma_s, expm1_b, ratio_b, fac;
    int adj_is_one;
    sonar_momentum_cfg c;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> px = load<V>(x, i), pd = load<V>(den2, i), pm = load<V>(md1, i);
        Pack<V> ph, pn, rx, rd, rh;
        if (h_in) ph = load<V>(h_in, i);
        if (noise) pn = load<V>(noise, i);
        const bool early = adj_is_one || c.mode == SONAR_MODE_DENOISED;
        const float one_minus_fac = 1.0f - fac;
        const PendingNorm pending(noise_norm);
        bool present = false;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            HistState hs{h_in ? ph.v[k] : 0.0f, h_in != nullptr};
            const float md2 = momentum_denoised(c, hs, true, px.v[k], pd.v[k], sigma_s);
            const float dd = one_minus_fac * pm.v[k] + fac * md2;
            const float diff1 = expm1_b * dd;
            const float m_d = momentum_d(c, hs, early, px.v[k], md2, sigma_s, diff1);
            float xn = ratio_b * px.v[k] - m_d;
            if (noise) xn = xn + pending(pn.v[k]) * noise_scale;
            rx.v[k] = xn;
            rd.v[k] = dd;
            rh.v[k] = hs.h;
            present = hs.present;
        }
        store<V>(x_out, i, rx);
        if (dd_out) store<V>(dd_out, i, rd);
        if (present && h_out) store<V>(h_out, i, rh);
    }
};

// Whether a history exists after the step (host-side mirror of the device logic).
static int hist_present_after(const sonar_momentum_cfg& c, bool h_in, bool second_update_possible) {
    if (h_in) return 1;
    if (c.init_kind != SONAR_INIT_NONE) return 1;
    if (c.update_hist) return 1;
    (void)second_update_possible;
    return 0;
}

}  // namespace sonar

using namespace sonar;

// ================================================================================================
static bool cfg_ok(const sonar_momentum_cfg* c) {
    return c && c->mode >= 0 && c->mode <= 2 && c->momentum_blend >= 0 && c->momentum_blend <= 2 &&
           c->history_blend >= 0 && c->history_blend <= 2 && c->init_kind >= 0 && c->init_kind <= 2;
}

extern "C" int sonar_momentum_euler_f32(const float* x, const float* denoised, const float* h_in, float* x_out,
                                        float* h_out, const float* noise, float noise_scale, float sigma, float dt,
                                        const sonar_momentum_cfg* cfg, int64_t n, int* h_out_present,
                                        const sonar_noise_norm* noise_norm, void* stream) {
    SONAR_REQUIRE(x && denoised && x_out && n >= 0 && cfg_ok(cfg), SONAR_ERR_ARG, "sonar_momentum_euler_f32: bad argument");
    const int present = hist_present_after(*cfg, h_in != nullptr, true);
    SONAR_REQUIRE(!present || h_out, SONAR_ERR_ARG, "sonar_momentum_euler_f32: h_out required (history is produced)");
    if (h_out_present) *h_out_present = present;
    const bool v = aligned16(x) && aligned16(denoised) && aligned16(x_out) && (!h_in || aligned16(h_in)) &&
                   (!h_out || aligned16(h_out)) && (!noise || aligned16(noise));
    if (v && !nt_stores_host(n))  // beyond 32 MiB: streaming stores
        return launch_ew(EulerOpT<true>{x, denoised, h_in, x_out, h_out, noise, noise ? noise_norm : nullptr, noise_scale, sigma, dt, *cfg}, n, v,
                         (hipStream_t)stream, "sonar_momentum_euler_f32");
    return launch_ew(EulerOp{x, denoised, h_in, x_out, h_out, noise, noise ? noise_norm : nullptr, noise_scale, sigma, dt, *cfg}, n, v,
                     (hipStream_t)stream, "sonar_momentum_euler_f32");
}

extern "C" int sonar_dpmpp_stage1_f32(const float* x, const float* denoised, const float* h_in, float* x2_out,
                                      float* md1_out, float* h_out, const float* noise, float noise_scale, float sigma,
                                      float expm1_a, float ratio_a, int adj_is_one, const sonar_momentum_cfg* cfg,
                                      int64_t n, int* h_out_present, const sonar_noise_norm* noise_norm, void* stream) {
    SONAR_REQUIRE(x && denoised && x2_out && md1_out && n >= 0 && cfg_ok(cfg), SONAR_ERR_ARG,
                  "sonar_dpmpp_stage1_f32: bad argument");
    const int present = hist_present_after(*cfg, h_in != nullptr, true);
    SONAR_REQUIRE(!present || h_out, SONAR_ERR_ARG, "sonar_dpmpp_stage1_f32: h_out required");
    if (h_out_present) *h_out_present = present;
    const bool v = aligned16(x) && aligned16(denoised) && aligned16(x2_out) && aligned16(md1_out) &&
                   (!h_in || aligned16(h_in)) && (!h_out || aligned16(h_out)) && (!noise || aligned16(noise));
    return launch_ew(Dpmpp1Op{x, denoised, h_in, x2_out, md1_out, h_out, noise, noise ? noise_norm : nullptr, noise_scale, sigma, expm1_a, ratio_a,
                              adj_is_one, *cfg},
                     n, v, (hipStream_t)stream, "sonar_dpmpp_stage1_f32");
}

extern "C" int sonar_dpmpp_stage2_f32(const float* x, const float* denoised2, const float* md1, const float* h_in,
                                      float* x_out, float* dd_out, float* h_out, const float* noise, float noise_scale,
                                      float sigma_s, float expm1_b, float ratio_b, float fac, int adj_is_one,
                                      const sonar_momentum_cfg* cfg, int64_t n, int* h_out_present,
                                      const sonar_noise_norm* noise_norm, void* stream) {
    SONAR_REQUIRE(x && denoised2 && md1 && x_out && n >= 0 && cfg_ok(cfg), SONAR_ERR_ARG,
                  "sonar_dpmpp_stage2_f32: bad argument");
    const int present = hist_present_after(*cfg, h_in != nullptr, true);
    SONAR_REQUIRE(!present || h_out, SONAR_ERR_ARG, "sonar_dpmpp_stage2_f32: h_out required");
    if (h_out_present) *h_out_present = present;
    const bool v = aligned16(x) && aligned16(denoised2) && aligned16(md1) && aligned16(x_out) &&
                   (!dd_out || aligned16(dd_out)) && (!h_in || aligned16(h_in)) && (!h_out || aligned16(h_out)) &&
                   (!noise || aligned16(noise));
    return launch_ew(Dpmpp2Op{x, denoised2, md1, h_in, x_out, dd_out, h_out, noise, noise ? noise_norm : nullptr, noise_scale, sigma_s, expm1_b,
                              ratio_b, fac, adj_is_one, *cfg},
                     n, v, (hipStream_t)stream, "sonar_dpmpp_stage2_f32");
}

extern "C" int sonar_norm_decision_f32(const double* partials, int64_t npart, int64_t n_total, float factor, float threshold_std_devs,
                                       sonar_noise_norm* out, void* stream) {
    SONAR_REQUIRE(partials && out && npart > 0 && n_total > 1, SONAR_ERR_ARG, "sonar_norm_decision_f32: bad argument");
    hipLaunchKernelGGL(norm_decision_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, partials, npart, n_total, factor, threshold_std_devs,
                       out);
    return check_launch("sonar_norm_decision_f32");
}

extern "C" int sonar_apply_norm_f32(float* x, int64_t n, const sonar_noise_norm* norm, void* stream) {
    SONAR_REQUIRE(x && norm && n >= 0, SONAR_ERR_ARG, "sonar_apply_norm_f32: bad argument");
    return launch_ew(ApplyNormOp{x, norm}, n, aligned16(x), (hipStream_t)stream, "sonar_apply_norm_f32");
}
