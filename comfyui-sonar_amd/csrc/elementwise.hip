// Whole-tensor streaming kernels: the (sum, sumsq) statistics and the global normalisation built on them (scale_noise, std_scale), and
// the pure streaming ops on ew_driver.h's driver: blends, chain accumulation (axpby, with statistics), affine, scalar, power law, mask
// mix, squared accumulation, Laplace, Student-t, the fp64 cast.  All HBM-bound: 16 B/lane coalesced accesses, fp64 block reductions.
#include <math.h>

#include "ew_driver.h"

namespace sonar {

// ------------------------------------------------------------------------------------------------
// stats: (sum, sumsq) partials in fp64
template <int V>
__global__ void __launch_bounds__(kBlock) stats_kernel(const float* __restrict__ x, int64_t n, double* partials) {
    kernarg_touch_for(x, n, partials);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    const int64_t nv = n / V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    // two independent loads in flight per iteration
    for (; i + stride < nv; i += 2 * stride) {
        const Pack<V> a = load<V>(x, i * V);
        const Pack<V> b = load<V>(x, (i + stride) * V);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double da = a.v[k], db = b.v[k];
            s += da; q += da * da;
            s += db; q += db * db;
        }
    }
    for (; i < nv; i += stride) {
        const Pack<V> a = load<V>(x, i * V);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double da = a.v[k];
            s += da; q += da * da;
        }
    }
    if (V > 1 && blockIdx.x == 0)
        for (int64_t j = nv * V + threadIdx.x; j < n; j += kBlock) {
            const double da = x[j];
            s += da; q += da * da;
        }
    write_partial<kBlock>(s, q, partials, red);
}

__global__ void __launch_bounds__(kBlock) stats_finalize_kernel(const double* __restrict__ partials, int64_t npart,
                                                                 int64_t n, double* out3) {
    kernarg_touch_for(partials, npart, n, out3);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    for (int64_t i = threadIdx.x; i < npart; i += kBlock) {
        s += partials[2 * i];
        q += partials[2 * i + 1];
    }
    block_sum2<kBlock>(s, q, red);
    if (threadIdx.x == 0) {
        out3[0] = s;
        out3[1] = q;
        out3[2] = (double)n;
    }
}

template <int V, bool NT = false /* common.h store4: launch-bound sizes */>
__global__ void __launch_bounds__(kBlock) scale_noise_kernel(float* x, int64_t n, float factor, int normalized,
                                                             float thr_sd, const double* __restrict__ partials,
                                                             int64_t npart, int64_t n_total, double* out_partials) {
    kernarg_touch_for(x, n, factor, normalized, thr_sd, partials, npart, n_total, out_partials);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    NormDecision d{0.f, 1.f, 0, 0};
    if (normalized) d = decide_norm<kBlock>(partials, npart, n_total, thr_sd, red, &sh);
    if (normalized == 2) {  // x *= factor / std (py/noise_generation.py:702): one multiplier, no mean shift
        factor = factor / d.stdv;
        d.do_sub = 0;
        d.do_div = 0;
    }
    const bool do_mul = factor != 1.0f;
    if (out_partials && blockIdx.x == 0) {
        // statistics of the RESULT, derived from the input's: y = ((x - m) / s) * f  ->  sum y = f (S - n m) / s,
        // sum y^2 = f^2 (Q - 2 m S + n m^2) / s^2.  A wrapper that normalises this tensor again reads them instead of the tensor.
        double S = 0.0, Q = 0.0;
        for (int64_t i = threadIdx.x; i < npart; i += kBlock) {
            S += partials[2 * i];
            Q += partials[2 * i + 1];
        }
        __syncthreads();
        block_sum2<kBlock>(S, Q, red);
        if (threadIdx.x == 0) {
            const double nt = (double)n_total, m = d.do_sub ? (double)d.mean : 0.0, sd = d.do_div ? (double)d.stdv : 1.0;
            const double f = do_mul ? (double)factor : 1.0;
            out_partials[0] = f * (S - nt * m) / sd;
            out_partials[1] = f * f * (Q - 2.0 * m * S + nt * m * m) / (sd * sd);
        }
        for (int j = 1 + threadIdx.x; j < kNPart; j += kBlock) {
            out_partials[2 * j] = 0.0;
            out_partials[2 * j + 1] = 0.0;
        }
    }
    if (!d.do_sub && !d.do_div && !do_mul) return;  // nothing to change (every block takes the same decision)
    const int64_t nv = n / V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    auto f = [&](float v) {
        if (d.do_sub) v = v - d.mean;
        if (d.do_div) v = v / d.stdv;
        if (do_mul) v = v * factor;
        return v;
    };
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < nv; i += 2 * stride) {
        Pack<V> a = load<V>(x, i * V);
        Pack<V> b = load<V>(x, (i + stride) * V);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            a.v[k] = f(a.v[k]);
            b.v[k] = f(b.v[k]);
        }
        store<V, NT>(x, i * V, a);
        store<V, NT>(x, (i + stride) * V, b);
    }
    for (; i < nv; i += stride) {
        Pack<V> a = load<V>(x, i * V);
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] = f(a.v[k]);
        store<V, NT>(x, i * V, a);
    }
    if (V > 1 && blockIdx.x == 0)
        for (int64_t j = nv * V + threadIdx.x; j < n; j += kBlock) x[j] = f(x[j]);
}

// ------------------------------------------------------------------------------------------------
struct BlendOp {
    int mode;
    const float *a, *b;
    float t;
    float* out;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> pa = load<V>(a, i), pb = load<V>(b, i);
        Pack<V> r;
#pragma unroll
        for (int k = 0; k < V; ++k) r.v[k] = blend<float>(mode, pa.v[k], pb.v[k], t);
        store<V>(out, i, r);
    }
};

struct BlendTensorOp {
    int mode;
    const float *a, *b, *t;
    int64_t tn;
    float* out;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> pa = load<V>(a, i), pb = load<V>(b, i);
        Pack<V> r;
#pragma unroll
        for (int k = 0; k < V; ++k) r.v[k] = blend<float>(mode, pa.v[k], pb.v[k], t[(i + k) % tn]);
        store<V>(out, i, r);
    }
};

struct AxpbyOp {
    float* y;
    float ymul;
    const float* x;
    float xmul;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> py = load<V>(y, i);
        const Pack<V> px = load<V>(x, i);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            // y*ymul and x*xmul are skipped when the multiplier is exactly 1 (the reference's
            // scale_noise/add_ sequence does not multiply then)
            const float yy = ymul != 1.0f ? py.v[k] * ymul : py.v[k];
            const float xx = xmul != 1.0f ? px.v[k] * xmul : px.v[k];
            py.v[k] = yy + xx;
        }
        store<V>(y, i, py);
    }
};

struct AffineOp {
    float* x;
    float sub, mul, add;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> p = load<V>(x, i);
#pragma unroll
        for (int k = 0; k < V; ++k) p.v[k] = (p.v[k] - sub) * mul + add;
        store<V>(x, i, p);
    }
};

struct ScalarOp {
    int op;
    const float *a, *b;
    float s;
    float* out;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> pa = load<V>(a, i);
        Pack<V> pb, r;
        if (op == 2) pb = load<V>(b, i);
#pragma unroll
        for (int k = 0; k < V; ++k) r.v[k] = op == 0 ? pa.v[k] * s : op == 1 ? pa.v[k] / s : (pa.v[k] - pb.v[k]) / s;
        store<V>(out, i, r);
    }
};

// LaplacianNoiseGenerator (py/noise_generation.py:789-802): x = x / div_fac + Laplace(loc, scale) with the Laplace variate built
// from a uniform u in (eps - 1, 1) exactly as torch.distributions.Laplace.rsample does: loc - scale * sign(u) * log1p(-|u|)
struct LaplaceAddOp {
    float* x;
    const float* u;
    float div_fac, loc, scale;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> p = load<V>(x, i);
        const Pack<V> pu = load<V>(u, i);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float uu = pu.v[k];
            const float a = fmaxf(fabsf(uu), 1.17549435e-38f);  // clamp(min=finfo.tiny)
            const float sgn = uu > 0.0f ? 1.0f : uu < 0.0f ? -1.0f : 0.0f;
            p.v[k] = p.v[k] / div_fac + (loc - scale * sgn * log1pf(-a));
        }
        store<V>(x, i, p);
    }
};

// ---- StudentTNoiseGenerator (py/noise_generation.py:652-677) --------------------------------------------------------------------
// x (a standard normal draw) -> loc + scale * x * rsqrt(max(g / 0.5, tiny) / df), g the torch._standard_gamma(df / 2) draw
// (torch.distributions.StudentT.rsample / Chi2 / Gamma.rsample)
struct StudentTOp {
    float* x;
    const float* g;
    float loc, scale, df;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> p = load<V>(x, i);
        const Pack<V> pg = load<V>(g, i);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float z = fmaxf(pg.v[k] / 0.5f, 1.17549435e-38f);
            p.v[k] = loc + scale * (p.v[k] * (1.0f / sqrtf(z / df)));
        }
        store<V>(x, i, p);
    }
};

// acc = (first ? 0 : acc) + mul * z^2: chi-square of an integer df built from squared normals (on-device StudentT draws)
struct SqAccOp {
    float* acc;
    const float* z;
    float mul;
    int first;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> a = load<V>(acc, i);
        const Pack<V> pz = load<V>(z, i);
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] = (first ? 0.0f : a.v[k]) + mul * (pz.v[k] * pz.v[k]);
        store<V>(acc, i, a);
    }
};

// y = y*ymul + x*xmul with the (sum, sumsq) partials of the result: the last accumulation of a noise chain feeds the chain's
// normalisation without a separate statistics sweep
__global__ void __launch_bounds__(kBlock) axpby_stats_kernel(float* y, float ymul, const float* __restrict__ x, float xmul, int64_t n,
                                                              double* partials) {
    kernarg_touch_for(y, ymul, x, xmul, n, partials);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    const int64_t nv = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nv; i += (int64_t)gridDim.x * kBlock) {
        Pack<4> py = load<4>(y, i * 4);
        const Pack<4> px = load<4>(x, i * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float yy = ymul != 1.0f ? py.v[k] * ymul : py.v[k];
            const float xx = xmul != 1.0f ? px.v[k] * xmul : px.v[k];
            const float v = yy + xx;
            py.v[k] = v;
            s += (double)v;
            q += (double)v * (double)v;
        }
        store<4>(y, i * 4, py);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nv * 4; i < n; ++i) {
            const float v = (ymul != 1.0f ? y[i] * ymul : y[i]) + (xmul != 1.0f ? x[i] * xmul : x[i]);
            y[i] = v;
            s += (double)v;
            q += (double)v * (double)v;
        }
    write_partial<kBlock>(s, q, partials, red);
}

struct PowerLawOp {
    float* x;
    float alpha;
    int use_sign;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Pack<V> p = load<V>(x, i);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float v = p.v[k];
            const float av = fabsf(v);  // ATen special-cases these exponents (pow_tensor_scalar), keep them exact
            const float mod = alpha == 0.0f ? 1.0f : alpha == 1.0f ? av : alpha == 0.5f ? sqrtf(av) : alpha == 2.0f ? av * av : powf(av, alpha);
            const float base = use_sign ? (v > 0.0f ? 1.0f : v < 0.0f ? -1.0f : v) : v;  // torch.sign keeps 0 and NaN
            p.v[k] = base * mod;
        }
        store<V>(x, i, p);
    }
};

struct MaskMixOp {
    const float *dst, *src, *mask;
    int64_t mask_n;
    float* out;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> pd = load<V>(dst, i), ps = load<V>(src, i);
        Pack<V> r;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float m = mask[(i + k) % mask_n];
            // py/noise.py:528-530: noise_dst *= (1 - mask); noise_src *= mask; dst + src
            r.v[k] = pd.v[k] * (1.0f - m) + ps.v[k] * m;
        }
        store<V>(out, i, r);
    }
};

struct CastOp {
    const float* in;
    double* out;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        const Pack<V> p = load<V>(in, i);
        if constexpr (V == 4) {
            *reinterpret_cast<double2*>(out + i) = make_double2((double)p.v[0], (double)p.v[1]);
            *reinterpret_cast<double2*>(out + i + 2) = make_double2((double)p.v[2], (double)p.v[3]);
        } else {
            out[i] = (double)p.v[0];
        }
    }
};

}  // namespace sonar

using namespace sonar;

// ================================================================================================
extern "C" int sonar_stats_f32(const float* x, int64_t n, double* partials, void* stream) {
    SONAR_REQUIRE(x && partials && n >= 0, SONAR_ERR_ARG, "sonar_stats_f32: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(x)) {
        const int g = (int)std::min<int64_t>(kNPart, grid_for(n / 4 + 1, kBlock * 2));
        hipLaunchKernelGGL((stats_kernel<4>), dim3(g), dim3(kBlock), 0, st, x, n, partials);
    } else {
        const int g = (int)std::min<int64_t>(kNPart, grid_for(n, kBlock * 4));
        hipLaunchKernelGGL((stats_kernel<1>), dim3(g), dim3(kBlock), 0, st, x, n, partials);
    }
    return check_launch("sonar_stats_f32");
}

extern "C" int sonar_stats_finalize(const double* partials, int64_t npart, int64_t n, double* out3, void* stream) {
    SONAR_REQUIRE(partials && out3 && npart > 0, SONAR_ERR_ARG, "sonar_stats_finalize: bad argument");
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, partials, npart, n, out3);
    return check_launch("sonar_stats_finalize");
}

static int scale_noise_launch(float* x, int64_t n, float factor, int normalized, float threshold_std_devs, const double* partials,
                              int64_t npart, int64_t n_total, double* out_partials, void* stream) {
    SONAR_REQUIRE(x && n >= 0, SONAR_ERR_ARG, "sonar_scale_noise_f32: bad argument");
    SONAR_REQUIRE(!normalized || (partials && npart > 0 && n_total > 0), SONAR_ERR_ARG,
                  "sonar_scale_noise_f32: normalized=1 needs partials");
    SONAR_REQUIRE(!out_partials || (normalized && out_partials != partials), SONAR_ERR_ARG,
                  "sonar_scale_noise_stats_f32: result statistics need normalized=1 and a separate buffer");
    if (n == 0 || (!normalized && factor == 1.0f)) return SONAR_OK;
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(x) && nt_stores_host(n)) {
        hipLaunchKernelGGL((scale_noise_kernel<4, true>), dim3(grid_for(n / 4 + 1, kBlock * 2)), dim3(kBlock), 0, st, x, n,
                           factor, normalized, threshold_std_devs, partials, npart, n_total, out_partials);
    } else if (aligned16(x)) {
        hipLaunchKernelGGL((scale_noise_kernel<4>), dim3(grid_for(n / 4 + 1, kBlock * 2)), dim3(kBlock), 0, st, x, n,
                           factor, normalized, threshold_std_devs, partials, npart, n_total, out_partials);
    } else {
        hipLaunchKernelGGL((scale_noise_kernel<1>), dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, st, x, n, factor,
                           normalized, threshold_std_devs, partials, npart, n_total, out_partials);
    }
    return check_launch("sonar_scale_noise_f32");
}

extern "C" int sonar_scale_noise_f32(float* x, int64_t n, float factor, int normalized, float threshold_std_devs,
                                     const double* partials, int64_t npart, int64_t n_total, void* stream) {
    return scale_noise_launch(x, n, factor, normalized, threshold_std_devs, partials, npart, n_total, nullptr, stream);
}

extern "C" int sonar_scale_noise_stats_f32(float* x, int64_t n, float factor, float threshold_std_devs, const double* partials,
                                           int64_t npart, int64_t n_total, double* out_partials, void* stream) {
    SONAR_REQUIRE(out_partials, SONAR_ERR_ARG, "sonar_scale_noise_stats_f32: bad argument");
    return scale_noise_launch(x, n, factor, 1, threshold_std_devs, partials, npart, n_total, out_partials, stream);
}

extern "C" int sonar_std_scale_f32(float* x, int64_t n, float mul, const double* partials, int64_t npart, int64_t n_total,
                                   void* stream) {
    SONAR_REQUIRE(x && partials && n >= 0 && npart > 0 && n_total >= 1, SONAR_ERR_ARG, "sonar_std_scale_f32: bad argument");  // one element: its std is NaN, as in torch
    if (n == 0) return SONAR_OK;
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(x))
        hipLaunchKernelGGL((scale_noise_kernel<4>), dim3(grid_for(n / 4 + 1, kBlock * 2)), dim3(kBlock), 0, st, x, n, mul, 2, 0.0f,
                           partials, npart, n_total, (double*)nullptr);
    else
        hipLaunchKernelGGL((scale_noise_kernel<1>), dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, st, x, n, mul, 2, 0.0f, partials,
                           npart, n_total, (double*)nullptr);
    return check_launch("sonar_std_scale_f32");
}

extern "C" int sonar_blend_f32(int mode, const float* a, const float* b, float t, float* out, int64_t n, void* stream) {
    SONAR_REQUIRE(a && b && out && n >= 0 && mode >= 0 && mode <= 2, SONAR_ERR_ARG, "sonar_blend_f32: bad argument");
    return launch_ew(BlendOp{mode, a, b, t, out}, n, aligned16(a) && aligned16(b) && aligned16(out),
                     (hipStream_t)stream, "sonar_blend_f32");
}

extern "C" int sonar_blend_tensor_f32(int mode, const float* a, const float* b, const float* t, int64_t tn, float* out,
                                      int64_t n, void* stream) {
    SONAR_REQUIRE(a && b && t && out && n >= 0 && tn > 0 && mode >= 0 && mode <= 2, SONAR_ERR_ARG,
                  "sonar_blend_tensor_f32: bad argument");
    return launch_ew(BlendTensorOp{mode, a, b, t, tn, out}, n, aligned16(a) && aligned16(b) && aligned16(out),
                     (hipStream_t)stream, "sonar_blend_tensor_f32");
}

extern "C" int sonar_axpby_stats_f32(float* y, float ymul, const float* x, float xmul, int64_t n, double* partials, void* stream) {
    SONAR_REQUIRE(x && y && partials && n >= 0 && aligned16(x) && aligned16(y), SONAR_ERR_ARG,
                  "sonar_axpby_stats_f32: bad argument (16-byte aligned buffers required)");
    const int g = (int)std::min<int64_t>(kNPart, std::max<int64_t>(1, grid_for(n / 4 + 1, kBlock)));
    hipLaunchKernelGGL(axpby_stats_kernel, dim3(g), dim3(kBlock), 0, (hipStream_t)stream, y, ymul, x, xmul, n, partials);
    return check_launch("sonar_axpby_stats_f32");
}

extern "C" int sonar_axpby_f32(float* y, float ymul, const float* x, float xmul, int64_t n, void* stream) {
    SONAR_REQUIRE(x && y && n >= 0, SONAR_ERR_ARG, "sonar_axpby_f32: bad argument");
    return launch_ew(AxpbyOp{y, ymul, x, xmul}, n, aligned16(x) && aligned16(y), (hipStream_t)stream, "sonar_axpby_f32");
}

extern "C" int sonar_affine_f32(float* x, float sub, float mul, float add, int64_t n, void* stream) {
    SONAR_REQUIRE(x && n >= 0, SONAR_ERR_ARG, "sonar_affine_f32: bad argument");
    return launch_ew(AffineOp{x, sub, mul, add}, n, aligned16(x), (hipStream_t)stream, "sonar_affine_f32");
}

extern "C" int sonar_scalar_op_f32(int op, const float* a, const float* b, float s, float* out, int64_t n, void* stream) {
    SONAR_REQUIRE(a && out && n >= 0 && op >= 0 && op <= 2 && (op != 2 || b), SONAR_ERR_ARG, "sonar_scalar_op_f32: bad argument");
    return launch_ew(ScalarOp{op, a, b, s, out}, n, aligned16(a) && aligned16(out) && (!b || aligned16(b)), (hipStream_t)stream,
                     "sonar_scalar_op_f32");
}

extern "C" int sonar_powerlaw_f32(float* x, float alpha, int use_sign, int64_t n, void* stream) {
    SONAR_REQUIRE(x && n >= 0, SONAR_ERR_ARG, "sonar_powerlaw_f32: bad argument");
    return launch_ew(PowerLawOp{x, alpha, use_sign}, n, aligned16(x), (hipStream_t)stream, "sonar_powerlaw_f32");
}

extern "C" int sonar_laplace_add_f32(float* x, const float* u, float div_fac, float loc, float scale, int64_t n, void* stream) {
    SONAR_REQUIRE(x && u && n >= 0 && div_fac != 0.0f, SONAR_ERR_ARG, "sonar_laplace_add_f32: bad argument");
    return launch_ew(LaplaceAddOp{x, u, div_fac, loc, scale}, n, aligned16(x) && aligned16(u), (hipStream_t)stream, "sonar_laplace_add_f32");
}

extern "C" int sonar_studentt_f32(float* x, const float* gamma, float loc, float scale, float df, int64_t n, void* stream) {
    SONAR_REQUIRE(x && gamma && n >= 0 && df > 0.0f, SONAR_ERR_ARG, "sonar_studentt_f32: bad argument");
    return launch_ew(StudentTOp{x, gamma, loc, scale, df}, n, aligned16(x) && aligned16(gamma), (hipStream_t)stream, "sonar_studentt_f32");
}

extern "C" int sonar_sq_acc_f32(float* acc, const float* z, float mul, int first, int64_t n, void* stream) {
    SONAR_REQUIRE(acc && z && n >= 0, SONAR_ERR_ARG, "sonar_sq_acc_f32: bad argument");
    return launch_ew(SqAccOp{acc, z, mul, first}, n, aligned16(acc) && aligned16(z), (hipStream_t)stream, "sonar_sq_acc_f32");
}

extern "C" int sonar_mask_mix_f32(const float* dst, const float* src, const float* mask, int64_t mask_n, float* out,
                                  int64_t n, void* stream) {
    SONAR_REQUIRE(dst && src && mask && out && n >= 0 && mask_n > 0, SONAR_ERR_ARG, "sonar_mask_mix_f32: bad argument");
    return launch_ew(MaskMixOp{dst, src, mask, mask_n, out}, n, aligned16(dst) && aligned16(src) && aligned16(out),
                     (hipStream_t)stream, "sonar_mask_mix_f32");
}

extern "C" int sonar_cast_f32_f64(const float* in, double* out, int64_t n, void* stream) {
    SONAR_REQUIRE(in && out && n >= 0, SONAR_ERR_ARG, "sonar_cast_f32_f64: bad argument");
    return launch_ew(CastOp{in, out}, n, aligned16(in) && aligned16(out), (hipStream_t)stream, "sonar_cast_f32_f64");
}
