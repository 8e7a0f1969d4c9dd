// Distro noise, generate mode (DistroNoiseGenerator, py/noise_generation.py:805-1256): one fp32 value per output element, the selected
// component of one draw of a torch.distributions family.  Each element owns its Philox4x32-10 blocks (counter = element index, block
// number): values do not depend on the launch geometry or on how a batch is sharded.  Block allotment and word conversions are the
// stream contract of INTEGRATION.md 3b; tests/test_gpu_distro.py restates the fixed-word families in numpy and tests/distro_refs.py the
// rejection-sampled ones (gamma_draw, poisson_draw, vonmises_draw), proposal by proposal, in fp64.
#include <float.h>
#include <math.h>

#include <utility>

#include "common.h"

namespace sonar {

namespace {

constexpr int kMaxProposals = SONAR_DISTRO_MAX_PROPOSALS;
constexpr int kMaxEvent = SONAR_DISTRO_MAX_EVENT;
constexpr uint32_t kGammaBlock0 = 64;  // gamma slot s proposes from blocks kGammaBlock0 + 64 s + j, j < kMaxProposals
constexpr uint32_t kRowBlocks = 8;     // matrix families: normal (i, j) of the row-major lower triangle is block i * 8 + j
static_assert(kRowBlocks * kRowBlocks <= kGammaBlock0, "the matrix normals stay below the gamma slots");

struct DistroKey {
    uint32_t c0, c1, c2, k0, k1;  // counter words except the block number, key
    __device__ __forceinline__ DistroKey(uint64_t seed, uint64_t stream_id, uint64_t idx)
        : c0((uint32_t)idx), c1((uint32_t)(idx >> 32) | ((uint32_t)(stream_id >> 32) << 16)), c2((uint32_t)stream_id),
          k0((uint32_t)seed), k1((uint32_t)(seed >> 32) ^ SONAR_DISTRO_DOMAIN) {}
    __device__ __forceinline__ Philox4 block(uint32_t b) const { return philox4x32_10(c0, c1, b, c2, k0, k1); }
};

__device__ __forceinline__ float u_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }  // (0, 1), exact: 24 bits
__device__ __forceinline__ float u_half(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }            // [0, 1)
// Box-Muller, cosine branch, from words 0 and 1 of a block
__device__ __forceinline__ float normal_of(const Philox4& p) { return sqrtf(-2.0f * logf(u_open(p.v[0]))) * cospif(2.0f * u_half(p.v[1])); }
__device__ __forceinline__ float normal_at(const DistroKey& key, uint32_t b) { return normal_of(key.block(b)); }

// Gamma(alpha, 1) (Marsaglia-Tsang; alpha < 1 boosted as Gamma(alpha + 1) * U^(1 / alpha), formed in log space).  Proposal j takes block
// first + j: words 0, 1 the normal, word 2 the acceptance uniform, word 3 of the accepted block the boost uniform.  After kMaxProposals
// rejections the value is d = alpha' - 1/3 (the proposal's centre).  Clamped to FLT_MIN as torch's sampler is.
__device__ __forceinline__ float gamma_draw(const DistroKey& key, uint32_t slot, float alpha) {
    const uint32_t first = kGammaBlock0 + slot * kMaxProposals;
    const bool boost = alpha < 1.0f;
    const float a = boost ? alpha + 1.0f : alpha;
    const float d = a - 1.0f / 3.0f;
    const float c = 1.0f / sqrtf(9.0f * d);
    float g = d, ub = 0.5f;
    for (int j = 0; j < kMaxProposals; ++j) {
        const Philox4 p = key.block(first + j);
        const float x = normal_of(p);
        const float t = 1.0f + c * x;
        if (t <= 0.0f) continue;
        const float v = t * t * t;
        const float u = u_open(p.v[2]);
        if (logf(u) < 0.5f * x * x + d - d * v + d * logf(v)) {
            g = d * v;
            ub = u_open(p.v[3]);
            break;
        }
    }
    if (boost) g = expf(logf(g) + logf(ub) / alpha);
    return fmaxf(g, FLT_MIN);
}

// Poisson: inversion of one uniform below rate 10 (the CDF summed in double), Hoermann's PTRS above (proposal j: block j, words 0 and 1;
// after kMaxProposals rejections floor(rate)).  k and the slow-path inequality are formed in double: both add terms of the size of
// rate log(rate) to terms of size 1, which fp32 loses from rate ~1e3 up (the pmf fails a chi-square at 1e5).  The squeeze stays fp32.
__device__ __forceinline__ float poisson_draw(const DistroKey& key, float rate) {
    if (rate < 10.0f) {
        const double u = (double)u_half(key.block(0).v[0]);
        double pk = exp(-(double)rate), cdf = pk;
        int k = 0;
        for (; k < kMaxProposals && u >= cdf; ++k) {  // the cap: P(X > 64) < 1e-25 at rate 10
            pk *= (double)rate / (double)(k + 1);
            cdf += pk;
        }
        return (float)k;
    }
    const float slam = sqrtf(rate);
    const double drate = (double)rate, dloglam = log(drate);
    const float b = 0.931f + 2.53f * slam, a = -0.059f + 0.02483f * b;
    const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f), vr = 0.9277f - 3.6224f / (b - 2.0f);
    for (int j = 0; j < kMaxProposals; ++j) {
        const Philox4 p = key.block(j);
        const float U = u_open(p.v[0]) - 0.5f, V = u_open(p.v[1]);
        const float us = 0.5f - fabsf(U);
        const float k = (float)floor((double)((2.0f * a / us + b) * U) + drate + 0.43);
        if (us >= 0.07f && V <= vr) return k;
        if (k < 0.0f || (us < 0.013f && V > us)) continue;
        if ((double)(logf(V) + logf(inv_alpha) - logf(a / (us * us) + b)) <= -drate + (double)k * dloglam - lgamma((double)k + 1.0)) return k;
    }
    return floorf(rate);
}

// von Mises (Best-Fisher, torch's _rejection_sample): proposal j takes block j, words 0-2; wrapped to [-pi, pi) as torch does.  After
// kMaxProposals rejections the offset from loc is 0 (the mode).  With z = cos(pi u) and f = (1 + r z) / (r + z), torch's c = conc (r - f)
// and acos(f) cancel for large conc (r - 1 ~ 1 / (2 conc)) and acos loses half its digits at both ends.  The host passes rm1 = r - 1 from
// double and everything is formed from 1 - z = 2 sin^2(pi u / 2) and 1 + z = 2 cos^2(pi u / 2): r + z = rm1 + (1 + z),
// 1 - f = rm1 (1 - z) / (r + z), 1 + f = (r + 1) (1 + z) / (r + z), c = conc (rm1 + (1 - f)), angle = 2 atan2(sqrt(1 - f), sqrt(1 + f)).
__device__ __forceinline__ float vonmises_draw(const DistroKey& key, float loc, float conc, float rm1) {
    float x = 0.0f;
    for (int j = 0; j < kMaxProposals; ++j) {
        const Philox4 p = key.block(j);
        const float h = 0.5f * u_half(p.v[0]);  // [0, 1/2): the cosine stays positive
        const float sh = sinpif(h), ch = cospif(h);
        const float omz = 2.0f * sh * sh, opz = 2.0f * ch * ch;
        const float omf = rm1 * omz / (rm1 + opz);
        const float c = conc * (rm1 + omf);
        const float u2 = u_open(p.v[1]);
        if (c * (2.0f - c) - u2 > 0.0f || logf(c / u2) + 1.0f - c >= 0.0f) {
            x = copysignf(2.0f * atan2f(sqrtf(rm1 * omz), sqrtf((rm1 + 2.0f) * opz)), u_half(p.v[2]) - 0.5f);
            break;
        }
    }
    const float two_pi = 6.283185307179586f;
    const float t = x + 3.141592653589793f + loc;
    return t - two_pi * floorf(t / two_pi) - 3.141592653589793f;
}

template <int FAM, int D>
__device__ __forceinline__ float distro_value(const sonar_distro_params& p, const DistroKey& key) {
    if constexpr (FAM == SONAR_DISTRO_EXPONENTIAL) {
        return -logf(u_open(key.block(0).v[0])) / p.a;
    } else if constexpr (FAM == SONAR_DISTRO_CAUCHY) {
        const float t = u_open(key.block(0).v[0]) - 0.5f;
        return p.a + p.b * (sinpif(t) / cospif(t));
    } else if constexpr (FAM == SONAR_DISTRO_GEOMETRIC) {
        return ceilf(logf(u_open(key.block(0).v[0])) / log1pf(-p.a));
    } else if constexpr (FAM == SONAR_DISTRO_LOG_NORMAL) {
        return expf(p.a + p.b * normal_at(key, 0));
    } else if constexpr (FAM == SONAR_DISTRO_NORMAL) {
        return p.a + p.b * normal_at(key, 0);
    } else if constexpr (FAM == SONAR_DISTRO_BETA) {
        const float g1 = gamma_draw(key, 0, p.a), g0 = gamma_draw(key, 1, p.b);
        return g1 / (g1 + g0);
    } else if constexpr (FAM == SONAR_DISTRO_CONTINUOUS_BERNOULLI) {
        const float u = u_half(key.block(0).v[0]);
        if (p.a > 0.499f && p.a < 0.501f) return u;  // torch's unstable region: the uniform itself
        return (log1pf(-p.a + u * (2.0f * p.a - 1.0f)) - log1pf(-p.a)) / (logf(p.a) - log1pf(-p.a));
    } else if constexpr (FAM == SONAR_DISTRO_DIRICHLET) {
        float sum = 0.0f, sel = 0.0f;
#pragma unroll
        for (int i = 0; i < kMaxEvent; ++i) {
            if (i < p.k) {
                const float g = gamma_draw(key, i, p.v[i]);
                sum += g;
                if (i == p.row) sel = g;
            }
        }
        return sel / sum;
    } else if constexpr (FAM == SONAR_DISTRO_FISHER_SNEDECOR) {
        const float g1 = gamma_draw(key, 0, 0.5f * p.a), g2 = gamma_draw(key, 1, 0.5f * p.b);
        return (g1 / p.a) / (g2 / p.b);
    } else if constexpr (FAM == SONAR_DISTRO_GAMMA) {
        return gamma_draw(key, 0, p.a) / p.b;
    } else if constexpr (FAM == SONAR_DISTRO_GUMBEL) {
        return p.a - p.b * logf(-logf(u_open(key.block(0).v[0])));
    } else if constexpr (FAM == SONAR_DISTRO_INVERSE_GAMMA) {
        return p.b / gamma_draw(key, 0, p.a);
    } else if constexpr (FAM == SONAR_DISTRO_KUMARASWAMY) {
        return powf(-expm1f(logf(u_open(key.block(0).v[0])) / p.b), 1.0f / p.a);
    } else if constexpr (FAM == SONAR_DISTRO_LAPLACIAN) {
        const float v = 2.0f * u_open(key.block(0).v[0]) - 1.0f;
        return p.a - p.b * copysignf(1.0f, v) * log1pf(-fabsf(v));
    } else if constexpr (FAM == SONAR_DISTRO_LKJCHOLESKY) {
        // onion method (torch's LKJCholesky.sample): row i >= 1 is sqrt(y_i) times a unit direction over columns < i, y_i ~ Beta(i - 1/2,
        // eta + (d - 2) / 2 - (i - 1) / 2), the diagonal sqrt(1 - y_i); row 0 is (1, 0, ...)
        const int i = p.row, j = p.col;
        if (j > i) return 0.0f;
        if (i == 0) return 1.0f;
        const float g1 = gamma_draw(key, 0, (float)i - 0.5f);
        const float g0 = gamma_draw(key, 1, p.a + 0.5f * (float)(D - 2) - 0.5f * (float)(i - 1));
        const float y = g1 / (g1 + g0);
        if (j == i) return sqrtf(fmaxf(1.0f - y, FLT_MIN));
        float ss = 0.0f, zj = 0.0f;
#pragma unroll
        for (int c = 0; c < D - 1; ++c) {
            if (c < i) {
                const float z = normal_at(key, (uint32_t)(i * kRowBlocks + c));
                ss += z * z;
                if (c == j) zj = z;
            }
        }
        return sqrtf(y) * zj / sqrtf(ss);
    } else if constexpr (FAM == SONAR_DISTRO_LRMVARIATE_NORMAL) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < kMaxEvent; ++r)
            if (r < p.k) s += p.v[r] * normal_at(key, (uint32_t)r);
        return p.a + s + p.b * normal_at(key, (uint32_t)(kMaxEvent + p.row));
    } else if constexpr (FAM == SONAR_DISTRO_MVARIATE_NORMAL) {
        return p.a + p.b * normal_at(key, (uint32_t)p.row);
    } else if constexpr (FAM == SONAR_DISTRO_PARETO) {
        return p.a * expf(-logf(u_open(key.block(0).v[0])) / p.b);
    } else if constexpr (FAM == SONAR_DISTRO_POISSON) {
        return poisson_draw(key, p.a);
    } else if constexpr (FAM == SONAR_DISTRO_RELAXED_BERNOULLI) {
        const float u = u_open(key.block(0).v[0]);
        const float y = (p.a + (logf(u) - log1pf(-u))) / p.b;
        return fminf(fmaxf(1.0f / (1.0f + expf(-y)), FLT_MIN), 1.0f - FLT_EPSILON);  // torch's clipped sigmoid
    } else if constexpr (FAM == SONAR_DISTRO_RELAXED_ONEHOTCATEGORICAL) {
        // softmax of (logit_i + gumbel_i) / temperature, gumbel i from word i % 4 of block i / 4; online max and sum
        float m = -INFINITY, s = 0.0f, sel = 0.0f;
#pragma unroll
        for (int q = 0; q < kMaxEvent / 4; ++q) {
            if (4 * q < p.k) {
                const Philox4 w = key.block((uint32_t)q);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int i = 4 * q + t;
                    if (i < p.k) {
                        const float y = (p.v[i] - logf(-logf(u_open(w.v[t])))) / p.a;
                        const float m2 = fmaxf(m, y);
                        s = s * expf(m - m2) + expf(y - m2);
                        m = m2;
                        if (i == p.row) sel = y;
                    }
                }
            }
        }
        return expf(sel - m) / s;
    } else if constexpr (FAM == SONAR_DISTRO_STUDENTT) {
        const float z = normal_at(key, 0);
        const float chi2 = 2.0f * gamma_draw(key, 0, 0.5f * p.c);
        return p.a + p.b * (z * sqrtf(p.c / chi2));
    } else if constexpr (FAM == SONAR_DISTRO_UNIFORM) {
        return p.a + u_half(key.block(0).v[0]) * (p.b - p.a);
    } else if constexpr (FAM == SONAR_DISTRO_VONMISES) {
        return vonmises_draw(key, p.a, p.b, p.c);
    } else if constexpr (FAM == SONAR_DISTRO_WEIBULL) {
        return p.a * powf(-logf(u_open(key.block(0).v[0])), 1.0f / p.b);
    } else if constexpr (FAM == SONAR_DISTRO_WISHART) {
        // Bartlett: A_ii = sqrt(chi2(df - i)) (gamma slot i, clamped to FLT_EPSILON as torch does), A_ik = normal (i, k) below the
        // diagonal; entry (i, j) of cov_multiplier * A A^T
        const int lo = min(p.row, p.col), hi = max(p.row, p.col);
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < D - 1; ++c)
            if (c < lo) s += normal_at(key, (uint32_t)(lo * kRowBlocks + c)) * normal_at(key, (uint32_t)(hi * kRowBlocks + c));
        const float a_lo = fmaxf(sqrtf(2.0f * gamma_draw(key, (uint32_t)lo, 0.5f * (p.a - (float)lo))), FLT_EPSILON);
        s += a_lo * (hi == lo ? a_lo : normal_at(key, (uint32_t)(hi * kRowBlocks + lo)));
        return p.b * s;
    }
    return 0.0f;
}

// Whole groups of 4 values (16-byte stores, no range checks) over the first n - n % 4 elements; the last n % 4 by block 0.
template <int FAM, int D>
__global__ void __launch_bounds__(kBlock) distro_fill_kernel(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                                             sonar_distro_params p) {
    kernarg_touch_for(out, n, seed, stream_id, elem_offset, p);
    const int64_t groups = n >> 2;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = distro_value<FAM, D>(p, DistroKey(seed, stream_id, (uint64_t)(elem_offset + 4 * g + k)));
        *reinterpret_cast<float4*>(out + 4 * g) = make_float4(v[0], v[1], v[2], v[3]);
    }
    const int64_t tail = n & 3;
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < tail) {
        const int64_t e = 4 * groups + threadIdx.x;
        out[e] = distro_value<FAM, D>(p, DistroKey(seed, stream_id, (uint64_t)(elem_offset + e)));
    }
}

using FillFn = void (*)(float*, int64_t, uint64_t, uint64_t, int64_t, sonar_distro_params);

template <int FAM>
FillFn fill_fn(int d) {
    if constexpr (FAM == SONAR_DISTRO_LKJCHOLESKY || FAM == SONAR_DISTRO_WISHART) {
        switch (d) {
            case 2: return distro_fill_kernel<FAM, 2>;
            case 3: return distro_fill_kernel<FAM, 3>;
            case 4: return distro_fill_kernel<FAM, 4>;
            case 5: return distro_fill_kernel<FAM, 5>;
            case 6: return distro_fill_kernel<FAM, 6>;
            case 7: return distro_fill_kernel<FAM, 7>;
            case 8: return distro_fill_kernel<FAM, 8>;
            default: return nullptr;
        }
    } else {
        return distro_fill_kernel<FAM, 0>;
    }
}

template <int... F>
FillFn pick(int family, int d, std::integer_sequence<int, F...>) {
    FillFn fn = nullptr;
    ((family == F ? (fn = fill_fn<F>(d), 0) : 0), ...);
    return fn;
}

bool params_ok(const sonar_distro_params& p) {
    if (!(isfinite(p.a) && isfinite(p.b) && isfinite(p.c))) return false;
    for (int i = 0; i < kMaxEvent; ++i)
        if (!isfinite(p.v[i])) return false;
    switch (p.family) {
        case SONAR_DISTRO_DIRICHLET:
        case SONAR_DISTRO_RELAXED_ONEHOTCATEGORICAL:
            return p.k >= 1 && p.k <= kMaxEvent && p.row >= 0 && p.row < p.k;
        case SONAR_DISTRO_LRMVARIATE_NORMAL:
            return p.k >= 1 && p.k <= kMaxEvent && p.row >= 0 && p.row < kMaxEvent;
        case SONAR_DISTRO_MVARIATE_NORMAL:
            return p.row >= 0 && p.row < kMaxEvent;
        case SONAR_DISTRO_LKJCHOLESKY:
        case SONAR_DISTRO_WISHART:
            return p.k >= 2 && p.k <= 8 && p.row >= 0 && p.row < p.k && p.col >= 0 && p.col < p.k;
        default:
            return true;
    }
}

}  // namespace

}  // namespace sonar

extern "C" int sonar_distro_fill_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset, const sonar_distro_params* p,
                                     void* stream) {
    using namespace sonar;
    SONAR_REQUIRE(out && p && n >= 0 && elem_offset >= 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 &&
                      (uint64_t)(elem_offset + n) < ((uint64_t)1 << 48) && stream_id < ((uint64_t)1 << 48),
                  SONAR_ERR_ARG, "sonar_distro_fill_f32: bad argument");
    SONAR_REQUIRE(p->family >= 0 && p->family <= SONAR_DISTRO_WISHART && params_ok(*p), SONAR_ERR_ARG,
                  "sonar_distro_fill_f32: bad parameters for family %d", p->family);
    const FillFn fn = pick(p->family, p->k, std::make_integer_sequence<int, SONAR_DISTRO_WISHART + 1>{});
    SONAR_REQUIRE(fn != nullptr, SONAR_ERR_UNSUPPORTED, "sonar_distro_fill_f32: no kernel for family %d, d = %d", p->family, p->k);
    if (n == 0) return SONAR_OK;
    hipLaunchKernelGGL(fn, dim3(grid_for(n >> 2 > 0 ? n >> 2 : 1, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, out, n, seed, stream_id,
                       elem_offset, *p);
    return check_launch("sonar_distro_fill_f32");
}
