// Per-row and per-mid-axis kernels: one workgroup per row (row_visit, SONAR_ROW_LAUNCH) or one thread per element with its row's
// values broadcast -- row statistics, min/max and the rescales built on them, amax / std / division over a middle axis, the
// ModulatedNoise gain and ratio mix, the |x| quantile per row with its clamp, and the periodic table multiply.
// The folds shared with group_stats.hip's strided kernels live in headers: extremes and the NaN flag in range_reduce.h (which NaN rule a
// kernel follows is said at its reduction), the mean / std tail (mean_std_of) and the rescale sequences in common.h.
#include <math.h>

#include "common.h"
#include "range_reduce.h"

namespace sonar {

// Kernels with ONE workgroup per row (a row is usually a whole latent or plane, and there are few of them) run at the latency of that
// workgroup's loads, not at any throughput: kRowThreads threads, and row_visit keeps four independent 16-byte loads per thread in
// flight (amax over four rows of 65536 values: 63 -> 6 us).  f sees every element once, in no particular order.
// Short rows (there are then usually many) keep 256-thread workgroups.
constexpr int kRowThreads = 1024;
constexpr int64_t kLongRow = 8192;
template <int THREADS, typename F>
__device__ __forceinline__ void row_visit(const float* __restrict__ row, int64_t n, F&& f) {
    if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0 && (n & 3) == 0) {
        const float4* row4 = reinterpret_cast<const float4*>(row);
        const int64_t n4 = n >> 2;
        int64_t i = threadIdx.x;
        for (; i + 3 * THREADS < n4; i += 4 * THREADS) {
            const float4 a = row4[i], b = row4[i + THREADS], c = row4[i + 2 * THREADS], d = row4[i + 3 * THREADS];
            f(a.x); f(a.y); f(a.z); f(a.w);
            f(b.x); f(b.y); f(b.z); f(b.w);
            f(c.x); f(c.y); f(c.z); f(c.w);
            f(d.x); f(d.y); f(d.z); f(d.w);
        }
        for (; i < n4; i += THREADS) {
            const float4 a = row4[i];
            f(a.x); f(a.y); f(a.z); f(a.w);
        }
    } else {
        for (int64_t i = threadIdx.x; i < n; i += THREADS) f(row[i]);
    }
}

// one workgroup per row: 1024 threads for long rows, 256 for short ones
#define SONAR_ROW_LAUNCH(kernel, row_len, nrows, lds, st, ...) \
    do { \
        if ((row_len) >= kLongRow) hipLaunchKernelGGL(kernel<kRowThreads>, dim3(grid_for(nrows, 1)), dim3(kRowThreads), lds, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel<kBlock>, dim3(grid_for(nrows, 1)), dim3(kBlock), lds, st, __VA_ARGS__); \
    } while (0)

// normalize_dims variant (py/utils.py:96-99): one block per row of `inner` contiguous elements
template <int THREADS>
__global__ void __launch_bounds__(THREADS) scale_rows_kernel(float* x, int64_t rows, int64_t inner, float factor) {
    kernarg_touch_for(x, rows, inner, factor);
    __shared__ double red[2 * THREADS / 64];
    __shared__ float sh_val;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        float* row = x + r * inner;
        double s = 0.0, q = 0.0;
        row_visit<THREADS>(row, inner, [&](float f) {
            const double v = f;
            s += v; q += v * v;
        });
        block_sum2<THREADS>(s, q, red);
        if (threadIdx.x == 0) sh_val = mean_std_of(s, q, (double)inner).stdv;
        __syncthreads();
        const float sd = sh_val;
        double s2 = 0.0, q2 = 0.0;
        row_visit<THREADS>(row, inner, [&](float f) { s2 += (double)(f / sd); });
        __syncthreads();
        block_sum2<THREADS>(s2, q2, red);
        if (threadIdx.x == 0) sh_val = (float)(s2 / (double)inner);
        __syncthreads();
        const float mean = sh_val;
        if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0 && (inner & 3) == 0) {
            float4* row4 = reinterpret_cast<float4*>(row);
            for (int64_t i = threadIdx.x; i < (inner >> 2); i += THREADS) {
                float4 v = row4[i];
                v.x = (v.x / sd - mean) * factor; v.y = (v.y / sd - mean) * factor;
                v.z = (v.z / sd - mean) * factor; v.w = (v.w / sd - mean) * factor;
                row4[i] = v;
            }
        } else {
            for (int64_t i = threadIdx.x; i < inner; i += THREADS) row[i] = (row[i] / sd - mean) * factor;
        }
        __syncthreads();
    }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) minmax_rows_kernel(const float* __restrict__ x, int64_t rows, int64_t inner,
                                                              float* out_min, float* out_max) {
    kernarg_touch_for(x, rows, inner, out_min, out_max);
    __shared__ float red[2 * THREADS / 64];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* row = x + r * inner;
        float lo = INFINITY, hi = -INFINITY;
        row_visit<THREADS>(row, inner, [&](float v) {
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        });
        block_minmax<THREADS>(lo, hi, red);  // a NaN never wins; its closing barrier frees `red` for the next row
        if (threadIdx.x == 0) {
            out_min[r] = lo;
            out_max[r] = hi;
        }
    }
}

template <int THREADS>
__global__ void __launch_bounds__(THREADS) rowstats_kernel(const float* __restrict__ x, int64_t rows, int64_t inner,
                                                           float* mean, float* stdv) {
    kernarg_touch_for(x, rows, inner, mean, stdv);
    __shared__ double red[2 * THREADS / 64];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* row = x + r * inner;
        double s = 0.0, q = 0.0;
        row_visit<THREADS>(row, inner, [&](float f) {
            const double v = f;
            s += v; q += v * v;
        });
        block_sum2<THREADS>(s, q, red);
        if (threadIdx.x == 0) {
            const MeanStd ms = mean_std_of(s, q, (double)inner);
            mean[r] = ms.mean;
            stdv[r] = ms.stdv;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) row_affine_kernel(int op, const float* __restrict__ x, int64_t rows,
                                                             int64_t inner, const float* __restrict__ a,
                                                             const float* __restrict__ b, float* out) {
    kernarg_touch_for(op, x, rows, inner, a, b, out);
    const int64_t total = rows * inner;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / inner;
        out[i] = row_affine_value(op, x[i], a[r], b[r]);
    }
}

// normalize_to_scale's tail (py/utils.py:462-469) per row: minmax_rescale_value (common.h)
__global__ void __launch_bounds__(kBlock) minmax_rescale_kernel(const float* __restrict__ x, int64_t rows, int64_t inner,
                                                                 const float* __restrict__ lo, const float* __restrict__ hi, float eps,
                                                                 float tmin, float tmax, float span, float* out) {
    kernarg_touch_for(x, rows, inner, lo, hi, eps, tmin, tmax, span, out);
    const int64_t total = rows * inner;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / inner;
        out[i] = minmax_rescale_value(x[i], lo[r], hi[r], eps, tmin, tmax, span);
    }
}

// normalize_to_scale_adv (py/utils.py:473-510): the negative and the positive values of a row are rescaled separately, each between its
// own extremes.  Pass 1: per row (min, max) over the negatives and over the positives (+-inf where a sign has no value).
__global__ void __launch_bounds__(kBlock) signed_minmax_rows_kernel(const float* __restrict__ x, int64_t rows, int64_t inner, float4* __restrict__ out) {
    kernarg_touch_for(x, rows, inner, out);
    __shared__ float red[4 * kBlock / 64];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};  // [0]: the negatives, [1]: the positives
        const float* row = x + r * inner;
        for (int64_t i = threadIdx.x; i < inner; i += kBlock) {
            const float v = row[i];
            if (v < 0.0f) {
                lo[0] = fminf(lo[0], v);
                hi[0] = fmaxf(hi[0], v);
            } else if (v > 0.0f) {
                lo[1] = fminf(lo[1], v);
                hi[1] = fmaxf(hi[1], v);
            }
        }
        block_minmax<kBlock, 2>(lo, hi, red);  // a NaN never wins; its closing barrier frees `red` for the next row
        if (threadIdx.x == 0) out[r] = make_float4(lo[0], hi[0], lo[1], hi[1]);
    }
}

// Pass 2: x < 0 -> normalize_to_scale over the negatives to [min_neg, max_neg] (max_neg >= 0: the row's own largest negative), x > 0 ->
// over the positives to [min_pos, max_pos] (min_pos < 0: the row's own smallest positive), 0 stays 0; a skipped sign is copied.  Each
// step rounded on its own, as the reference's in-place tensor ops are (the same sequence as minmax_rescale_kernel).
__global__ void __launch_bounds__(kBlock) signed_rescale_kernel(const float* __restrict__ x, int64_t rows, int64_t inner,
                                                                 const float4* __restrict__ stats, double min_neg, double max_neg, double min_pos,
                                                                 double max_pos, int skip_neg, int skip_pos, float eps, float* __restrict__ out) {
    kernarg_touch_for(x, rows, inner, stats, min_neg, max_neg, min_pos, max_pos, skip_neg, skip_pos, eps, out);
    const int64_t total = rows * inner;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const float4 st = stats[i / inner];
        const float v = x[i];
        float res = 0.0f;
        if (v < 0.0f || v > 0.0f) {
            const bool neg = v < 0.0f;
            if (neg ? skip_neg : skip_pos) {
                res = v;
            } else {
                const float lo = neg ? st.x : st.z, hi = neg ? st.y : st.w;
                // the targets are Python floats in the reference (the data-derived ones `.item()` of an fp32 value): their difference is
                // formed in double and meets the fp32 tensor as one rounded scalar; add_ / clamp_ round each bound on its own
                const double tmin_d = neg ? min_neg : (min_pos < 0.0 ? (double)st.z : min_pos);
                const double tmax_d = neg ? (max_neg >= 0.0 ? (double)st.y : max_neg) : max_pos;
                const float span = (float)(tmax_d - tmin_d), tmin = (float)tmin_d, tmax = (float)tmax_d;
                res = minmax_rescale_value(v, lo, hi, eps, tmin, tmax, span);
            }
        } else if (v != v) {
            res = 0.0f;  // NaN is neither < 0 nor > 0: the reference's masks leave the zero of zeros_like
        }
        out[i] = res;
    }
}

__global__ void __launch_bounds__(kBlock) amax_mid_kernel(const float* __restrict__ x, int64_t outer, int64_t mid,
                                                           int64_t inner, int use_abs, float* peak) {
    kernarg_touch_for(x, outer, mid, inner, use_abs, peak);
    const int64_t total = outer * inner;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t o = t / inner, i = t - o * inner;
        const float* p = x + o * mid * inner + i;
        float hi = -INFINITY;
        bool nan = false;
        for (int64_t m = 0; m < mid; ++m) {
            float v = p[m * inner];
            if (use_abs) v = fabsf(v);
            nan |= v != v;
            hi = fmaxf(hi, v);
        }
        peak[t] = nan_poisons(nan, hi);  // torch.amax propagates NaN
    }
}

// inner == 1: one workgroup per row of `mid` contiguous elements
template <int THREADS>
__global__ void __launch_bounds__(THREADS) amax_row_kernel(const float* __restrict__ x, int64_t rows, int64_t len, int use_abs,
                                                                float* peak) {
    kernarg_touch_for(x, rows, len, use_abs, peak);
    __shared__ float red[2 * THREADS / 64];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        float hi = -INFINITY;
        int nan = 0;
        row_visit<THREADS>(x + r * len, len, [&](float v) {
            if (use_abs) v = fabsf(v);
            nan |= v != v;
            hi = fmaxf(hi, v);
        });
        const float top = block_max_poisoned<THREADS>(hi, nan, red);  // a NaN poisons; its closing barrier frees `red` for the next row
        if (threadIdx.x == 0) peak[r] = top;
    }
}

__global__ void __launch_bounds__(kBlock) div_mid_kernel(float* x, int64_t outer, int64_t mid, int64_t inner,
                                                          const float* __restrict__ d) {
    kernarg_touch_for(x, outer, mid, inner, d);
    const int64_t total = outer * mid * inner, plane = mid * inner;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t o = t / plane;
        const int64_t i = (t - o * plane) % inner;
        x[t] = x[t] / d[o * inner + i];
    }
}

// ---- ModulatedNoise (py/noise.py:784-866) ----------------------------------------------------------------------------------
// unbiased std over the middle axis of x[outer][mid][inner] (torch.std(dim=-3, keepdim=True)); mid == 1 gives NaN like torch
__global__ void __launch_bounds__(kBlock) std_mid_kernel(const float* __restrict__ x, int64_t outer, int64_t mid, int64_t inner,
                                                          float* stdv) {
    kernarg_touch_for(x, outer, mid, inner, stdv);
    const int64_t total = outer * inner;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t o = t / inner, i = t - o * inner;
        const float* p = x + o * mid * inner + i;
        double s = 0.0;
        for (int64_t m = 0; m < mid; ++m) s += (double)p[m * inner];
        const double mean = s / (double)mid;
        double q = 0.0;
        for (int64_t m = 0; m < mid; ++m) {
            const double d = (double)p[m * inner] - mean;
            q += d * d;
        }
        stdv[t] = (float)sqrt(q / (double)(mid - 1));
    }
}

// v = x * k * (1 / (std * |strength| + 1) + 1), std broadcast through (so, sm, si) strides over x's [outer][mid][inner] view
// (py/noise.py:799-803: noise * scaling + noise).  Optional store; optional partials: slot pair (sum x^2, sum v^2) per block.
__global__ void __launch_bounds__(kBlock) bcast_gain_kernel(const float* __restrict__ x, const float* __restrict__ stdv, int64_t outer,
                                                             int64_t mid, int64_t inner, int64_t so, int64_t sm, int64_t si,
                                                             float abs_strength, float k, float* out, double* partials) {
    kernarg_touch_for(x, stdv, outer, mid, inner, so, sm, si, abs_strength, k, out, partials);
    __shared__ double red[2 * kBlock / 64];
    const int64_t total = outer * mid * inner, plane = mid * inner;
    double sx = 0.0, sv = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t o = t / plane, r = t - o * plane, m = r / inner, i = r - m * inner;
        const float sd = stdv[o * so + m * sm + i * si];
        const float gain = 1.0f / (sd * abs_strength + 1.0f);
        const float xv = x[t];
        const float plain = xv * k;
        const float v = plain * gain + plain;
        if (out) out[t] = v;
        sx += (double)xv * (double)xv;
        sv += (double)v * (double)v;
    }
    if (partials) write_partial<kBlock>(sx, sv, partials, red);
}

// out = a * (a_mul * rho) + x * x_mul with rho = sqrt(num_mul * sum(num[2i]) / sum(den[2i+1])) -- the "scale to normal noise
// strength" ratio of two L2 norms (py/noise.py:805-810), taken from partial slots so the host never reads it back
__global__ void __launch_bounds__(kBlock) ratio_mix_kernel(const float* __restrict__ a, float a_mul, const float* __restrict__ x,
                                                            float x_mul, const double* __restrict__ num, double num_mul,
                                                            const double* __restrict__ den, float* out, int64_t n) {
    kernarg_touch_for(a, a_mul, x, x_mul, num, num_mul, den, out, n);
    __shared__ double red[2 * kBlock / 64];
    __shared__ float srho;
    double sn = 0.0, sd = 0.0;
    for (int j = threadIdx.x; j < kNPart; j += kBlock) {
        sn += num[2 * j];
        sd += den[2 * j + 1];
    }
    block_sum2<kBlock>(sn, sd, red);
    if (threadIdx.x == 0) srho = (float)sqrt(num_mul * sn / sd);
    __syncthreads();
    const float am = a_mul * srho;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock)
        out[t] = a[t] * am + x[t] * x_mul;
}

// q-quantile (torch.quantile, linear interpolation) of |x| over each row of `inner` contiguous values: radix select on the bit
// patterns (non-negative floats order like unsigned integers), four 8-bit histogram passes in LDS, then one pass for the next
// order statistic.  One workgroup per row.  rank = lo + frac is computed by the host in fp32 like torch does.
// The first pass sees the exponent byte -- two or three bins take every value -- so each bin is kept in kQuantReplicas copies (lane
// mod 32 picks one, copies of a bin in distinct banks): same-address LDS atomics serialise, 226 -> 20 us for four rows of 65536.
constexpr int kQuantReplicas = 32;
template <int THREADS>
__global__ void __launch_bounds__(THREADS) abs_quantile_rows_kernel(const float* __restrict__ x, int64_t rows, int64_t inner, int64_t lo,
                                                                        float frac, float* out) {
    kernarg_touch_for(x, rows, inner, lo, frac, out);
    __shared__ unsigned hist[256 * kQuantReplicas];
    __shared__ unsigned total[256];
    __shared__ unsigned sh_prefix, sh_k, sh_cnt, sh_min;
    const unsigned rep = threadIdx.x & (kQuantReplicas - 1);
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* row = x + r * inner;
        const bool vec = (reinterpret_cast<uintptr_t>(row) & 15u) == 0 && (inner & 3) == 0;
        const float4* row4 = reinterpret_cast<const float4*>(row);
        unsigned prefix = 0, mask = 0, k = (unsigned)lo;
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int b = threadIdx.x; b < 256 * kQuantReplicas; b += THREADS) hist[b] = 0;
            __syncthreads();
            auto tally = [&](float v) {
                const unsigned bits = __float_as_uint(v) & 0x7FFFFFFFu;
                if ((bits & mask) == prefix) atomicAdd(&hist[((bits >> shift) & 255u) * kQuantReplicas + rep], 1u);
            };
            if (vec) {
                for (int64_t i = threadIdx.x; i < (inner >> 2); i += THREADS) {
                    const float4 v = row4[i];
                    tally(v.x); tally(v.y); tally(v.z); tally(v.w);
                }
            } else {
                for (int64_t i = threadIdx.x; i < inner; i += THREADS) tally(row[i]);
            }
            __syncthreads();
            if (threadIdx.x < 256) {
                unsigned sum = 0;
                for (int j = 0; j < kQuantReplicas; ++j) sum += hist[threadIdx.x * kQuantReplicas + ((j + threadIdx.x) & (kQuantReplicas - 1))];
                total[threadIdx.x] = sum;
            }
            __syncthreads();
            if (threadIdx.x < 64) {
                // the first bin b with (bins 0..b) > k, 255 if there is none: lane l owns bins 4l..4l+3
                const unsigned a0 = total[4 * threadIdx.x], a1 = total[4 * threadIdx.x + 1], a2 = total[4 * threadIdx.x + 2], a3 = total[4 * threadIdx.x + 3];
                const unsigned own = a0 + a1 + a2 + a3;
                unsigned incl = own;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned up = __shfl_up(incl, off, 64);
                    if ((int)threadIdx.x >= off) incl += up;
                }
                const unsigned excl = incl - own;
                if ((excl <= k && k < incl) || (threadIdx.x == 63 && k >= incl)) {
                    unsigned cum = excl, b = 4 * threadIdx.x;
                    if (cum + a0 <= k) {
                        cum += a0; ++b;
                        if (cum + a1 <= k) {
                            cum += a1; ++b;
                            if (cum + a2 <= k) { cum += a2; ++b; }
                        }
                    }
                    sh_prefix = prefix | (b << shift);
                    sh_k = k - cum;
                }
            }
            __syncthreads();
            prefix = sh_prefix;
            k = sh_k;
            mask |= 255u << shift;
            __syncthreads();
        }
        // prefix = bits of the lo-th smallest |x|; the next order statistic is the same value if it repeats, else the smallest larger one
        if (threadIdx.x == 0) {
            sh_cnt = 0;
            sh_min = 0x7FFFFFFFu;
        }
        __syncthreads();
        unsigned cnt = 0, mn = 0x7FFFFFFFu;
        auto look = [&](float v) {
            const unsigned bits = __float_as_uint(v) & 0x7FFFFFFFu;
            cnt += bits <= prefix;
            if (bits > prefix) mn = min(mn, bits);
        };
        if (vec) {
            for (int64_t i = threadIdx.x; i < (inner >> 2); i += THREADS) {
                const float4 v = row4[i];
                look(v.x); look(v.y); look(v.z); look(v.w);
            }
        } else {
            for (int64_t i = threadIdx.x; i < inner; i += THREADS) look(row[i]);
        }
        atomicAdd(&sh_cnt, cnt);
        atomicMin(&sh_min, mn);
        __syncthreads();
        if (threadIdx.x == 0) {
            const float vlo = __uint_as_float(prefix);
            const float vhi = (lo + 1 < (int64_t)sh_cnt || lo + 1 >= inner) ? vlo : __uint_as_float(sh_min);
            out[r] = blend<float>(SONAR_BLEND_LERP, vlo, vhi, frac);
        }
        __syncthreads();
    }
}

// x = copysign(|clamp(x, -lim, lim)|^p, x) per row, lim = limit[row] * mul (StudentT: clamp to the quantile, compress the tails)
__global__ void __launch_bounds__(kBlock) clamp_signpow_rows_kernel(float* x, int64_t rows, int64_t inner, const float* __restrict__ limit,
                                                                     float mul, float p) {
    kernarg_touch_for(x, rows, inner, limit, mul, p);
    const int64_t total = rows * inner;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const float lim = limit[i / inner] * mul;
        const float v = fminf(fmaxf(x[i], -lim), lim);
        const float a = fabsf(v);
        const float m = p == 0.5f ? sqrtf(a) : p == 1.0f ? a : p == 2.0f ? a * a : powf(a, p);
        x[i] = copysignf(m, v);
    }
}

// RippleFilteredNoise (py/noise.py:1134-1202): x *= s[(i / inner) % len] with a small periodic table s broadcast over the
// tensor; with `follow_sign` the result takes the sign of 1 - s (torch.copysign(result, 1 - s))
__global__ void __launch_bounds__(kBlock) mul_table_kernel(float* x, const float* __restrict__ s, int64_t n, int64_t inner, int64_t len,
                                                            int follow_sign) {
    kernarg_touch_for(x, s, n, inner, len, follow_sign);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float sv = s[(i / inner) % len];
        float v = x[i] * sv;
        if (follow_sign) v = copysignf(v, 1.0f - sv);
        x[i] = v;
    }
}

}  // namespace sonar

using namespace sonar;

// ================================================================================================
extern "C" int sonar_scale_noise_rows_f32(float* x, int64_t rows, int64_t inner, float factor, void* stream) {
    SONAR_REQUIRE(x && rows >= 0 && inner > 0, SONAR_ERR_ARG, "sonar_scale_noise_rows_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    SONAR_ROW_LAUNCH(scale_rows_kernel, inner, rows, 0, (hipStream_t)stream, x, rows, inner,
                       factor);
    return check_launch("sonar_scale_noise_rows_f32");
}

extern "C" int sonar_minmax_rows_f32(const float* x, int64_t rows, int64_t inner, float* out_min, float* out_max,
                                     void* stream) {
    SONAR_REQUIRE(x && out_min && out_max && rows >= 0 && inner > 0, SONAR_ERR_ARG, "sonar_minmax_rows_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    SONAR_ROW_LAUNCH(minmax_rows_kernel, inner, rows, 0, (hipStream_t)stream, x, rows, inner,
                       out_min, out_max);
    return check_launch("sonar_minmax_rows_f32");
}

extern "C" int sonar_rowstats_f32(const float* x, int64_t rows, int64_t inner, float* mean, float* stdv, void* stream) {
    SONAR_REQUIRE(x && mean && stdv && rows >= 0 && inner > 0, SONAR_ERR_ARG, "sonar_rowstats_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    SONAR_ROW_LAUNCH(rowstats_kernel, inner, rows, 0, (hipStream_t)stream, x, rows, inner, mean, stdv);
    return check_launch("sonar_rowstats_f32");
}

extern "C" int sonar_row_affine_f32(int op, const float* x, int64_t rows, int64_t inner, const float* a, const float* b,
                                    float* out, void* stream) {
    SONAR_REQUIRE(x && a && b && out && rows >= 0 && inner > 0 && (op == 0 || op == 1), SONAR_ERR_ARG,
                  "sonar_row_affine_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    hipLaunchKernelGGL(row_affine_kernel, dim3(grid_for(rows * inner, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, op, x,
                       rows, inner, a, b, out);
    return check_launch("sonar_row_affine_f32");
}

extern "C" int sonar_minmax_rescale_f32(const float* x, int64_t rows, int64_t inner, const float* lo, const float* hi, float eps,
                                        double target_min, double target_max, float* out, void* stream) {
    SONAR_REQUIRE(x && lo && hi && out && rows >= 0 && inner > 0, SONAR_ERR_ARG, "sonar_minmax_rescale_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    hipLaunchKernelGGL(minmax_rescale_kernel, dim3(grid_for(rows * inner, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, rows,
                       inner, lo, hi, eps, (float)target_min, (float)target_max, (float)(target_max - target_min), out);
    return check_launch("sonar_minmax_rescale_f32");
}

extern "C" int sonar_signed_rescale_f32(const float* x, int64_t rows, int64_t inner, double min_neg, double max_neg, double min_pos, double max_pos,
                                        float eps, float* stats_ws, float* out, void* stream) {
    SONAR_REQUIRE(x && out && stats_ws && rows >= 0 && inner > 0 && (reinterpret_cast<uintptr_t>(stats_ws) & 15u) == 0, SONAR_ERR_ARG,
                  "sonar_signed_rescale_f32: bad argument (a 16-byte aligned workspace of 4 floats per row is required)");
    if (rows == 0) return SONAR_OK;
    // py/utils.py:482-483
    const int skip_pos = max_pos <= 0.0 || min_pos >= max_pos, skip_neg = min_neg >= 0.0 || min_neg >= max_neg;
    float4* st = reinterpret_cast<float4*>(stats_ws);
    hipLaunchKernelGGL(signed_minmax_rows_kernel, dim3((int)std::min<int64_t>(rows, 4096)), dim3(kBlock), 0, (hipStream_t)stream, x, rows, inner, st);
    hipLaunchKernelGGL(signed_rescale_kernel, dim3(grid_for(rows * inner, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, rows, inner, st,
                       min_neg, max_neg, min_pos, max_pos, skip_neg, skip_pos, eps, out);
    return check_launch("sonar_signed_rescale_f32");
}

extern "C" int sonar_amax_mid_f32(const float* x, int64_t outer, int64_t mid, int64_t inner, int use_abs, float* peak,
                                  void* stream) {
    SONAR_REQUIRE(x && peak && outer >= 0 && mid > 0 && inner > 0, SONAR_ERR_ARG, "sonar_amax_mid_f32: bad argument");
    if (outer == 0) return SONAR_OK;
    if (inner == 1)
        SONAR_ROW_LAUNCH(amax_row_kernel, mid, outer, 0, (hipStream_t)stream, x, outer, mid, use_abs, peak);
    else
        hipLaunchKernelGGL(amax_mid_kernel, dim3(grid_for(outer * inner, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, x, outer,
                           mid, inner, use_abs, peak);
    return check_launch("sonar_amax_mid_f32");
}

extern "C" int sonar_div_mid_f32(float* x, int64_t outer, int64_t mid, int64_t inner, const float* d, void* stream) {
    SONAR_REQUIRE(x && d && outer >= 0 && mid > 0 && inner > 0, SONAR_ERR_ARG, "sonar_div_mid_f32: bad argument");
    if (outer == 0) return SONAR_OK;
    hipLaunchKernelGGL(div_mid_kernel, dim3(grid_for(outer * mid * inner, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x,
                       outer, mid, inner, d);
    return check_launch("sonar_div_mid_f32");
}

extern "C" int sonar_abs_quantile_rows_f32(const float* x, int64_t rows, int64_t inner, int64_t rank_lo, float rank_frac, float* out,
                                           void* stream) {
    SONAR_REQUIRE(x && out && rows >= 0 && inner > 0 && rank_lo >= 0 && rank_lo < inner && rank_frac >= 0.0f && rank_frac <= 1.0f,
                  SONAR_ERR_ARG, "sonar_abs_quantile_rows_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    SONAR_ROW_LAUNCH(abs_quantile_rows_kernel, inner, rows, 0, (hipStream_t)stream, x, rows, inner, rank_lo,
                       rank_frac, out);
    return check_launch("sonar_abs_quantile_rows_f32");
}

extern "C" int sonar_clamp_signpow_rows_f32(float* x, int64_t rows, int64_t inner, const float* limit, float mul, float p, void* stream) {
    SONAR_REQUIRE(x && limit && rows >= 0 && inner > 0, SONAR_ERR_ARG, "sonar_clamp_signpow_rows_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    hipLaunchKernelGGL(clamp_signpow_rows_kernel, dim3(grid_for(rows * inner, kBlock * 4)), dim3(kBlock), 0, (hipStream_t)stream, x, rows,
                       inner, limit, mul, p);
    return check_launch("sonar_clamp_signpow_rows_f32");
}

extern "C" int sonar_mul_table_f32(float* x, const float* table, int64_t n, int64_t inner, int64_t len, int follow_sign, void* stream) {
    SONAR_REQUIRE(x && table && n >= 0 && inner > 0 && len > 0, SONAR_ERR_ARG, "sonar_mul_table_f32: bad argument");
    if (n == 0) return SONAR_OK;
    hipLaunchKernelGGL(mul_table_kernel, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, (hipStream_t)stream, x, table, n, inner, len,
                       follow_sign);
    return check_launch("sonar_mul_table_f32");
}

extern "C" int sonar_std_mid_f32(const float* x, int64_t outer, int64_t mid, int64_t inner, float* stdv, void* stream) {
    SONAR_REQUIRE(x && stdv && outer >= 0 && mid > 0 && inner > 0, SONAR_ERR_ARG, "sonar_std_mid_f32: bad argument");
    if (outer == 0) return SONAR_OK;
    hipLaunchKernelGGL(std_mid_kernel, dim3(grid_for(outer * inner, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, x, outer, mid, inner,
                       stdv);
    return check_launch("sonar_std_mid_f32");
}

extern "C" int sonar_bcast_gain_f32(const float* x, const float* stdv, int64_t outer, int64_t mid, int64_t inner, int bcast,
                                    float abs_strength, float k, float* out, double* partials, void* stream) {
    SONAR_REQUIRE(x && stdv && (out || partials) && outer >= 0 && mid > 0 && inner > 0 && bcast >= 0 && bcast <= 2, SONAR_ERR_ARG,
                  "sonar_bcast_gain_f32: bad argument");
    // bcast 0: std[outer] (dims -3,-2,-1)   1: std[outer][mid] (dims -2,-1)   2: std[outer][inner] (dim -3)
    const int64_t so = bcast == 0 ? 1 : bcast == 1 ? mid : inner, sm = bcast == 1 ? 1 : 0, si = bcast == 2 ? 1 : 0;
    const int64_t n = outer * mid * inner;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>(grid_for(n, kBlock * 4), 1), kNPart);
    hipLaunchKernelGGL(bcast_gain_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, x, stdv, outer, mid, inner, so, sm, si,
                       abs_strength, k, out, partials);
    return check_launch("sonar_bcast_gain_f32");
}

extern "C" int sonar_ratio_mix_f32(const float* a, float a_mul, const float* x, float x_mul, const double* num_partials,
                                   double num_mul, const double* den_partials, float* out, int64_t n, void* stream) {
    SONAR_REQUIRE(a && x && num_partials && den_partials && out && n >= 0, SONAR_ERR_ARG, "sonar_ratio_mix_f32: bad argument");
    if (n == 0) return SONAR_OK;
    hipLaunchKernelGGL(ratio_mix_kernel, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, (hipStream_t)stream, a, a_mul, x, x_mul,
                       num_partials, num_mul, den_partials, out, n);
    return check_launch("sonar_ratio_mix_f32");
}
