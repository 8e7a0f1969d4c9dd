// Quantile filtering (the reference's utils.quantile_normalize, py/utils.py:123-449): per-row |x| quantile by radix select, an
// optional second row statistic (max |x|, mean, signed lower median, mode of the rounded values), then one of the 43 outlier strategies,
// the "centered" back-mapping and the sign-preserving power -- and the replace* family's global candidate compaction.
//
// Rows are `inner` contiguous values (the caller moves a non-trailing dim last).  One workgroup per row:
//   * rows of up to 64 Ki values stay in registers (VPT values per thread) across every pass: read once, written once;
//   * longer rows are re-read from memory on every pass (same code, VPT = 0).
#include "common.h"
#include "range_reduce.h"

namespace sonar {

namespace {

// strategy codes (include/sonar_hip.h SONAR_Q_*)
constexpr int kQClamp = 0, kQTanh = 1, kQTanhOut = 2, kQSigmoid = 3, kQSigmoidKeep = 4, kQSigmoidOut = 5, kQAtan = 6, kQTenth = 7,
              kQHalf = 8, kQZero = 9, kQReverseZero = 10, kQScaleDown = 11, kQMean = 12, kQMedian = 13, kQMode1 = 14, kQMode2 = 15,
              kQWave = 16;
constexpr int kQWaveCos = 1 << 8, kQWaveWholePi = 1 << 9, kQWaveWrong = 1 << 10, kQWaveKeepSign = 1 << 11;

constexpr int kQReplicas = 32;                 // copies of each radix bin (lane mod 32), as in abs_quantile_rows_kernel
constexpr int kQBins = 256 * kQReplicas;        // LDS words of the radix histogram; the mode windows reuse them
constexpr int kQModeWindow = kQBins;            // rounded-value bins counted per pass of the mode search
constexpr int kQRowThreads = 1024;
constexpr int kQResidentMax = kQRowThreads * 64;  // longest row kept in registers

__device__ __forceinline__ float sgnf(float v) { return v > 0.0f ? 1.0f : v < 0.0f ? -1.0f : 0.0f; }

// proxy of the "centered" mode: sign(x) * (max|x| - |x|)
__device__ __forceinline__ float centered_proxy(float x, float maxabs) { return sgnf(x) * __fsub_rn(maxabs, fabsf(x)); }

// order-preserving key of a signed float (for the median)
__device__ __forceinline__ unsigned signed_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float signed_key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// torch.round(x, decimals=d) for d = 1, 2: nearbyint(x * 10^d) / 10^d
__device__ __forceinline__ int mode_key(float v, float tp) {
    const float r = rintf(__fmul_rn(v, tp));
    return (int)fminf(fmaxf(r, -1073741824.0f), 1073741824.0f);  // finite values only; |key| <= 2^30 (beyond +-2^30 / 10^d: the end bins)
}

// copysign(|v|^p, v) for p not in {0, 1}; torch.pow's special exponents
__device__ __forceinline__ float signpow(float v, float p) {
    const float a = fabsf(v);
    const float m = p == 0.5f ? sqrtf(a) : p == 2.0f ? a * a : p == -0.5f ? 1.0f / sqrtf(a) : p == -1.0f ? 1.0f / a : powf(a, p);
    return copysignf(m, v);
}

// the strategy on one value; nq is the row's threshold, s2 its second statistic (nq / max|x| for scale_down)
__device__ __forceinline__ float q_apply(int op, float x, float nq, float s2) {
    const float anq = fabsf(nq);
    const bool out = fabsf(x) > nq;
    switch (op & 0xFF) {
        case kQClamp: return fminf(fmaxf(x, -nq), nq);
        case kQTanh: return tanhf(x) * anq;
        case kQTanhOut: return out ? tanhf(x) * anq : x;
        case kQSigmoid: return __fsub_rn(__fmul_rn(1.0f / (1.0f + expf(-x)), anq * 2.0f), anq);
        case kQSigmoidKeep: return copysignf(__fmul_rn(1.0f / (1.0f + expf(-x)), anq), x);
        case kQSigmoidOut: return out ? copysignf(__fmul_rn(1.0f / (1.0f + expf(-x)), anq), x) : x;
        case kQAtan: return atanf(x) * (anq / 1.57079637f);
        case kQTenth: return out ? x * 0.1f : x;
        case kQHalf: return out ? x * 0.5f : x;
        case kQZero: return out ? 0.0f : x;
        case kQReverseZero: return fabsf(x) >= nq ? x : 0.0f;
        case kQScaleDown: return out ? x * s2 : x;
        case kQMean:
        case kQMedian:
        case kQMode1:
        case kQMode2: return out ? s2 : x;
        default: {  // kQWave: wave(x * mult) * nq
            const float pipf = (op & kQWaveWholePi) ? 3.14159274f : 1.57079637f;
            const float mult = 1.0f / ((op & kQWaveWrong) ? pipf / nq : nq / pipf);
            const float a = __fmul_rn(x, mult);
            const float w = __fmul_rn((op & kQWaveCos) ? cosf(a) : sinf(a), nq);
            return (op & kQWaveKeepSign) ? copysignf(w, x) : w;
        }
    }
}

// the tail shared by every route: centered back-mapping, then the power
__device__ __forceinline__ float q_finish(float o, bool centered, float maxabs, float pow_fac) {
    if (centered) o = sgnf(o) * __fsub_rn(maxabs, fabsf(o));
    if (pow_fac != 0.0f && pow_fac != 1.0f) o = signpow(o, pow_fac);
    return o;
}

// Strategies without transcendentals and powers without powf: cheap enough to apply inside the row kernel, next to the row it keeps in
// registers.  The others (tanh, sigmoid*, atan, sin*, cos*, a general power) would inline libm code into every unrolled register slot;
// they get the row's statistics and run in quantile_apply_kernel instead (one more read of the input).
__host__ __device__ __forceinline__ bool q_light(int op, float pow_fac) {
    const int base = op & 0xFF;
    const bool light_op = base == kQClamp || (base >= kQTenth && base <= kQMode2);
    return light_op && (pow_fac == 0.0f || pow_fac == 1.0f || pow_fac == 0.5f || pow_fac == 2.0f);
}
__device__ __forceinline__ float q_apply_light(int op, float x, float nq, float s2) {
    const bool out = fabsf(x) > nq;
    switch (op & 0xFF) {
        case kQClamp: return fminf(fmaxf(x, -nq), nq);
        case kQTenth: return out ? x * 0.1f : x;
        case kQHalf: return out ? x * 0.5f : x;
        case kQZero: return out ? 0.0f : x;
        case kQReverseZero: return fabsf(x) >= nq ? x : 0.0f;
        case kQScaleDown: return out ? x * s2 : x;
        default: return out ? s2 : x;  // mean, median, mode
    }
}
__device__ __forceinline__ float q_finish_light(float o, bool centered, float maxabs, float pow_fac) {
    if (centered) o = sgnf(o) * __fsub_rn(maxabs, fabsf(o));
    if (pow_fac == 0.5f) o = copysignf(sqrtf(fabsf(o)), o);
    else if (pow_fac == 2.0f) o = copysignf(o * o, o);
    return o;
}

// (block reductions: block_reduce of range_reduce.h -- the totals in every thread, waves joined in ascending order)

// ---- the row: in registers (VPT > 0) or re-read from memory (VPT == 0) --------------------------------------------------------------
template <int THREADS, int VPT>
struct QRow {
    const float* row;
    int n;       // row length (< 2^31)
    int nslots;  // slots j < nslots of this thread hold values of the row (the same test for every slot: no per-slot masks)
    bool vec;    // float4 layout: slot j of a thread is element ((j / 4) * THREADS + tid) * 4 + j % 4; else j * THREADS + tid
                 // (one layout for the loads and for map_store: both the row and its destination must allow 16-byte accesses)
    float v[VPT > 0 ? VPT : 1];

    __device__ __forceinline__ void load(const float* r, int len, const float* dst) {
        row = r;
        n = len;
        vec = ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0 && (len & 3) == 0;  // (dst may be null)
        const int tid = threadIdx.x;
        nslots = vec ? 4 * (((len >> 2) - tid + THREADS - 1) / THREADS) : (len - tid + THREADS - 1) / THREADS;
        if constexpr (VPT > 0) {
            if (vec) {
                const float4* r4 = reinterpret_cast<const float4*>(r);
#pragma unroll
                for (int j = 0; j < VPT; j += 4) {
                    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (j < nslots) q = r4[(j >> 2) * THREADS + tid];
                    v[j] = q.x; v[j + 1] = q.y; v[j + 2] = q.z; v[j + 3] = q.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < VPT; ++j) v[j] = j < nslots ? r[j * THREADS + tid] : 0.0f;
            }
        }
    }
    template <typename F>
    __device__ __forceinline__ void each(F&& f) const {
        if constexpr (VPT > 0) {
#pragma unroll
            for (int j = 0; j < VPT; ++j) {
                // an opaque copy: otherwise the compiler hoists each pass's key of every slot out of the callers' pass loops and keeps
                // VPT keys live next to the VPT values (the 64-slot kernel then spilled 450 bytes per lane)
                float xv = v[j];
                asm volatile("" : "+v"(xv));
                if (j < nslots) f(xv);
            }
        } else {
            if (vec) {
                const float4* r4 = reinterpret_cast<const float4*>(row);
                for (int i = threadIdx.x; i < (n >> 2); i += THREADS) {
                    const float4 q = r4[i];
                    f(q.x); f(q.y); f(q.z); f(q.w);
                }
            } else {
                for (int i = threadIdx.x; i < n; i += THREADS) f(row[i]);
            }
        }
    }
    // out[i] = g(x[i]) over the row
    template <typename G>
    __device__ __forceinline__ void map_store(float* out, G&& g) const {
        const int tid = threadIdx.x;
        if (vec) {
            float4* o4 = reinterpret_cast<float4*>(out);
            if constexpr (VPT > 0) {
#pragma unroll
                for (int j = 0; j < VPT; j += 4)
                    if (j < nslots) o4[(j >> 2) * THREADS + tid] = make_float4(g(v[j]), g(v[j + 1]), g(v[j + 2]), g(v[j + 3]));
            } else {
                const float4* r4 = reinterpret_cast<const float4*>(row);
                for (int i = tid; i < (n >> 2); i += THREADS) {
                    const float4 q = r4[i];
                    o4[i] = make_float4(g(q.x), g(q.y), g(q.z), g(q.w));
                }
            }
        } else {
            if constexpr (VPT > 0) {
#pragma unroll
                for (int j = 0; j < VPT; ++j)
                    if (j < nslots) out[j * THREADS + tid] = g(v[j]);
            } else {
                for (int i = tid; i < n; i += THREADS) out[i] = g(row[i]);
            }
        }
    }
};

// bits of the k-th smallest key(x) over the row: four 8-bit radix passes with an LDS histogram
template <int THREADS, int VPT, typename Key>
__device__ __forceinline__ unsigned row_select(const QRow<THREADS, VPT>& row, Key key, unsigned k, unsigned* hist, unsigned* total, unsigned* sh) {
    const unsigned rep = threadIdx.x & (kQReplicas - 1);
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        #pragma unroll 4
        for (int b = threadIdx.x; b < kQBins; b += THREADS) hist[b] = 0;
        __syncthreads();
        row.each([&](float x) {
            const unsigned bits = key(x);
            if ((bits & mask) == prefix) atomicAdd(&hist[((bits >> shift) & 255u) * kQReplicas + rep], 1u);
        });
        __syncthreads();
        if (threadIdx.x < 256) {
            unsigned sum = 0;
            #pragma unroll 4
            for (int j = 0; j < kQReplicas; ++j) sum += hist[threadIdx.x * kQReplicas + ((j + threadIdx.x) & (kQReplicas - 1))];
            total[threadIdx.x] = sum;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // the first bin b with (bins 0..b) > k, 255 if there is none: lane l owns bins 4l..4l+3
            const unsigned a0 = total[4 * threadIdx.x], a1 = total[4 * threadIdx.x + 1], a2 = total[4 * threadIdx.x + 2],
                           a3 = total[4 * threadIdx.x + 3];
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
                sh[0] = prefix | (b << shift);
                sh[1] = k - cum;
            }
        }
        __syncthreads();
        prefix = sh[0];
        k = sh[1];
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

struct QRowArgs {
    const float* x;
    float* out;     // nullptr: statistics only
    float* stats;   // [rows][3] = (nq, max|x|, second statistic), or nullptr
    int64_t rows, inner, rank_lo;
    float rank_frac, nq_fac, eps, pow_fac;
    int op, centered;
};

template <int THREADS, int VPT>
__global__ void __launch_bounds__(THREADS) quantile_rows_kernel(QRowArgs a) {
    kernarg_touch_for(a);
    __shared__ unsigned hist[kQBins];
    __shared__ unsigned total[256];
    __shared__ unsigned sh[2];
    __shared__ float redf[THREADS / 64];
    __shared__ double redd[THREADS / 64];
    __shared__ int redi[THREADS / 64];
    const bool centered = a.centered != 0;
    const int base = a.op & 0xFF;
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        QRow<THREADS, VPT> row;
        row.load(a.x + r * a.inner, (int)a.inner, a.out ? a.out + r * a.inner : nullptr);
        auto fmax_ = [](float p, float q) { return fmaxf(p, q); };
        float mx = 0.0f;
        row.each([&](float x) { mx = fmaxf(mx, fabsf(x)); });
        const float maxabs = block_reduce<THREADS>(mx, fmax_, redf);
        auto pv = [&](float x) { return centered ? centered_proxy(x, maxabs) : x; };

        // nq = torch.quantile(|p|, q) * nq_fac + eps (linear interpolation between order statistics lo and lo + 1)
        const unsigned lo_bits =
            row_select(row, [&](float x) { return __float_as_uint(pv(x)) & 0x7FFFFFFFu; }, (unsigned)a.rank_lo, hist, total, sh);
        unsigned cnt = 0, mn = 0x7FFFFFFFu;
        row.each([&](float x) {
            const unsigned bits = __float_as_uint(pv(x)) & 0x7FFFFFFFu;
            cnt += bits <= lo_bits;
            if (bits > lo_bits) mn = min(mn, bits);
        });
        const unsigned cnt_all = (unsigned)block_reduce<THREADS>((int)cnt, [](int p, int q) { return p + q; }, redi);
        const unsigned mn_all =
            (unsigned)block_reduce<THREADS>((int)mn, [](int p, int q) { return min(p, q); }, redi);  // (keys < 2^31: signed min is fine)
        const float vlo = __uint_as_float(lo_bits);
        const float vhi = (a.rank_lo + 1 < (int64_t)cnt_all || a.rank_lo + 1 >= a.inner) ? vlo : __uint_as_float(mn_all);
        const float nq = __fadd_rn(__fmul_rn(blend<float>(SONAR_BLEND_LERP, vlo, vhi, a.rank_frac), a.nq_fac), a.eps);

        float s2 = 0.0f;
        if (base == kQScaleDown) {
            float m2 = 0.0f;
            if (centered) row.each([&](float x) { m2 = fmaxf(m2, fabsf(pv(x))); });
            const float mv = fmaxf(centered ? block_reduce<THREADS>(m2, fmax_, redf) : maxabs, 1e-6f);
            s2 = nq / mv;
        } else if (base == kQMean) {
            double s = 0.0;
            row.each([&](float x) { s += (double)pv(x); });
            s = block_reduce<THREADS>(s, [](double p, double q) { return p + q; }, redd);
            s2 = (float)(s / (double)a.inner);
        } else if (base == kQMedian) {
            s2 = signed_key_value(row_select(row, [&](float x) { return signed_key(pv(x)); }, (unsigned)((a.inner - 1) / 2), hist, total, sh));
        } else if (base == kQMode1 || base == kQMode2) {
            // mode of round(p, d) over the row's finite values: smallest most frequent rounded value (torch.mode), counted in windows of
            // kQModeWindow keys.  Each counting pass also finds the smallest key above its window, where the next window starts: empty
            // stretches of the key range cost nothing, so the passes are bounded by the occupied windows (at most one per value)
            const float tp = base == kQMode1 ? 10.0f : 100.0f;
            int kmin = 0x7FFFFFFF;
            row.each([&](float x) {
                const float p = pv(x);
                if (isfinite(p)) kmin = min(kmin, mode_key(p, tp));
            });
            kmin = block_reduce<THREADS>(kmin, [](int p, int q) { return min(p, q); }, redi);
            int best_key = kmin, best_cnt = 0;
            for (int64_t w0 = kmin; w0 < 0x7FFFFFFF;) {
                #pragma unroll 4
                for (int b = threadIdx.x; b < kQModeWindow; b += THREADS) hist[b] = 0;
                __syncthreads();
                int next = 0x7FFFFFFF;
                row.each([&](float x) {
                    const float p = pv(x);
                    if (!isfinite(p)) return;
                    const int key = mode_key(p, tp);
                    const int64_t d = (int64_t)key - w0;
                    if (d >= 0 && d < kQModeWindow) atomicAdd(&hist[d], 1u);
                    else if (d >= kQModeWindow) next = min(next, key);
                });
                next = block_reduce<THREADS>(next, [](int p, int q) { return min(p, q); }, redi);  // (its barriers order the tallies too)
                // (count, -bin) maximum: the most frequent, the smallest of equals
                int64_t local = -1;
                #pragma unroll 4
                for (int b = threadIdx.x; b < kQModeWindow; b += THREADS) {
                    const int64_t c = ((int64_t)hist[b] << 32) | (uint32_t)(kQModeWindow - 1 - b);
                    local = local > c ? local : c;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const int64_t o = __shfl_xor(local, off, 64);
                    local = local > o ? local : o;
                }
                if ((threadIdx.x & 63) == 0) reinterpret_cast<int64_t*>(redd)[threadIdx.x >> 6] = local;
                __syncthreads();
                int64_t win = reinterpret_cast<int64_t*>(redd)[0];
                for (int w = 1; w < THREADS / 64; ++w) {
                    const int64_t o = reinterpret_cast<int64_t*>(redd)[w];
                    win = win > o ? win : o;
                }
                __syncthreads();
                const int c = (int)(win >> 32);
                if (c > best_cnt) {
                    best_cnt = c;
                    best_key = (int)(w0 + (kQModeWindow - 1 - (int)(win & 0xFFFFFFFF)));
                }
                w0 = next;
            }
            s2 = best_cnt > 0 ? (float)best_key / tp : __int_as_float(0x7FC00000);  // no finite value: NaN
        }

        if (a.out) {
            const int op = a.op;
            const float pf = a.pow_fac;
            row.map_store(a.out + r * a.inner, [&](float x) { return q_finish_light(q_apply_light(op, pv(x), nq, s2), centered, maxabs, pf); });
        }
        if (a.stats && threadIdx.x == 0) {
            a.stats[3 * r] = nq;
            a.stats[3 * r + 1] = maxabs;
            a.stats[3 * r + 2] = s2;
        }
        __syncthreads();
    }
}

// ---- multi-workgroup route: rows too long to keep on chip, or too few rows to fill the GPU ------------------------------------------
// Every pass is one launch over (chunk, row) workgroups; per row a small state block in global memory carries the radix prefix, the
// rank still to find and a 256-bin histogram from pass to pass; a one-wave-per-row pick kernel narrows the prefix between passes.
constexpr int kMwThreads = 256, kMwChunk = 16384, kMwReplicas = 8;
constexpr int kMwState = 16, kMwRowWords = kMwState + 256;  // state words per row: [0] prefix [1] k [2] count <= prefix [3] min key > prefix
                                                            // [4] max|x| bits [5] max|p| bits; then the histogram
__device__ __forceinline__ unsigned mw_key(int kind, float p) { return kind == 0 ? (__float_as_uint(p) & 0x7FFFFFFFu) : signed_key(p); }

struct QMwArgs {
    const float* x;
    unsigned* ws;
    double* partial;  // [rows][chunks]: per-chunk sums (mean)
    int64_t rows, inner, chunks;
    int centered, kind, shift;
};

// max|x| (pass 0) or max|p| of the centered proxy (pass 1) into the state, as bit patterns (non-negative floats order like integers)
__global__ void __launch_bounds__(kMwThreads) mw_max_kernel(QMwArgs a, int pass) {
    kernarg_touch_for(a, pass);
    __shared__ float red[kMwThreads / 64];
    const int64_t r = blockIdx.y, c0 = (int64_t)blockIdx.x * kMwChunk;
    const float* row = a.x + r * a.inner;
    unsigned* st = a.ws + r * kMwRowWords;
    const float maxabs = __uint_as_float(st[4]);
    float m = 0.0f;
    for (int64_t i = c0 + threadIdx.x; i < min(c0 + kMwChunk, a.inner); i += kMwThreads) {
        const float v = row[i];
        m = fmaxf(m, fabsf(pass == 0 ? v : centered_proxy(v, maxabs)));
    }
    m = block_reduce<kMwThreads>(m, [](float p, float q) { return fmaxf(p, q); }, red);
    if (threadIdx.x == 0) atomicMax(&st[4 + pass], __float_as_uint(m));
}

// one radix pass: keys matching the row's prefix above `shift`, binned by their byte at `shift`, added to the row's histogram
__global__ void __launch_bounds__(kMwThreads) mw_hist_kernel(QMwArgs a) {
    kernarg_touch_for(a);
    __shared__ unsigned hist[256 * kMwReplicas];
    const int64_t r = blockIdx.y, c0 = (int64_t)blockIdx.x * kMwChunk;
    const float* row = a.x + r * a.inner;
    unsigned* st = a.ws + r * kMwRowWords;
    const unsigned prefix = st[0], mask = a.shift == 24 ? 0u : ~((1u << (a.shift + 8)) - 1u);
    const float maxabs = __uint_as_float(st[4]);
    for (int b = threadIdx.x; b < 256 * kMwReplicas; b += kMwThreads) hist[b] = 0;
    __syncthreads();
    const unsigned rep = threadIdx.x & (kMwReplicas - 1);
    for (int64_t i = c0 + threadIdx.x; i < min(c0 + kMwChunk, a.inner); i += kMwThreads) {
        const float v = row[i];
        const unsigned key = mw_key(a.kind, a.centered ? centered_proxy(v, maxabs) : v);
        if ((key & mask) == prefix) atomicAdd(&hist[((key >> a.shift) & 255u) * kMwReplicas + rep], 1u);
    }
    __syncthreads();
    unsigned sum = 0;
    for (int j = 0; j < kMwReplicas; ++j) sum += hist[threadIdx.x * kMwReplicas + j];
    if (sum) atomicAdd(&st[kMwState + threadIdx.x], sum);
}

// one wave per row: the bin holding rank k, the prefix and rank narrowed to it; the histogram cleared for the next pass
__global__ void __launch_bounds__(64) mw_pick_kernel(QMwArgs a) {
    kernarg_touch_for(a);
    unsigned* st = a.ws + (int64_t)blockIdx.x * kMwRowWords;
    unsigned* h = st + kMwState;
    const unsigned k = st[1], l = threadIdx.x;
    const unsigned a0 = h[4 * l], a1 = h[4 * l + 1], a2 = h[4 * l + 2], a3 = h[4 * l + 3];
    const unsigned own = a0 + a1 + a2 + a3;
    unsigned incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off, 64);
        if ((int)l >= off) incl += up;
    }
    const unsigned excl = incl - own;
    h[4 * l] = 0; h[4 * l + 1] = 0; h[4 * l + 2] = 0; h[4 * l + 3] = 0;
    if ((excl <= k && k < incl) || (l == 63 && k >= incl)) {
        unsigned cum = excl, b = 4 * l;
        if (cum + a0 <= k) {
            cum += a0; ++b;
            if (cum + a1 <= k) {
                cum += a1; ++b;
                if (cum + a2 <= k) { cum += a2; ++b; }
            }
        }
        st[0] |= b << a.shift;
        st[1] = k - cum;
    }
}

// after the |p| select: how many keys are <= the selected one, and the smallest key above it (the next order statistic)
__global__ void __launch_bounds__(kMwThreads) mw_next_kernel(QMwArgs a) {
    kernarg_touch_for(a);
    __shared__ int red[kMwThreads / 64];
    const int64_t r = blockIdx.y, c0 = (int64_t)blockIdx.x * kMwChunk;
    const float* row = a.x + r * a.inner;
    unsigned* st = a.ws + r * kMwRowWords;
    const unsigned lo = st[0];
    const float maxabs = __uint_as_float(st[4]);
    int cnt = 0, mn = 0x7FFFFFFF;
    for (int64_t i = c0 + threadIdx.x; i < min(c0 + kMwChunk, a.inner); i += kMwThreads) {
        const float v = row[i];
        const unsigned key = mw_key(0, a.centered ? centered_proxy(v, maxabs) : v);
        cnt += key <= lo;
        if (key > lo) mn = min(mn, (int)key);
    }
    cnt = block_reduce<kMwThreads>(cnt, [](int p, int q) { return p + q; }, red);
    mn = block_reduce<kMwThreads>(mn, [](int p, int q) { return min(p, q); }, red);
    if (threadIdx.x == 0) {
        atomicAdd(&st[2], (unsigned)cnt);
        atomicMin(&st[3], (unsigned)mn);
    }
}

// per-chunk sums of p (the mean), in a fixed order: no floating-point atomics
__global__ void __launch_bounds__(kMwThreads) mw_sum_kernel(QMwArgs a) {
    kernarg_touch_for(a);
    __shared__ double red[kMwThreads / 64];
    const int64_t r = blockIdx.y, c0 = (int64_t)blockIdx.x * kMwChunk;
    const float* row = a.x + r * a.inner;
    const float maxabs = __uint_as_float(a.ws[r * kMwRowWords + 4]);
    double s = 0.0;
    for (int64_t i = c0 + threadIdx.x; i < min(c0 + kMwChunk, a.inner); i += kMwThreads) {
        const float v = row[i];
        s += (double)(a.centered ? centered_proxy(v, maxabs) : v);
    }
    s = block_reduce<kMwThreads>(s, [](double p, double q) { return p + q; }, red);
    if (threadIdx.x == 0) a.partial[r * a.chunks + blockIdx.x] = s;
}

// state of every row: prefix 0, rank k, no count, no minimum above, max|x| = max|p| = 0, empty histogram
__global__ void __launch_bounds__(kMwThreads) mw_init_kernel(QMwArgs a, int64_t k) {
    kernarg_touch_for(a, k);
    unsigned* st = a.ws + (int64_t)blockIdx.x * kMwRowWords;
    for (int i = threadIdx.x; i < kMwRowWords; i += kMwThreads) st[i] = i == 1 ? (unsigned)k : i == 3 ? 0x7FFFFFFFu : 0u;
}

// nq from the two order statistics; the state re-armed for a signed select of rank k2 (the median)
__global__ void __launch_bounds__(kMwThreads) mw_nq_kernel(QMwArgs a, int64_t rank_lo, float frac, float nq_fac, float eps, float* stats,
                                                           int64_t k2) {
    kernarg_touch_for(a, rank_lo, frac, nq_fac, eps, stats, k2);
    const int64_t r = (int64_t)blockIdx.x * kMwThreads + threadIdx.x;
    if (r >= a.rows) return;
    unsigned* st = a.ws + r * kMwRowWords;
    const float vlo = __uint_as_float(st[0]);
    const float vhi = (rank_lo + 1 < (int64_t)st[2] || rank_lo + 1 >= a.inner) ? vlo : __uint_as_float(st[3]);
    stats[3 * r] = __fadd_rn(__fmul_rn(blend<float>(SONAR_BLEND_LERP, vlo, vhi, frac), nq_fac), eps);
    stats[3 * r + 1] = __uint_as_float(st[4]);
    st[0] = 0;
    st[1] = (unsigned)k2;
}

// the second statistic of the row into stats[3 * r + 2]
__global__ void __launch_bounds__(kMwThreads) mw_final_kernel(QMwArgs a, int op, float* stats) {
    kernarg_touch_for(a, op, stats);
    const int64_t r = (int64_t)blockIdx.x * kMwThreads + threadIdx.x;
    if (r >= a.rows) return;
    const unsigned* st = a.ws + r * kMwRowWords;
    const int base = op & 0xFF;
    float s2 = 0.0f;
    if (base == kQScaleDown) {
        s2 = stats[3 * r] / fmaxf(__uint_as_float(st[a.centered ? 5 : 4]), 1e-6f);
    } else if (base == kQMean) {
        double s = 0.0;
        for (int64_t c = 0; c < a.chunks; ++c) s += a.partial[r * a.chunks + c];
        s2 = (float)(s / (double)a.inner);
    } else if (base == kQMedian) {
        s2 = signed_key_value(st[0]);
    }
    stats[3 * r + 2] = s2;
}

// Rows beyond the register-resident length take this route, however few they are (one row of 33.5 M values: 30.7 ms on one workgroup,
// 0.41 ms split).  Few resident-length rows stay on the row kernel: 8 rows of 64 Ki took 93 us split, launch-bound across ~14 passes,
// against 44 us for the one-workgroup-per-row composition.  mode_* keeps the row kernel (its window search is row-local).
bool mw_route(int64_t rows, int64_t inner, int op) {
    const int base = op & 0xFF;
    if (base == kQMode1 || base == kQMode2) return false;
    return rows > 0 && inner > kQResidentMax;
}

int64_t mw_ws_bytes(int64_t rows, int64_t inner) {
    const int64_t chunks = (inner + kMwChunk - 1) / kMwChunk;
    return rows * kMwRowWords * 4 + 8 + rows * chunks * 8;
}

void mw_stats(const float* x, int64_t rows, int64_t inner, int64_t rank_lo, float frac, float nq_fac, float eps, int op, int centered,
              float* stats, void* ws, hipStream_t st) {
    const int64_t chunks = (inner + kMwChunk - 1) / kMwChunk;
    unsigned* w = static_cast<unsigned*>(ws);
    double* partial = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(w + rows * kMwRowWords) + 7) & ~uintptr_t(7));
    QMwArgs a{x, w, partial, rows, inner, chunks, centered, 0, 24};
    const dim3 grid((unsigned)chunks, (unsigned)rows), rgrid((unsigned)((rows + kMwThreads - 1) / kMwThreads));
    const int base = op & 0xFF;
    hipLaunchKernelGGL(mw_init_kernel, dim3((unsigned)rows), dim3(kMwThreads), 0, st, a, rank_lo);
    hipLaunchKernelGGL(mw_max_kernel, grid, dim3(kMwThreads), 0, st, a, 0);
    auto select = [&](int kind) {
        a.kind = kind;
        for (int shift = 24; shift >= 0; shift -= 8) {
            a.shift = shift;
            hipLaunchKernelGGL(mw_hist_kernel, grid, dim3(kMwThreads), 0, st, a);
            hipLaunchKernelGGL(mw_pick_kernel, dim3((unsigned)rows), dim3(64), 0, st, a);
        }
    };
    select(0);
    hipLaunchKernelGGL(mw_next_kernel, grid, dim3(kMwThreads), 0, st, a);
    hipLaunchKernelGGL(mw_nq_kernel, rgrid, dim3(kMwThreads), 0, st, a, rank_lo, frac, nq_fac, eps, stats, (inner - 1) / 2);
    if (base == kQScaleDown && centered) hipLaunchKernelGGL(mw_max_kernel, grid, dim3(kMwThreads), 0, st, a, 1);
    if (base == kQMean) hipLaunchKernelGGL(mw_sum_kernel, grid, dim3(kMwThreads), 0, st, a);
    if (base == kQMedian) select(1);
    hipLaunchKernelGGL(mw_final_kernel, rgrid, dim3(kMwThreads), 0, st, a, op, stats);
}

// the strategies of !q_light, elementwise over rows of `inner` values, from the row statistics
__global__ void __launch_bounds__(kBlock) quantile_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats, int64_t n,
                                                                 int64_t inner, int op, int centered, float pow_fac, float* out) {
    kernarg_touch_for(x, stats, n, inner, op, centered, pow_fac, out);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / inner;
        const float nq = stats[3 * r], maxabs = stats[3 * r + 1], s2 = stats[3 * r + 2];
        const float v = x[i];
        const float p = centered ? centered_proxy(v, maxabs) : v;
        out[i] = q_finish(q_apply(op, p, nq, s2), centered != 0, maxabs, pow_fac);
    }
}

// ---- replace*: compaction, in memory order, of the values with |p| <= nq over the WHOLE tensor ---------------------------------------
// element i belongs to statistics row (i / (len * stride)) * stride + i % stride (the row runs along one dim of length `len`, `stride`
// elements apart; contiguous rows: stride 1)
constexpr int kRepThreads = 256, kRepPer = 16, kRepChunk = kRepThreads * kRepPer;

struct QRepArgs {
    const float* x;
    const float* stats;
    float* cand;
    int64_t* counts;  // [chunks + 1]: per-chunk counts, then (after the scan) exclusive offsets and the total at [chunks]
    float* out;
    int64_t n, len, stride, chunks;
    float pow_fac;
    int centered, count, flip, sign_mode;  // sign_mode 0 none, 1 keep, 2 avoid
};

__device__ __forceinline__ float rep_proxy(const QRepArgs& a, int64_t i, float& nq, float& maxabs) {
    const int64_t row = (i / (a.len * a.stride)) * a.stride + i % a.stride;
    nq = a.stats[3 * row];
    maxabs = a.stats[3 * row + 1];
    const float x = a.x[i];
    return a.centered ? centered_proxy(x, maxabs) : x;
}

__global__ void __launch_bounds__(kRepThreads) replace_count_kernel(QRepArgs a) {
    kernarg_touch_for(a);
    __shared__ int red[kRepThreads / 64];
    const int64_t c0 = (int64_t)blockIdx.x * kRepChunk;
    int cnt = 0;
    for (int j = threadIdx.x; j < kRepChunk; j += kRepThreads) {
        const int64_t i = c0 + j;
        if (i < a.n) {
            float nq, mx;
            cnt += fabsf(rep_proxy(a, i, nq, mx)) <= nq;
        }
    }
    cnt = block_reduce<kRepThreads>(cnt, [](int p, int q) { return p + q; }, red);
    if (threadIdx.x == 0) a.counts[blockIdx.x] = cnt;
}

// exclusive scan of the chunk counts in place (one workgroup); counts[chunks] = the total
__global__ void __launch_bounds__(1024) replace_scan_kernel(QRepArgs a) {
    kernarg_touch_for(a);
    __shared__ int64_t part[1024];
    const int64_t per = (a.chunks + 1023) / 1024, b0 = threadIdx.x * per;
    int64_t s = 0;
    for (int64_t b = b0; b < b0 + per && b < a.chunks; ++b) s += a.counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t up = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += up;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - s;
    for (int64_t b = b0; b < b0 + per && b < a.chunks; ++b) {
        const int64_t c = a.counts[b];
        a.counts[b] = run;
        run += c;
    }
    if (threadIdx.x == 1023) a.counts[a.chunks] = part[1023];
}

// each thread owns kRepPer consecutive elements of the chunk; an in-order block scan of the per-thread counts places them
__global__ void __launch_bounds__(kRepThreads) replace_scatter_kernel(QRepArgs a) {
    kernarg_touch_for(a);
    __shared__ int part[kRepThreads];
    const int64_t i0 = (int64_t)blockIdx.x * kRepChunk + (int64_t)threadIdx.x * kRepPer;
    int cnt = 0;
    for (int j = 0; j < kRepPer; ++j) {
        const int64_t i = i0 + j;
        if (i < a.n) {
            float nq, mx;
            cnt += fabsf(rep_proxy(a, i, nq, mx)) <= nq;
        }
    }
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 1; off < kRepThreads; off <<= 1) {
        const int up = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += up;
        __syncthreads();
    }
    int64_t pos = a.counts[blockIdx.x] + part[threadIdx.x] - cnt;
    for (int j = 0; j < kRepPer; ++j) {
        const int64_t i = i0 + j;
        if (i < a.n) {
            float nq, mx;
            const float p = rep_proxy(a, i, nq, mx);
            if (fabsf(p) <= nq) a.cand[pos++] = p;
        }
    }
}

// out[j] = p[j] in range, else the mean over k < count of cand[((j - s_k) mod n) mod n_cand] (s_k = k, -k for odd k when flipping)
__global__ void __launch_bounds__(kBlock) replace_apply_kernel(QRepArgs a) {
    kernarg_touch_for(a);
    const int64_t nc = a.counts[a.chunks];
    if (nc <= 0) return;  // the host refuses this case (the reference divides by zero)
    const float m = 1.0f / (float)a.count;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * kBlock) {
        float nq, maxabs;
        const float p = rep_proxy(a, j, nq, maxabs);
        float o = p;
        if (!(fabsf(p) <= nq)) {
            if (a.count < 2) {
                o = a.cand[j % nc];
            } else {
                o = __fmul_rn(a.cand[j % nc], m);
                for (int k = 1; k < a.count; ++k) {
                    const int64_t s = (a.flip && (k & 1)) ? -k : k;
                    int64_t idx = (j - s) % a.n;
                    if (idx < 0) idx += a.n;
                    o = __fadd_rn(o, __fmul_rn(a.cand[idx % nc], m));
                }
            }
            if (a.sign_mode == 1) o = copysignf(o, p);
            else if (a.sign_mode == 2) o = copysignf(o, -p);
        }
        a.out[j] = q_finish(o, a.centered != 0, maxabs, a.pow_fac);
    }
}

bool q_op_ok(int op) {
    const int base = op & 0xFF, flags = op >> 8;
    if (base == kQWave) return flags >= 0 && flags < 16;
    return base >= 0 && base < kQWave && flags == 0;
}

}  // namespace

}  // namespace sonar

using namespace sonar;

extern "C" int64_t sonar_quantile_rows_ws_bytes(int64_t rows, int64_t inner, int op) {
    if (rows < 0 || inner <= 0) return -1;
    return mw_route(rows, inner, op) ? mw_ws_bytes(rows, inner) : 0;
}

extern "C" int sonar_quantile_rows_f32(const float* x, int64_t rows, int64_t inner, int64_t rank_lo, float rank_frac, float nq_fac,
                                       float eps, int op, int centered, float pow_fac, float* out, float* stats, void* ws, void* stream) {
    SONAR_REQUIRE(x && stats && rows >= 0 && inner > 0 && rank_lo >= 0 && rank_lo < inner && rank_frac >= 0.0f &&
                      rank_frac <= 1.0f && q_op_ok(op) && (centered == 0 || centered == 1) && inner < ((int64_t)1 << 31),
                  SONAR_ERR_ARG, "sonar_quantile_rows_f32: bad argument");
    if (rows == 0) return SONAR_OK;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t n = rows * inner;
    if (mw_route(rows, inner, op)) {
        SONAR_REQUIRE(ws && rows < 65536, SONAR_ERR_ARG, "sonar_quantile_rows_f32: this shape needs the workspace (sonar_quantile_rows_ws_bytes)");
        mw_stats(x, rows, inner, rank_lo, rank_frac, nq_fac, eps, op, centered, stats, ws, st);
        if (out) hipLaunchKernelGGL(quantile_apply_kernel, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, st, x, stats, n, inner, op, centered,
                                    pow_fac, out);
        return check_launch("sonar_quantile_rows_f32");
    }
    const bool fused = out && q_light(op, pow_fac);
    const QRowArgs a{x, fused ? out : nullptr, stats, rows, inner, rank_lo, rank_frac, nq_fac, eps, pow_fac, op, centered};
    const dim3 grid((unsigned)std::min<int64_t>(rows, 65535));  // (the kernel loops over further rows)
    if (inner <= 1024) hipLaunchKernelGGL((quantile_rows_kernel<256, 4>), grid, dim3(256), 0, st, a);
    else if (inner <= kQRowThreads * 16) hipLaunchKernelGGL((quantile_rows_kernel<kQRowThreads, 16>), grid, dim3(kQRowThreads), 0, st, a);
    else if (inner <= kQResidentMax) hipLaunchKernelGGL((quantile_rows_kernel<kQRowThreads, 64>), grid, dim3(kQRowThreads), 0, st, a);
    else hipLaunchKernelGGL((quantile_rows_kernel<kQRowThreads, 0>), grid, dim3(kQRowThreads), 0, st, a);
    if (out && !fused)
        hipLaunchKernelGGL(quantile_apply_kernel, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, st, x, stats, n, inner, op, centered, pow_fac,
                           out);
    return check_launch("sonar_quantile_rows_f32");
}

extern "C" int64_t sonar_quantile_replace_ws_elems(int64_t n) {
    return n < 0 ? -1 : (n + kRepChunk - 1) / kRepChunk + 1;
}

extern "C" int sonar_quantile_replace_compact_f32(const float* x, const float* stats, int64_t n, int64_t len, int64_t stride, int centered,
                                                  float* cand, int64_t* counts, void* stream) {
    SONAR_REQUIRE(x && stats && cand && counts && n > 0 && len > 0 && stride > 0 && n % (len * stride) == 0 &&
                      (centered == 0 || centered == 1),
                  SONAR_ERR_ARG, "sonar_quantile_replace_compact_f32: bad argument");
    const int64_t chunks = (n + kRepChunk - 1) / kRepChunk;
    const QRepArgs a{x, stats, cand, counts, nullptr, n, len, stride, chunks, 0.0f, centered, 1, 0, 0};
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(replace_count_kernel, dim3((unsigned)chunks), dim3(kRepThreads), 0, st, a);
    hipLaunchKernelGGL(replace_scan_kernel, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(replace_scatter_kernel, dim3((unsigned)chunks), dim3(kRepThreads), 0, st, a);
    return check_launch("sonar_quantile_replace_compact_f32");
}

extern "C" int sonar_quantile_replace_apply_f32(const float* x, const float* stats, int64_t n, int64_t len, int64_t stride, int centered,
                                                const float* cand, const int64_t* counts, int count, int flip, int sign_mode,
                                                float pow_fac, float* out, void* stream) {
    SONAR_REQUIRE(x && stats && cand && counts && out && n > 0 && len > 0 && stride > 0 && n % (len * stride) == 0 &&
                      (centered == 0 || centered == 1) && count >= 1 && count <= 64 && (flip == 0 || flip == 1) && sign_mode >= 0 &&
                      sign_mode <= 2,
                  SONAR_ERR_ARG, "sonar_quantile_replace_apply_f32: bad argument");
    const int64_t chunks = (n + kRepChunk - 1) / kRepChunk;
    const QRepArgs a{x, stats, const_cast<float*>(cand), const_cast<int64_t*>(counts), out, n, len, stride, chunks, pow_fac, centered,
                     count, flip, sign_mode};
    hipLaunchKernelGGL(replace_apply_kernel, dim3(grid_for(n, kBlock * 4)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("sonar_quantile_replace_apply_f32");
}
