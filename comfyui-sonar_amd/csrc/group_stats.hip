// Statistics and per-group updates over the groups of ANY subset of a tensor's dimensions (torch.mean / torch.std / amin / amax with
// dim = a tuple, keepdim = True), on the contiguous fp32 tensor as it lies: no transposed copy.
//
// The caller collapses (shape, reduced dims) into at most six ALTERNATING segments, outermost first: adjacent dimensions of one kind
// merged, size-1 dimensions dropped.  Segment k is reduced when (k odd) != first_reduced.  A "group" is one coordinate of the kept
// segments, numbered row-major over them (the flattened keepdim=True layout); its members are the R coordinates of the reduced segments,
// numbered row-major as well ("e").  Element (g, e) lives at base(g) + offset(e): both are sums of coordinate x stride over the segments of
// one kind, so an index is taken apart with one division per segment -- by a constant the host turned into a multiply and a shift (the
// segment table travels in the kernel's argument block; tensors stay below 2^31 elements, where the 32-bit form is exact).
//
// Two sweeps, both coalesced:
//   innermost segment REDUCED  a group's members come in contiguous runs: a wave owns a (group, slice of e), its lanes take consecutive e;
//   innermost segment KEPT     consecutive groups are consecutive addresses: a lane owns a group (of a slice of e) and walks e, the
//                              wave's 64 loads of one e are one 256-byte line.
// Few groups with many members each would leave the chip idle (dims = (0, 2, 3) of 512 x 4 x 128 x 128: 4 groups of 8.4 M), so the
// members are cut into S slices (split_of below), every (group, slice) leaves its partial results in the workspace and a second launch
// adds them in slice order: a function of the shape alone, so two runs give the same bits (no atomics).
//
// Accumulation: rowstats_kernel's (rows.hip) -- sum and sum of squares in fp64 (a product of two floats is exact in a double), mean
// = s / n, var = (q - s * mean) / (n - 1), the one tail both share (mean_std_of, common.h) -- with the partial sums of lanes, waves and
// slices added in fp64 in a fixed order.  n == 1 gives 0 / 0 = NaN like torch.  Min / max are fminf / fmaxf folds as in minmax_rows_kernel
// (a NaN never wins), the peak torch.amax's (a NaN poisons); a wave joins its lanes through range_reduce.h, where both rules are stated.
//
// The same two sweeps carry two more per-group results (the `X` parameter of the kernels):
//   peak          amax of x or of |x| with torch.amax's NaN (amax_mid_kernel's fold): PowerLawNoiseGenerator's div_max_dims over any dims,
//                 followed by x / peak[g] in place (group_div_kernel);
//   divided mean  the mean of x / d[g], every quotient rounded to fp32 first and added in fp64: scale_rows_kernel's second statistic, so
//                 that scale_noise(normalize_dims=...) over any dims is group_stats (std) -> divided mean -> group_scale_noise_kernel.
#include "common.h"
#include "range_reduce.h"

namespace sonar {
namespace {

constexpr int kMaxSegs = SONAR_GROUP_MAX_SEGMENTS;
// split rule (see split_of)
constexpr uint32_t kRunSlice = 1024;    // innermost reduced: a wave's slice is at least 16 loads per lane ...
constexpr uint32_t kRunItems = 8192;    // ... and slices are cut until 8192 waves have work (256 CUs x 8 workgroups x 4 waves)
constexpr uint32_t kLaneSlice = 64;     // innermost kept: a lane's slice is at least 64 members ...
constexpr uint32_t kLaneBlocks = 1024;  // ... and slices are cut until 1024 workgroups have work (4 per CU)

struct Segs {
    uint32_t size[kMaxSegs];     // outermost first
    uint32_t stride[kMaxSegs];   // elements between two coordinates of the segment
    uint32_t gstride[kMaxSegs];  // kept segments: groups between two coordinates
    uint32_t magic[kMaxSegs], shift[kMaxSegs];  // n / size = (umulhi(n, magic) + n) >> shift for n < 2^31
    int nseg, first_reduced;
};

__device__ __forceinline__ bool seg_reduced(const Segs& sg, int k) { return ((k & 1) != 0) != (sg.first_reduced != 0); }
__device__ __forceinline__ uint32_t seg_div(const Segs& sg, int k, uint32_t n) { return (__umulhi(n, sg.magic[k]) + n) >> sg.shift[k]; }

// offset of coordinate `v` (row-major over the segments of one kind) from the tensor's first element
template <bool REDUCED>
__device__ __forceinline__ uint32_t offset_of(const Segs& sg, uint32_t v) {
    uint32_t off = 0;
#pragma unroll
    for (int k = kMaxSegs - 1; k >= 0; --k) {
        if (k < sg.nseg && seg_reduced(sg, k) == REDUCED) {
            const uint32_t q = seg_div(sg, k, v);
            off += (v - q * sg.size[k]) * sg.stride[k];
            v = q;
        }
    }
    return off;
}

// group of flat element i
__device__ __forceinline__ uint32_t group_of(const Segs& sg, uint32_t i) {
    uint32_t g = 0;
#pragma unroll
    for (int k = kMaxSegs - 1; k >= 0; --k) {
        if (k < sg.nseg) {
            const uint32_t q = seg_div(sg, k, i);
            if (!seg_reduced(sg, k)) g += (i - q * sg.size[k]) * sg.gstride[k];
            i = q;
        }
    }
    return g;
}

constexpr int kPlain = 0, kPeak = 1, kPeakAbs = 2, kDivMean = 3;  // X: what else a sweep accumulates (MS and MM false; kDivMean: MS alone)

template <bool MS, bool MM, int X = kPlain>
struct Acc {
    double s = 0.0, q = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    float d = 1.0f;    // kDivMean: the group's divisor
    bool nan = false;  // kPeak / kPeakAbs: a member was NaN
    __device__ __forceinline__ void add(float f) {
        if constexpr (X == kDivMean) {
            s += (double)(f / d);
        } else if constexpr (X != kPlain) {
            fold(X == kPeakAbs ? fabsf(f) : f);
        } else {
            if constexpr (MS) {
                const double v = f;
                s += v;
                q += v * v;
            }
            if constexpr (MM) {
                lo = fminf(lo, f);
                hi = fmaxf(hi, f);
            }
        }
    }
    // kPeak / kPeakAbs: another lane's, wave's or slice's peak() joins
    __device__ __forceinline__ void fold(float v) {
        nan |= v != v;
        hi = fmaxf(hi, v);
    }
    __device__ __forceinline__ float peak() const { return nan_poisons(nan, hi); }  // torch.amax propagates NaN
};

// what a (group, slice) leaves: the final values (S == 1) or its partials, plane p of the workspace at ws[(p * S + slice) * G + g]
// (kPeak / kPeakAbs: the peak goes to hi, one plane; kDivMean: the mean to `mean`, one plane)
template <bool MS, bool MM, int X>
__device__ __forceinline__ void leave(const Acc<MS, MM, X>& a, uint32_t g, uint32_t sl, uint32_t G, uint32_t R, uint32_t S, float* mean,
                                      float* stdv, float* lo, float* hi, double* ws) {
    if constexpr (X == kDivMean) {
        if (S == 1) mean[g] = (float)(a.s / (double)R);
        else ws[(size_t)sl * G + g] = a.s;
        return;
    } else if constexpr (X != kPlain) {
        if (S == 1) hi[g] = a.peak();
        else ws[(size_t)sl * G + g] = (double)a.peak();
        return;
    }
    if (S == 1) {
        if constexpr (MS) {
            const MeanStd ms = mean_std_of(a.s, a.q, (double)R);
            mean[g] = ms.mean;
            stdv[g] = ms.stdv;
        }
        if constexpr (MM) {
            lo[g] = a.lo;
            hi[g] = a.hi;
        }
        return;
    }
    const size_t plane = (size_t)S * G, at = (size_t)sl * G + g;
    if constexpr (MS) {
        ws[at] = a.s;
        ws[plane + at] = a.q;
    }
    if constexpr (MM) {
        ws[(MS ? 2 : 0) * plane + at] = (double)a.lo;
        ws[(MS ? 3 : 1) * plane + at] = (double)a.hi;
    }
}

// innermost segment reduced: a wave per (group, slice), lanes over consecutive members
template <bool MS, bool MM, int X = kPlain>
__global__ void __launch_bounds__(kBlock) group_stats_runs_kernel(const float* __restrict__ x, Segs sg, uint32_t G, uint32_t R, uint32_t S,
                                                                   uint32_t chunk, float* mean, float* stdv, float* lo, float* hi, double* ws) {
    kernarg_touch_for(x, sg, G, R, S, chunk, mean, stdv, lo, hi, ws);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t items = (uint64_t)G * S, nwaves = (uint64_t)gridDim.x * (kBlock / 64);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); item < items; item += nwaves) {
        const uint32_t g = (uint32_t)(item / S), sl = (uint32_t)(item - (uint64_t)g * S);
        const float* base = x + offset_of<false>(sg, g);
        const uint32_t e0 = sl * chunk, e1 = min(R, e0 + chunk);  // e0 < R: no slice is empty (split_of)
        Acc<MS, MM, X> a;
        if constexpr (X == kDivMean) a.d = stdv[g];  // (the divisor table comes in stdv's place)
        uint32_t e = e0 + lane;
        for (; e + 3 * 64 < e1; e += 4 * 64) {  // four independent loads per lane in flight
            const float v0 = base[offset_of<true>(sg, e)], v1 = base[offset_of<true>(sg, e + 64)];
            const float v2 = base[offset_of<true>(sg, e + 128)], v3 = base[offset_of<true>(sg, e + 192)];
            a.add(v0); a.add(v1); a.add(v2); a.add(v3);
        }
        for (; e < e1; e += 64) a.add(base[offset_of<true>(sg, e)]);
        if constexpr (MS) {
            a.s = wave_sum(a.s);
            if constexpr (X == kPlain) a.q = wave_sum(a.q);
        }
        if constexpr (MM) {  // a NaN never wins
            a.lo = wave_min(a.lo);
            a.hi = wave_max(a.hi);
        }
        if constexpr (X == kPeak || X == kPeakAbs) {  // a NaN poisons: the flag travels beside the maximum
            a.hi = wave_max(a.hi);
            a.nan = wave_or(a.nan) != 0;
        }
        if (lane == 0) leave<MS, MM, X>(a, g, sl, G, R, S, mean, stdv, lo, hi, ws);
    }
}

// innermost segment kept: a lane per (group, slice), workgroups over 256 consecutive groups
template <bool MS, bool MM, int X = kPlain>
__global__ void __launch_bounds__(kBlock) group_stats_lanes_kernel(const float* __restrict__ x, Segs sg, uint32_t G, uint32_t R, uint32_t S,
                                                                    uint32_t chunk, float* mean, float* stdv, float* lo, float* hi, double* ws) {
    kernarg_touch_for(x, sg, G, R, S, chunk, mean, stdv, lo, hi, ws);
    const uint32_t gblocks = (G + kBlock - 1) / kBlock;
    const uint64_t items = (uint64_t)gblocks * S;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t sl = (uint32_t)(item / gblocks), gb = (uint32_t)(item - (uint64_t)sl * gblocks);
        const uint32_t g = gb * kBlock + threadIdx.x;
        if (g >= G) continue;
        const float* base = x + offset_of<false>(sg, g);
        const uint32_t e0 = sl * chunk, e1 = min(R, e0 + chunk);
        Acc<MS, MM, X> a;
        if constexpr (X == kDivMean) a.d = stdv[g];
        uint32_t e = e0;  // the same for every lane: the offsets below are the wave's, not the lane's
        for (; e + 3 < e1; e += 4) {
            const float v0 = base[offset_of<true>(sg, e)], v1 = base[offset_of<true>(sg, e + 1)];
            const float v2 = base[offset_of<true>(sg, e + 2)], v3 = base[offset_of<true>(sg, e + 3)];
            a.add(v0); a.add(v1); a.add(v2); a.add(v3);
        }
        for (; e < e1; ++e) a.add(base[offset_of<true>(sg, e)]);
        leave<MS, MM, X>(a, g, sl, G, R, S, mean, stdv, lo, hi, ws);
    }
}

// the slices of a group, added in slice order
template <bool MS, bool MM, int X = kPlain>
__global__ void __launch_bounds__(kBlock) group_stats_combine_kernel(const double* __restrict__ ws, uint32_t G, uint32_t R, uint32_t S,
                                                                      float* mean, float* stdv, float* lo, float* hi) {
    kernarg_touch_for(ws, G, R, S, mean, stdv, lo, hi);
    const size_t plane = (size_t)S * G;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < G; g += (uint64_t)gridDim.x * kBlock) {
        Acc<MS, MM, X> a;
        if constexpr (X != kPlain) {  // one plane
            for (uint32_t sl = 0; sl < S; ++sl) {
                const double v = ws[(size_t)sl * G + g];
                if constexpr (X == kDivMean) a.s += v;
                else a.fold((float)v);
            }
            if constexpr (X == kDivMean) mean[g] = (float)(a.s / (double)R);
            else hi[g] = a.peak();
            continue;
        }
        for (uint32_t sl = 0; sl < S; ++sl) {
            const size_t at = (size_t)sl * G + g;
            if constexpr (MS) {
                a.s += ws[at];
                a.q += ws[plane + at];
            }
            if constexpr (MM) {
                a.lo = fminf(a.lo, (float)ws[(MS ? 2 : 0) * plane + at]);
                a.hi = fmaxf(a.hi, (float)ws[(MS ? 3 : 1) * plane + at]);
            }
        }
        if constexpr (MS) {
            const MeanStd ms = mean_std_of(a.s, a.q, (double)R);
            mean[g] = ms.mean;
            stdv[g] = ms.stdv;
        }
        if constexpr (MM) {
            lo[g] = a.lo;
            hi[g] = a.hi;
        }
    }
}

// sonar_row_affine_f32's two operations with the operands of the element's group (a NULL a is 0, a NULL b is 1)
__global__ void __launch_bounds__(kBlock) group_affine_kernel(int op, const float* x, Segs sg, uint32_t total, const float* __restrict__ a,
                                                               const float* __restrict__ b, float* out) {
    kernarg_touch_for(op, x, sg, total, a, b, out);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t g = group_of(sg, (uint32_t)i);
        out[i] = row_affine_value(op, x[i], a ? a[g] : 0.0f, b ? b[g] : 1.0f);
    }
}

// sonar_minmax_rescale_f32's arithmetic with the (lo, hi) of the element's group
__global__ void __launch_bounds__(kBlock) group_minmax_rescale_kernel(const float* x, Segs sg, uint32_t total, const float* __restrict__ lo,
                                                                       const float* __restrict__ hi, float eps, float tmin, float tmax, float span,
                                                                       float* out) {
    kernarg_touch_for(x, sg, total, lo, hi, eps, tmin, tmax, span, out);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t g = group_of(sg, (uint32_t)i);
        out[i] = minmax_rescale_value(x[i], lo[g], hi[g], eps, tmin, tmax, span);
    }
}

// PowerLawNoiseGenerator's `noise /= amax(...)` (py/noise_generation.py:780-785) with the peak of the element's group: a true division
__global__ void __launch_bounds__(kBlock) group_div_kernel(float* x, Segs sg, uint32_t total, const float* __restrict__ d) {
    kernarg_touch_for(x, sg, total, d);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock)
        x[i] = x[i] / d[group_of(sg, (uint32_t)i)];
}

// scale_rows_kernel's last pass (rows.hip; py/utils.py:97-99) with the (std, mean of x / std) of the element's group
__global__ void __launch_bounds__(kBlock) group_scale_noise_kernel(float* x, Segs sg, uint32_t total, const float* __restrict__ sd,
                                                                    const float* __restrict__ mean, float factor) {
    kernarg_touch_for(x, sg, total, sd, mean, factor);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint32_t g = group_of(sg, (uint32_t)i);
        x[i] = (x[i] / sd[g] - mean[g]) * factor;
    }
}

// NormalizeToScaleNoise's two per-group scalars (py/noise.py:1288-1296), each step rounded on its own as the reference's tensor ops are:
// op 0: v * k   op 1: t = (v - 1) * k + 1, 1e-07 where t == 0 (a NaN is not 0 and stays)
__global__ void __launch_bounds__(kBlock) group_adjust_kernel(int op, const float* v, int64_t n, float k, float* out) {
    kernarg_touch_for(op, v, n, k, out);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (op == 0) {
            out[i] = v[i] * k;
        } else {
            const float t = (v[i] - 1.0f) * k + 1.0f;
            out[i] = t == 0.0f ? 1e-07f : t;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct Layout {
    Segs sg;
    int64_t total, groups, members;  // N, G, R
    bool inner_reduced;
};

// 0: fine; SONAR_ERR_*: refused (the text is set)
int layout_of(const char* who, int nseg, int first_reduced, const int64_t (&sizes)[kMaxSegs], Layout* lay) {
    SONAR_REQUIRE(nseg >= 1 && nseg <= kMaxSegs, SONAR_ERR_ARG, "%s: %d segments (1 to %d)", who, nseg, kMaxSegs);
    int64_t total = 1, groups = 1, members = 1;
    for (int k = 0; k < nseg; ++k) {
        SONAR_REQUIRE(sizes[k] >= 0, SONAR_ERR_ARG, "%s: segment %d has size %lld", who, k, (long long)sizes[k]);
        SONAR_REQUIRE(sizes[k] <= INT32_MAX && total * sizes[k] <= INT32_MAX, SONAR_ERR_UNSUPPORTED, "%s: tensors of 2^31 elements or more",
                      who);
        total *= sizes[k];
        const bool reduced = ((k & 1) != 0) != (first_reduced != 0);
        (reduced ? members : groups) *= sizes[k];
    }
    lay->sg = Segs{};
    lay->sg.nseg = nseg;
    lay->sg.first_reduced = first_reduced != 0;
    lay->total = total;
    lay->groups = groups;
    lay->members = members;
    lay->inner_reduced = ((nseg - 1) & 1) != (first_reduced != 0);
    if (total == 0) return 0;  // nothing will be launched
    uint32_t stride = 1, gstride = 1;
    for (int k = nseg - 1; k >= 0; --k) {
        const uint32_t d = (uint32_t)sizes[k];
        const bool reduced = ((k & 1) != 0) != (first_reduced != 0);
        uint32_t shift = 0;
        while (shift < 32 && (1ull << shift) < d) ++shift;
        lay->sg.size[k] = d;
        lay->sg.stride[k] = stride;
        lay->sg.gstride[k] = reduced ? 0 : gstride;
        lay->sg.magic[k] = (uint32_t)(((1ull << 32) * ((1ull << shift) - d)) / d + 1);
        lay->sg.shift[k] = shift;
        stride *= d;
        if (!reduced) gstride *= d;
    }
    return 0;
}

// The split rule.  S slices of `chunk` members each, none empty.  Innermost reduced: work items are waves, a slice is worth a wave from
// kRunSlice members on, and slicing stops once kRunItems waves have work.  Innermost kept: work items are workgroups of 256 groups, a slice
// is worth a lane from kLaneSlice members on, and slicing stops once kLaneBlocks workgroups have work.
void split_of(const Layout& lay, uint32_t* S, uint32_t* chunk) {
    const uint64_t R = (uint64_t)lay.members, G = (uint64_t)lay.groups;
    const uint64_t slice = lay.inner_reduced ? kRunSlice : kLaneSlice;
    const uint64_t have = lay.inner_reduced ? G : (G + kBlock - 1) / kBlock, want = lay.inner_reduced ? kRunItems : kLaneBlocks;
    uint64_t s = std::min((R + slice - 1) / slice, (want + have - 1) / have);
    if (s < 1) s = 1;
    const uint64_t c = (R + s - 1) / s;
    *chunk = (uint32_t)c;
    *S = (uint32_t)((R + c - 1) / c);
}

template <bool MS, bool MM, int X = kPlain>
void launch_stats(const Layout& lay, const float* x, float* mean, float* stdv, float* lo, float* hi, double* ws, hipStream_t st) {
    uint32_t S, chunk;
    split_of(lay, &S, &chunk);
    const uint32_t G = (uint32_t)lay.groups, R = (uint32_t)lay.members;
    if (lay.inner_reduced) {
        hipLaunchKernelGGL((group_stats_runs_kernel<MS, MM, X>), dim3(grid_for((int64_t)G * S, kBlock / 64)), dim3(kBlock), 0, st, x, lay.sg, G, R, S,
                           chunk, mean, stdv, lo, hi, ws);
    } else {
        hipLaunchKernelGGL((group_stats_lanes_kernel<MS, MM, X>), dim3(grid_for((int64_t)((G + kBlock - 1) / kBlock) * S, 1)), dim3(kBlock), 0, st, x,
                           lay.sg, G, R, S, chunk, mean, stdv, lo, hi, ws);
    }
    if (S > 1)
        hipLaunchKernelGGL((group_stats_combine_kernel<MS, MM, X>), dim3(grid_for(G, kBlock)), dim3(kBlock), 0, st, ws, G, R, S, mean, stdv, lo, hi);
}

int64_t ws_doubles(const Layout& lay, bool ms, bool mm) {
    if (lay.total == 0) return 0;
    uint32_t S, chunk;
    split_of(lay, &S, &chunk);
    return S > 1 ? (int64_t)S * lay.groups * ((ms ? 2 : 0) + (mm ? 2 : 0)) : 0;
}

}  // namespace
}  // namespace sonar

using namespace sonar;

extern "C" int64_t sonar_group_stats_ws_doubles(int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                                int64_t s5, int want_mean_std, int want_min_max) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_stats_ws_doubles", nseg, first_reduced, sizes, &lay);
    return rc != 0 ? rc : ws_doubles(lay, want_mean_std != 0, want_min_max != 0);
}

extern "C" int sonar_group_stats_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                     int64_t s5, float* mean, float* stdv, float* lo, float* hi, double* ws, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_stats_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    const bool ms = mean || stdv, mm = lo || hi;
    SONAR_REQUIRE((ms || mm) && (!ms || (mean && stdv)) && (!mm || (lo && hi)), SONAR_ERR_ARG,
                  "sonar_group_stats_f32: mean and stdv, lo and hi, or all four");
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x, SONAR_ERR_ARG, "sonar_group_stats_f32: x is NULL");
    SONAR_REQUIRE((const void*)mean != x && (const void*)stdv != x && (const void*)lo != x && (const void*)hi != x && (const void*)ws != x,
                  SONAR_ERR_ARG, "sonar_group_stats_f32: a result written over x");
    SONAR_REQUIRE(ws || ws_doubles(lay, ms, mm) == 0, SONAR_ERR_ARG, "sonar_group_stats_f32: this shape is split and needs the workspace");
    const hipStream_t st = (hipStream_t)stream;
    if (ms && mm) launch_stats<true, true>(lay, x, mean, stdv, lo, hi, ws, st);
    else if (ms) launch_stats<true, false>(lay, x, mean, stdv, lo, hi, ws, st);
    else launch_stats<false, true>(lay, x, mean, stdv, lo, hi, ws, st);
    return check_launch("sonar_group_stats_f32");
}

extern "C" int sonar_group_affine_f32(int op, const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                      int64_t s4, int64_t s5, const float* a, const float* b, float* out, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_affine_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    SONAR_REQUIRE(op == 0 || op == 1, SONAR_ERR_ARG, "sonar_group_affine_f32: op %d", op);
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x && out && (a || b), SONAR_ERR_ARG, "sonar_group_affine_f32: bad argument");
    SONAR_REQUIRE((const void*)a != out && (const void*)b != out, SONAR_ERR_ARG, "sonar_group_affine_f32: out over an operand table");
    hipLaunchKernelGGL(group_affine_kernel, dim3(grid_for(lay.total, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, op, x, lay.sg,
                       (uint32_t)lay.total, a, b, out);
    return check_launch("sonar_group_affine_f32");
}

extern "C" int sonar_group_minmax_rescale_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                              int64_t s4, int64_t s5, const float* lo, const float* hi, float eps, double target_min,
                                              double target_max, float* out, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_minmax_rescale_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x && lo && hi && out, SONAR_ERR_ARG, "sonar_group_minmax_rescale_f32: bad argument");
    SONAR_REQUIRE((const void*)lo != out && (const void*)hi != out, SONAR_ERR_ARG, "sonar_group_minmax_rescale_f32: out over lo / hi");
    hipLaunchKernelGGL(group_minmax_rescale_kernel, dim3(grid_for(lay.total, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, lay.sg,
                       (uint32_t)lay.total, lo, hi, eps, (float)target_min, (float)target_max, (float)(target_max - target_min), out);
    return check_launch("sonar_group_minmax_rescale_f32");
}

extern "C" int sonar_group_adjust_f32(int op, const float* v, int64_t n, float k, float* out, void* stream) {
    SONAR_REQUIRE((op == 0 || op == 1) && n >= 0, SONAR_ERR_ARG, "sonar_group_adjust_f32: bad argument");
    if (n == 0) return SONAR_OK;
    SONAR_REQUIRE(v && out, SONAR_ERR_ARG, "sonar_group_adjust_f32: bad argument");
    hipLaunchKernelGGL(group_adjust_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, op, v, n, k, out);
    return check_launch("sonar_group_adjust_f32");
}

// ---- PowerLawNoiseGenerator's div_max_dims and scale_noise's normalize_dims over any dims ----------------------------------------------
// ws of the two reductions: what sonar_group_stats_ws_doubles names for one pair (they keep one plane of its two)
extern "C" int sonar_group_peak_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                    int64_t s5, int use_abs, float* peak, double* ws, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_peak_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x && peak && (const void*)peak != x && (const void*)ws != x, SONAR_ERR_ARG, "sonar_group_peak_f32: bad argument");
    SONAR_REQUIRE(ws || ws_doubles(lay, false, true) == 0, SONAR_ERR_ARG, "sonar_group_peak_f32: this shape is split and needs the workspace");
    const hipStream_t st = (hipStream_t)stream;
    if (use_abs) launch_stats<false, false, kPeakAbs>(lay, x, nullptr, nullptr, nullptr, peak, ws, st);
    else launch_stats<false, false, kPeak>(lay, x, nullptr, nullptr, nullptr, peak, ws, st);
    return check_launch("sonar_group_peak_f32");
}

extern "C" int sonar_group_div_f32(float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                   int64_t s5, const float* d, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_div_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x && d && (const void*)d != x, SONAR_ERR_ARG, "sonar_group_div_f32: bad argument");
    hipLaunchKernelGGL(group_div_kernel, dim3(grid_for(lay.total, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, lay.sg,
                       (uint32_t)lay.total, d);
    return check_launch("sonar_group_div_f32");
}

extern "C" int sonar_group_divided_mean_f32(const float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                            int64_t s4, int64_t s5, const float* d, float* mean, double* ws, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_divided_mean_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x && d && mean && mean != d && (const void*)mean != x && (const void*)ws != x, SONAR_ERR_ARG,
                  "sonar_group_divided_mean_f32: bad argument");
    SONAR_REQUIRE(ws || ws_doubles(lay, true, false) == 0, SONAR_ERR_ARG,
                  "sonar_group_divided_mean_f32: this shape is split and needs the workspace");
    launch_stats<true, false, kDivMean>(lay, x, mean, const_cast<float*>(d), nullptr, nullptr, ws, (hipStream_t)stream);
    return check_launch("sonar_group_divided_mean_f32");
}

extern "C" int sonar_group_scale_noise_f32(float* x, int nseg, int first_reduced, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                           int64_t s5, const float* sd, const float* mean, float factor, void* stream) {
    const int64_t sizes[kMaxSegs] = {s0, s1, s2, s3, s4, s5};
    Layout lay;
    const int rc = layout_of("sonar_group_scale_noise_f32", nseg, first_reduced, sizes, &lay);
    if (rc != 0) return rc;
    if (lay.total == 0) return SONAR_OK;
    SONAR_REQUIRE(x && sd && mean && (const void*)sd != x && (const void*)mean != x, SONAR_ERR_ARG, "sonar_group_scale_noise_f32: bad argument");
    hipLaunchKernelGGL(group_scale_noise_kernel, dim3(grid_for(lay.total, kBlock * 2)), dim3(kBlock), 0, (hipStream_t)stream, x, lay.sg,
                       (uint32_t)lay.total, sd, mean, factor);
    return check_launch("sonar_group_scale_noise_f32");
}
