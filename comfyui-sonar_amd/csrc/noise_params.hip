// SonarCustomNoiseParameters (py/noise.py:2080-2187): everything the item does to the inner sampler's tensor, two launches and no host
// synchronisation.  The tensor is `planes` planes of `plane_in` values of which the first `plane_out` of each are kept (the square plane
// of ensure_square_aspect_ratio cropped back; plane_in == plane_out without it: the entry points then see one plane of n values).
//   scan:   one sweep over the generated tensor -> one slot of six 64-bit partials per block: the finite extremes over ALL values (the
//           padding of a squared plane included: fix_invalid runs before the crop; two floats in one word); over the KEPT values the sum
//           and sum of squares of the finite ones and the counts of +inf, -inf and NaN.
//   apply:  every block reduces the slots (scale_noise_kernel's decide_norm, with more columns), from which the replacement values
//           posval = max(largest finite, 0), negval = min(smallest finite, 0) (nan_to_num's extremes are taken AFTER the non-finite values
//           became 0) and the statistics of the fixed, cropped tensor follow without a second read: sum += n+ posval + n- negval, sumsq
//           += n+ posval^2 + n- negval^2.  Then per kept value: fix -> the two thresholded corrections (py/utils.py:100-105; the mean is
//           subtracted as two floats) -> * factor -> one rounding into the output dtype, written at p * plane_out + i.
// Source and output are fp32, fp16 or bf16 each; arithmetic is fp32, sums fp64 (sonar_stats_f32's form: for a mean-300 / std-1 tensor of
// 2^20 values the cancellation in sumsq - sum * mean leaves the variance good to 1e-8).  HBM-bound: two reads of the source and one write.  A
// work unit is one tile of kBlock * V values of ONE plane (so a lane never divides: the unit's plane is one uniform division per tile);
// V = 4 -- one 16-byte access of fp32, 8 bytes of a half type -- when both plane lengths are multiples of 4 and the buffers are 16-byte
// aligned (every plane then starts aligned and a vector is wholly kept or wholly padding), V = 1 otherwise, chosen per launch.  Tiles
// that lie wholly inside the kept part run unguarded, two at a time; a plane's last tile checks its lanes.
#include <math.h>

#include <algorithm>

#include "dtype_io.h"
#include "ew_driver.h"  // aligned16
#include "range_reduce.h"

namespace sonar {
namespace {

constexpr int kSlot = SONAR_NOISE_PARAMS_SLOT;
enum { S_SUM, S_SQ, S_POS, S_NEG, S_NAN, S_EXT };  // S_EXT: the finite maximum and minimum as two floats in one 64-bit word
constexpr int kSums = S_EXT;
static_assert(S_EXT + 1 == kSlot, "a slot holds the five sums and the pair of extremes");

__device__ __forceinline__ double pack_ext(float mx, float mn) {
    return __longlong_as_double((long long)(((uint64_t)__float_as_uint(mx) << 32) | (uint64_t)__float_as_uint(mn)));
}
__device__ __forceinline__ void unpack_ext(double w, float& mx, float& mn) {
    const uint64_t b = (uint64_t)__double_as_longlong(w);
    mx = __uint_as_float((uint32_t)(b >> 32));
    mn = __uint_as_float((uint32_t)b);
}

__device__ __forceinline__ bool finite_f(float y) { return fabsf(y) < INFINITY; }  // false for NaN

// what one thread has seen
struct Seen {
    double s = 0.0, q = 0.0;
    uint32_t npos = 0, nneg = 0, nnan = 0;
    float mx = -INFINITY, mn = INFINITY;
    // FIX: the finite / non-finite split; otherwise plain (sum, sumsq) of the kept values, whatever they are (scale_noise's statistics)
    template <bool FIX>
    __device__ __forceinline__ void add(float y, bool kept) {
        if constexpr (FIX) {
            const bool fin = finite_f(y);
            mx = fmaxf(mx, fin ? y : -INFINITY);
            mn = fminf(mn, fin ? y : INFINITY);
            const double d = fin && kept ? (double)y : 0.0;
            s += d;
            q += d * d;
            const bool bad = !fin && kept;
            nnan += bad && y != y ? 1u : 0u;
            npos += bad && y > 0.0f ? 1u : 0u;
            nneg += bad && y < 0.0f ? 1u : 0u;
        } else {
            const double d = kept ? (double)y : 0.0;
            s += d;
            q += d * d;
        }
    }
};

// the five sums and the extremes of a block, folded over its threads; valid in thread 0.  `red`: kSlot * kBlock / 64 doubles
__device__ __forceinline__ void block_fold(double (&sum)[kSums], float& mx, float& mn, double* red) {
    constexpr int NW = kBlock / 64;
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = wave_sum(sum[k]);
    mx = wave_max(mx);  // over the finite values only (Seen::add): no NaN reaches these folds
    mn = wave_min(mn);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) red[k * NW + wid] = sum[k];
        red[S_EXT * NW + wid] = pack_ext(mx, mn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) {
            double a = red[k * NW];
#pragma unroll
            for (int w = 1; w < NW; ++w) a += red[k * NW + w];
            sum[k] = a;
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            float a, b;
            unpack_ext(red[S_EXT * NW + w], a, b);
            mx = fmaxf(mx, a);
            mn = fminf(mn, b);
        }
    }
}

// units = planes * chunks tiles of kBlock * V source values; grid <= SONAR_NOISE_PARAMS_NPART, block b owns slot b
template <int V, typename T, bool FIX>
__global__ void __launch_bounds__(kBlock) noise_params_scan_kernel(const T* __restrict__ src, int64_t plane_in, int64_t plane_out, uint32_t chunks,
                                                                   uint32_t units, double* __restrict__ partials) {
    kernarg_touch_for(src, plane_in, plane_out, chunks, units, partials);
    __shared__ double red[kSlot * kBlock / 64];
    constexpr int64_t kTile = (int64_t)kBlock * V;
    // without FIX the padding is of no interest: a plane ends at plane_out
    const int64_t extent = FIX ? plane_in : plane_out;
    Seen seen;
    const uint32_t step = gridDim.x;
    auto whole = [&](uint32_t u, int64_t& at) {  // the tile lies inside the kept part of its plane: no lane checks
        const uint32_t p = u / chunks, c = u - p * chunks;
        at = (int64_t)p * plane_in + (int64_t)c * kTile + (int64_t)threadIdx.x * V;
        return ((int64_t)c + 1) * kTile <= plane_out;
    };
    auto guarded = [&](uint32_t u) {
        const uint32_t p = u / chunks, c = u - p * chunks;
        const int64_t i = (int64_t)c * kTile + (int64_t)threadIdx.x * V;
        if (i < extent) {  // V == 4: both plane lengths are multiples of 4, the vector is inside, and wholly kept or wholly padding
            const Pack<V> a = load<V>(src, (int64_t)p * plane_in + i);
#pragma unroll
            for (int k = 0; k < V; ++k) seen.add<FIX>(a.v[k], i < plane_out);
        }
    };
    uint32_t u = blockIdx.x;
    for (; u < units; u += 2 * step) {
        int64_t at0, at1 = 0;
        const bool w0 = whole(u, at0);
        const bool two = u + step < units && u + step > u;
        const bool w1 = two && whole(u + step, at1);
        if (w0 && w1) {  // two independent loads in flight
            const Pack<V> a = load<V>(src, at0), b = load<V>(src, at1);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                seen.add<FIX>(a.v[k], true);
                seen.add<FIX>(b.v[k], true);
            }
            continue;
        }
        if (w0) {
            const Pack<V> a = load<V>(src, at0);
#pragma unroll
            for (int k = 0; k < V; ++k) seen.add<FIX>(a.v[k], true);
        } else {
            guarded(u);
        }
        if (two) {
            if (w1) {
                const Pack<V> b = load<V>(src, at1);
#pragma unroll
                for (int k = 0; k < V; ++k) seen.add<FIX>(b.v[k], true);
            } else {
                guarded(u + step);
            }
        }
    }
    double sum[kSums] = {seen.s, seen.q, (double)seen.npos, (double)seen.nneg, (double)seen.nnan};
    block_fold(sum, seen.mx, seen.mn, red);
    if (threadIdx.x == 0) {
        double* slot = partials + (int64_t)blockIdx.x * kSlot;
#pragma unroll
        for (int k = 0; k < kSums; ++k) slot[k] = sum[k];
        slot[S_EXT] = pack_ext(seen.mx, seen.mn);
    }
}

// what every block of the apply launch derives from the slots
struct TailDecision {
    NormDecision norm;
    float mean_lo;  // mean - (float)mean: subtracted after norm.mean, so that a value next to the mean keeps its relative accuracy
    float posval, negval;
};

// units = planes * chunks tiles of kBlock * V KEPT values
template <int V, typename TS, typename TD>
__global__ void __launch_bounds__(kBlock) noise_params_apply_kernel(const TS* __restrict__ src, TD* __restrict__ out, int64_t plane_in,
                                                                    int64_t plane_out, uint32_t chunks, uint32_t units, int fix, int normalized,
                                                                    float factor, float thr_sd, const double* __restrict__ partials, int npart,
                                                                    int64_t n_total) {
    kernarg_touch_for(src, out, plane_in, plane_out, chunks, units, fix, normalized, factor, thr_sd, partials, npart, n_total);
    __shared__ double red[kSlot * kBlock / 64];
    __shared__ TailDecision sh;
    TailDecision t{NormDecision{0.f, 1.f, 0, 0}, 0.f, 0.f, 0.f};
    if (partials != nullptr) {
        double col[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
        float mx = -INFINITY, mn = INFINITY;
        for (int i = threadIdx.x; i < npart; i += kBlock) {
            const double* slot = partials + (int64_t)i * kSlot;
#pragma unroll
            for (int k = 0; k < kSums; ++k) col[k] += slot[k];
            float a, b;
            unpack_ext(slot[S_EXT], a, b);
            mx = fmaxf(mx, a);
            mn = fminf(mn, b);
        }
        block_fold(col, mx, mn, red);
        if (threadIdx.x == 0) {
            // the extremes nan_to_num_ is handed are those of the tensor whose non-finite values are 0 already
            t.posval = fmaxf(mx, 0.0f);
            t.negval = fminf(mn, 0.0f);
            if (normalized) {
                const double pv = t.posval, nv = t.negval;
                const double s = col[S_SUM] + col[S_POS] * pv + col[S_NEG] * nv;
                const double q = col[S_SQ] + col[S_POS] * (pv * pv) + col[S_NEG] * (nv * nv);
                t.norm = decision_from_totals(s, q, n_total, thr_sd);
                const double lo = s * rcp_f64((double)n_total) - (double)t.norm.mean;  // (the mean as decision_from_totals forms it)
                t.mean_lo = lo == lo && fabs(lo) < 1.0 ? (float)lo : 0.0f;              // a NaN / infinite mean has no low part
            }
            sh = t;
        }
        __syncthreads();
        t = sh;
    }
    const NormDecision d = t.norm;
    const bool do_mul = factor != 1.0f;
    auto f = [&](float y) {
        if (fix && !finite_f(y)) y = y != y ? 0.0f : (y > 0.0f ? t.posval : t.negval);
        // scale_noise's sequence (common.h apply_norm) with the mean as two floats: y - mean is exact for y next to the mean, and what
        // float32 dropped from the mean would otherwise be that result's whole error (3e-8 absolute on a value of 4e-7: four bfloat16 ulps)
        if (d.do_sub) y = (y - d.mean) - t.mean_lo;
        if (d.do_div) y = y / d.stdv;
        if (do_mul) y = y * factor;
        return y;
    };
    constexpr int64_t kTile = (int64_t)kBlock * V;
    const uint32_t step = gridDim.x;
    auto place = [&](uint32_t u, int64_t& from, int64_t& to) {  // true: the whole tile is kept
        const uint32_t p = u / chunks, c = u - p * chunks;
        const int64_t i = (int64_t)c * kTile + (int64_t)threadIdx.x * V;
        from = (int64_t)p * plane_in + i;
        to = (int64_t)p * plane_out + i;
        return ((int64_t)c + 1) * kTile <= plane_out;
    };
    auto one = [&](int64_t from, int64_t to) {
        Pack<V> a = load<V>(src, from);
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] = f(a.v[k]);
        store<V>(out, to, a);
    };
    auto guarded = [&](uint32_t u) {
        const uint32_t p = u / chunks, c = u - p * chunks;
        const int64_t i = (int64_t)c * kTile + (int64_t)threadIdx.x * V;
        if (i < plane_out) one((int64_t)p * plane_in + i, (int64_t)p * plane_out + i);  // V == 4: plane_out is a multiple of 4
    };
    for (uint32_t u = blockIdx.x; u < units; u += 2 * step) {
        int64_t f0, t0, f1 = 0, t1 = 0;
        const bool w0 = place(u, f0, t0);
        const bool two = u + step < units && u + step > u;
        const bool w1 = two && place(u + step, f1, t1);
        if (w0 && w1) {
            Pack<V> a = load<V>(src, f0), b = load<V>(src, f1);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                a.v[k] = f(a.v[k]);
                b.v[k] = f(b.v[k]);
            }
            store<V>(out, t0, a);
            store<V>(out, t1, b);
            continue;
        }
        if (w0) one(f0, t0);
        else guarded(u);
        if (two) {
            if (w1) one(f1, t1);
            else guarded(u + step);
        }
    }
}

// tiles of `extent` values per plane at vector width v; false: more tiles than a 32-bit unit index holds
inline bool tiling(int64_t planes, int64_t extent, int v, uint32_t& chunks, uint32_t& units) {
    const int64_t tile = (int64_t)kBlock * v;
    const int64_t c = (extent + tile - 1) / tile;
    if (c > INT32_MAX || planes > INT32_MAX / c) return false;
    chunks = (uint32_t)c;
    units = (uint32_t)(planes * c);
    return true;
}

struct ScanShape {
    int v;
    uint32_t chunks, units;
    int grid;
};

// the scan launch's shape from what BOTH entry points are told (the apply launch reduces exactly the slots the scan wrote)
inline bool scan_shape(const void* src, int64_t planes, int64_t plane_in, int64_t plane_out, int fix, ScanShape& s) {
    s.v = (plane_in % 4 == 0 && plane_out % 4 == 0 && aligned16(src)) ? 4 : 1;
    if (!tiling(planes, fix ? plane_in : plane_out, s.v, s.chunks, s.units)) return false;
    s.grid = (int)std::min<uint32_t>(s.units, SONAR_NOISE_PARAMS_NPART);
    return true;
}

// one plane of n values when nothing is cropped
inline void flatten_planes(int64_t& planes, int64_t& plane_in, int64_t& plane_out) {
    if (plane_in == plane_out) {
        plane_in = plane_out = planes * plane_in;
        planes = 1;
    }
}

inline bool shape_ok(int64_t planes, int64_t plane_in, int64_t plane_out) {
    return planes >= 0 && plane_out > 0 && plane_out <= plane_in && (planes == 0 || plane_in <= INT64_MAX / planes);
}

template <typename T>
int scan_typed(const void* src, int64_t plane_in, int64_t plane_out, int fix, const ScanShape& s, double* partials, hipStream_t st) {
    const dim3 grid(s.grid), block(kBlock);
#define SONAR_NP_SCAN(V, FIX) \
    hipLaunchKernelGGL((noise_params_scan_kernel<V, T, FIX>), grid, block, 0, st, (const T*)src, plane_in, plane_out, s.chunks, s.units, partials)
    if (s.v == 4) {
        if (fix) SONAR_NP_SCAN(4, true);
        else SONAR_NP_SCAN(4, false);
    } else {
        if (fix) SONAR_NP_SCAN(1, true);
        else SONAR_NP_SCAN(1, false);
    }
#undef SONAR_NP_SCAN
    return check_launch("sonar_noise_params_scan");
}

template <typename TS, typename TD>
int apply_typed(const void* src, void* out, int64_t planes, int64_t plane_in, int64_t plane_out, int fix, int normalized, float factor,
                float thr_sd, const double* partials, int npart, bool vec, hipStream_t st) {
    uint32_t chunks, units;
    SONAR_REQUIRE(tiling(planes, plane_out, vec ? 4 : 1, chunks, units), SONAR_ERR_ARG, "sonar_noise_params_apply: too many tiles");
    const dim3 grid((unsigned)std::min<uint32_t>(units, (uint32_t)kMaxGrid)), block(kBlock);
    const int64_t n_total = planes * plane_out;
    if (vec)
        hipLaunchKernelGGL((noise_params_apply_kernel<4, TS, TD>), grid, block, 0, st, (const TS*)src, (TD*)out, plane_in, plane_out, chunks, units,
                           fix, normalized, factor, thr_sd, partials, npart, n_total);
    else
        hipLaunchKernelGGL((noise_params_apply_kernel<1, TS, TD>), grid, block, 0, st, (const TS*)src, (TD*)out, plane_in, plane_out, chunks, units,
                           fix, normalized, factor, thr_sd, partials, npart, n_total);
    return check_launch("sonar_noise_params_apply");
}

}  // namespace
}  // namespace sonar

using namespace sonar;

extern "C" int64_t sonar_noise_params_ws_doubles(void) { return (int64_t)SONAR_NOISE_PARAMS_NPART * SONAR_NOISE_PARAMS_SLOT; }

extern "C" int sonar_noise_params_scan(int src_dtype, const void* src, int64_t planes, int64_t plane_in, int64_t plane_out, int fix_invalid,
                                       double* partials, void* stream) {
    SONAR_REQUIRE_DTYPE(src_dtype, "sonar_noise_params_scan");
    SONAR_REQUIRE(shape_ok(planes, plane_in, plane_out), SONAR_ERR_ARG, "sonar_noise_params_scan: bad planes / plane_in / plane_out");
    if (planes == 0) return SONAR_OK;
    SONAR_REQUIRE(src && partials, SONAR_ERR_ARG, "sonar_noise_params_scan: null pointer");
    flatten_planes(planes, plane_in, plane_out);
    ScanShape s;
    SONAR_REQUIRE(scan_shape(src, planes, plane_in, plane_out, fix_invalid != 0, s), SONAR_ERR_ARG, "sonar_noise_params_scan: too many tiles");
    const hipStream_t st = (hipStream_t)stream;
    return with_dtype(src_dtype, "sonar_noise_params_scan", [&](auto elem) {
        return scan_typed<typename decltype(elem)::type>(src, plane_in, plane_out, fix_invalid != 0, s, partials, st);
    });
}

extern "C" int sonar_noise_params_apply(int src_dtype, const void* src, int dst_dtype, void* out, int64_t planes, int64_t plane_in,
                                        int64_t plane_out, int fix_invalid, int normalized, float factor, float threshold_std_devs,
                                        const double* partials, void* stream) {
    SONAR_REQUIRE_DTYPE(src_dtype, "sonar_noise_params_apply");
    SONAR_REQUIRE_DTYPE(dst_dtype, "sonar_noise_params_apply");
    SONAR_REQUIRE(shape_ok(planes, plane_in, plane_out), SONAR_ERR_ARG, "sonar_noise_params_apply: bad planes / plane_in / plane_out");
    const int fix = fix_invalid != 0, norm = normalized != 0;
    SONAR_REQUIRE(partials || !(fix || norm), SONAR_ERR_ARG, "sonar_noise_params_apply: fix_invalid / normalized need the scan launch's partials");
    if (planes == 0) return SONAR_OK;
    SONAR_REQUIRE(src && out && src != out, SONAR_ERR_ARG, "sonar_noise_params_apply: null pointer, or out is src");
    flatten_planes(planes, plane_in, plane_out);
    int npart = 0;
    ScanShape s{};
    if (fix || norm) {
        SONAR_REQUIRE(scan_shape(src, planes, plane_in, plane_out, fix, s), SONAR_ERR_ARG, "sonar_noise_params_apply: too many tiles");
        npart = s.grid;
    } else {
        partials = nullptr;
    }
    const bool vec = plane_in % 4 == 0 && plane_out % 4 == 0 && aligned16(src) && aligned16(out);
    const hipStream_t st = (hipStream_t)stream;
    return with_dtype(src_dtype, "sonar_noise_params_apply", [&](auto from) {
        return with_dtype(dst_dtype, "sonar_noise_params_apply", [&](auto to) {
            return apply_typed<typename decltype(from)::type, typename decltype(to)::type>(src, out, planes, plane_in, plane_out, fix, norm, factor,
                                                                                           threshold_std_devs, partials, npart, vec, st);
        });
    });
}
