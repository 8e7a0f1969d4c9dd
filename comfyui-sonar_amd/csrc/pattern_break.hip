// PatternBreakNoise (utils.pattern_break, py/utils.py:575-596): the tensor rescaled to [-1, 1] between its own extremes, a chaotic map of
// the values (|v| * 1e6 mod 11 -> erfinv), optionally rescaled to the input's extremes, blended with the input.  Every step up to and
// including the map is one correctly rounded fp32 operation (or exact: min, max, fmod), written here in the reference's order, so the
// argument of erfinv equals the reference's bit for bit; what follows is smooth ("Pattern-break").
//
// Two routes with bit-equal outputs (one device function per step; min and max exact in any order, folded by block_minmax of
// range_reduce.h: a NaN never wins, as in sonar_minmax_rows_f32):
//   three launches  pb_range_kernel          (lo, hi) of x, one pair of partials per block
//                   pb_result_range_kernel   folds those, (lo, hi) of pb_result(x), one pair per block -- only with restore_scale
//                   pb_apply_kernel          folds both sets, recomputes pb_result, rescales, blends, stores, (sum, sumsq) of the output
//   one launch      pb_one_kernel            one workgroup of 1024 runs the three phases over the whole tensor, LDS reductions between
// Nothing is read on the host.  The result is recomputed in the last launch instead of being stored by the second: 16 bytes of traffic per
// element against 24.
#include "common.h"
#include "range_reduce.h"

namespace sonar {

namespace {

constexpr int kPbMaxPart = SONAR_PATTERN_BREAK_NPART;
constexpr int kPbOneBlock = 1024;
// the one-launch route up to this many elements: where the two routes' times cross (profiles/pattern_break_time.txt)
constexpr int64_t kPbOneLaunchMax = SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX;
static_assert(SONAR_PATTERN_BREAK_WS == 4 * kPbMaxPart, "two sets of (lo, hi) pairs");
static_assert(kPbMaxPart <= kNPart, "the apply launch owns one (sum, sumsq) slot per block");

// scalar elements [0, head) and [head + 4 nv, n), 16-byte groups between them
struct PbLayout {
    int64_t head, nv, n;
};

template <typename F4, typename F1>
__device__ __forceinline__ void pb_visit(const PbLayout& L, int64_t tid, int64_t nthreads, F4&& f4, F1&& f1) {
    for (int64_t i = tid; i < L.nv; i += nthreads) f4(L.head + 4 * i);
    const int64_t tail = L.head + 4 * L.nv;
    const int64_t nscalar = L.head + (L.n - tail);
    for (int64_t j = tid; j < nscalar; j += nthreads) f1(j < L.head ? j : tail + (j - L.head));
}

// fmodf(m, 11) for m >= 0: the rounded quotient's floor is the true one or one above it, the fused step is exact (the remainder is a
// multiple of m's last place and below 22 in magnitude), and so is the correction
__device__ __forceinline__ float pb_remainder11(float m) {
    const float q = floorf(m / 11.0f);
    float r = __builtin_fmaf(-q, 11.0f, m);
    if (r < 0.0f) r = __fadd_rn(r, 11.0f);
    else if (r >= 11.0f) r = __fsub_rn(r, 11.0f);
    return r;
}

// the filtered value before restore_scale and the blend (py/utils.py:587-593).  The scalars are Python floats in the reference: formed in
// double and rounded to fp32 once (detail_scale = 1 + detail_level / 10 by the caller), each multiply rounded on its own in its order.
__device__ __forceinline__ float pb_result(float x, float lo, float hi, float detail_scale) {
    const float v = minmax_rescale_value(x, lo, hi, 1e-7f, -1.0f, 1.0f, 2.0f);
    const float m = __fmul_rn(fabsf(v), 1000000.0f);
    const float r = pb_remainder11(m) / 11.0f;
    const float a = __fsub_rn(__fmul_rn(2.0f, r), 1.0f);
    // r == 0 (one element in ~400) is a == -1: the infinity reaches the clamp
    const float e = a <= -1.0f ? -INFINITY : (a >= 1.0f ? INFINITY : erfinvf(a));
    const float y = __fmul_rn(__fmul_rn(__fmul_rn(detail_scale, e), (float)1.4142135623730951), (float)0.2);
    return y != y ? y : fminf(fmaxf(y, -1.0f), 1.0f);  // clamp_ keeps NaN
}

struct PbRange {
    float lo = INFINITY, hi = -INFINITY;
    __device__ __forceinline__ void take(float v) {
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
};

__device__ __forceinline__ PbRange pb_range_of(const float* __restrict__ x, const PbLayout& L, int64_t tid, int64_t nthreads) {
    PbRange r;
    pb_visit(L, tid, nthreads,
             [&](int64_t i) {
                 const float4 v = *reinterpret_cast<const float4*>(x + i);
                 r.take(v.x); r.take(v.y); r.take(v.z); r.take(v.w);
             },
             [&](int64_t i) { r.take(x[i]); });
    return r;
}

__device__ __forceinline__ PbRange pb_result_range_of(const float* __restrict__ x, const PbLayout& L, int64_t tid, int64_t nthreads, float lo,
                                                      float hi, float detail_scale) {
    PbRange r;
    pb_visit(L, tid, nthreads,
             [&](int64_t i) {
                 const float4 v = *reinterpret_cast<const float4*>(x + i);
                 r.take(pb_result(v.x, lo, hi, detail_scale)); r.take(pb_result(v.y, lo, hi, detail_scale));
                 r.take(pb_result(v.z, lo, hi, detail_scale)); r.take(pb_result(v.w, lo, hi, detail_scale));
             },
             [&](int64_t i) { r.take(pb_result(x[i], lo, hi, detail_scale)); });
    return r;
}

struct PbApply {
    float lo, hi, rlo, rhi, span, detail_scale, percentage;
    int mode;
    // restore_scale is normalize_to_scale(result, orig_min, orig_max): the targets went through .item(), their difference is a double's
    template <bool RESTORE>
    __device__ __forceinline__ float value(float x) const {
        float y = pb_result(x, lo, hi, detail_scale);
        if (RESTORE) y = minmax_rescale_value(y, rlo, rhi, 1e-7f, lo, hi, span);
        return blend<float>(mode, x, y, percentage);
    }
};

// the last phase; (s, q): this thread's share of the output's (sum, sumsq)
template <bool RESTORE>
__device__ __forceinline__ void pb_apply_to(const float* __restrict__ x, float* __restrict__ out, const PbLayout& L, int64_t tid,
                                            int64_t nthreads, const PbApply& A, double& s, double& q) {
    pb_visit(L, tid, nthreads,
             [&](int64_t i) {
                 const float4 v = *reinterpret_cast<const float4*>(x + i);
                 float4 o;
                 o.x = A.value<RESTORE>(v.x); o.y = A.value<RESTORE>(v.y); o.z = A.value<RESTORE>(v.z); o.w = A.value<RESTORE>(v.w);
                 *reinterpret_cast<float4*>(out + i) = o;
                 const double a = o.x, b = o.y, c = o.z, d = o.w;
                 s += a; q += a * a; s += b; q += b * b; s += c; q += c * c; s += d; q += d * d;
             },
             [&](int64_t i) {
                 const float o = A.value<RESTORE>(x[i]);
                 out[i] = o;
                 s += (double)o; q += (double)o * (double)o;
             });
}

__device__ __forceinline__ float pb_span(float lo, float hi) { return (float)((double)hi - (double)lo); }

__global__ void __launch_bounds__(kBlock) pb_range_kernel(const float* __restrict__ x, PbLayout L, float* __restrict__ part) {
    kernarg_touch_for(x, L, part);
    __shared__ float sm[2 * kBlock / 64];
    const PbRange r = pb_range_of(x, L, (int64_t)blockIdx.x * kBlock + threadIdx.x, (int64_t)gridDim.x * kBlock);
    float lo[1] = {r.lo}, hi[1] = {r.hi};
    block_minmax<kBlock, 1>(lo, hi, sm);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = lo[0];
        part[2 * blockIdx.x + 1] = hi[0];
    }
}

__global__ void __launch_bounds__(kBlock) pb_result_range_kernel(const float* __restrict__ x, PbLayout L, const float* __restrict__ xpart,
                                                                 int npart, float detail_scale, float* __restrict__ rpart) {
    kernarg_touch_for(x, L, xpart, npart, detail_scale, rpart);
    __shared__ float sm[2 * kBlock / 64];
    float lo[1] = {INFINITY}, hi[1] = {-INFINITY};
    for (int i = threadIdx.x; i < npart; i += kBlock) {
        lo[0] = fminf(lo[0], xpart[2 * i]);
        hi[0] = fmaxf(hi[0], xpart[2 * i + 1]);
    }
    block_minmax<kBlock, 1>(lo, hi, sm);
    const PbRange r = pb_result_range_of(x, L, (int64_t)blockIdx.x * kBlock + threadIdx.x, (int64_t)gridDim.x * kBlock, lo[0], hi[0], detail_scale);
    float rlo[1] = {r.lo}, rhi[1] = {r.hi};
    block_minmax<kBlock, 1>(rlo, rhi, sm);
    if (threadIdx.x == 0) {
        rpart[2 * blockIdx.x] = rlo[0];
        rpart[2 * blockIdx.x + 1] = rhi[0];
    }
}

template <bool RESTORE>
__global__ void __launch_bounds__(kBlock) pb_apply_kernel(const float* __restrict__ x, float* __restrict__ out, PbLayout L,
                                                          const float* __restrict__ xpart, const float* __restrict__ rpart, int npart,
                                                          int nrpart, float detail_scale, float percentage, int mode, double* stats) {
    kernarg_touch_for(x, out, L, xpart, rpart, npart, nrpart, detail_scale, percentage, mode, stats);
    __shared__ float sm[4 * kBlock / 64];
    __shared__ double red[2 * kBlock / 64];
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < npart; i += kBlock) {
        lo[0] = fminf(lo[0], xpart[2 * i]);
        hi[0] = fmaxf(hi[0], xpart[2 * i + 1]);
    }
    if (RESTORE)
        for (int i = threadIdx.x; i < nrpart; i += kBlock) {
            lo[1] = fminf(lo[1], rpart[2 * i]);
            hi[1] = fmaxf(hi[1], rpart[2 * i + 1]);
        }
    block_minmax<kBlock, 2>(lo, hi, sm);
    const PbApply A{lo[0], hi[0], lo[1], hi[1], pb_span(lo[0], hi[0]), detail_scale, percentage, mode};
    double s = 0.0, q = 0.0;
    pb_apply_to<RESTORE>(x, out, L, (int64_t)blockIdx.x * kBlock + threadIdx.x, (int64_t)gridDim.x * kBlock, A, s, q);
    if (stats != nullptr) write_partial<kBlock>(s, q, stats, red);
}

template <bool RESTORE>
__global__ void __launch_bounds__(kPbOneBlock) pb_one_kernel(const float* __restrict__ x, float* __restrict__ out, PbLayout L, float detail_scale,
                                                             float percentage, int mode, double* stats) {
    kernarg_touch_for(x, out, L, detail_scale, percentage, mode, stats);
    __shared__ float sm[2 * kPbOneBlock / 64];
    __shared__ double red[2 * kPbOneBlock / 64];
    const int64_t tid = threadIdx.x;
    const PbRange r = pb_range_of(x, L, tid, kPbOneBlock);
    float lo[1] = {r.lo}, hi[1] = {r.hi};
    block_minmax<kPbOneBlock, 1>(lo, hi, sm);
    float rlo[1] = {0.0f}, rhi[1] = {0.0f};
    if (RESTORE) {
        const PbRange rr = pb_result_range_of(x, L, tid, kPbOneBlock, lo[0], hi[0], detail_scale);
        rlo[0] = rr.lo;
        rhi[0] = rr.hi;
        block_minmax<kPbOneBlock, 1>(rlo, rhi, sm);
    }
    const PbApply A{lo[0], hi[0], rlo[0], rhi[0], pb_span(lo[0], hi[0]), detail_scale, percentage, mode};
    double s = 0.0, q = 0.0;
    pb_apply_to<RESTORE>(x, out, L, tid, kPbOneBlock, A, s, q);
    if (stats != nullptr) write_partial_at<kPbOneBlock>(s, q, stats, red, 0, 1);
}

}  // namespace

}  // namespace sonar

extern "C" int sonar_pattern_break_route(int64_t n) { return n <= sonar::kPbOneLaunchMax ? SONAR_PATTERN_BREAK_ONE : SONAR_PATTERN_BREAK_THREE; }

extern "C" int sonar_pattern_break_f32(const float* x, float* out, int64_t n, float detail_scale, float percentage, int blend_mode,
                                       int restore_scale, int route, float* ws, int64_t ws_floats, double* stats, void* stream) {
    using namespace sonar;
    const char* const who = "sonar_pattern_break_f32";
    SONAR_REQUIRE(x != nullptr && out != nullptr && ws != nullptr, SONAR_ERR_ARG, "%s: NULL tensor or workspace", who);
    SONAR_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)ws) & 3) == 0 && ((uintptr_t)stats & 7) == 0, SONAR_ERR_ARG,
                  "%s: a pointer is not aligned to its element", who);
    SONAR_REQUIRE(out != x && (const float*)ws != x && ws != out, SONAR_ERR_ARG, "%s: out and the workspace must not be x or each other", who);
    SONAR_REQUIRE(n > 0, SONAR_ERR_ARG, "%s: n = %lld", who, (long long)n);
    SONAR_REQUIRE(blend_mode == SONAR_BLEND_LERP || blend_mode == SONAR_BLEND_INJECT || blend_mode == SONAR_BLEND_SUBTRACT_B, SONAR_ERR_ARG,
                  "%s: unknown blend mode %d", who, blend_mode);
    SONAR_REQUIRE(route == SONAR_PATTERN_BREAK_AUTO || route == SONAR_PATTERN_BREAK_ONE || route == SONAR_PATTERN_BREAK_THREE, SONAR_ERR_ARG,
                  "%s: unknown route %d", who, route);
    SONAR_REQUIRE(ws_floats >= SONAR_PATTERN_BREAK_WS, SONAR_ERR_ARG, "%s: a workspace of %lld floats, SONAR_PATTERN_BREAK_WS = %d are needed", who,
                  (long long)ws_floats, SONAR_PATTERN_BREAK_WS);
    // 16-byte groups where x and out reach a 16-byte boundary together; every element through the scalar loop otherwise
    PbLayout L{n, 0, n};
    if ((((uintptr_t)x ^ (uintptr_t)out) & 15) == 0) {
        const int64_t head = (int64_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;
        if (head < n) L = PbLayout{head, (n - head) / 4, n};
    }
    const hipStream_t st = (hipStream_t)stream;
    if (route == SONAR_PATTERN_BREAK_AUTO) route = sonar_pattern_break_route(n);
    if (route == SONAR_PATTERN_BREAK_ONE) {
        if (restore_scale)
            hipLaunchKernelGGL(pb_one_kernel<true>, dim3(1), dim3(kPbOneBlock), 0, st, x, out, L, detail_scale, percentage, blend_mode, stats);
        else
            hipLaunchKernelGGL(pb_one_kernel<false>, dim3(1), dim3(kPbOneBlock), 0, st, x, out, L, detail_scale, percentage, blend_mode, stats);
        return check_launch(who);
    }
    int64_t blocks = (n + kBlock * 8 - 1) / (kBlock * 8);
    const int grid = (int)(blocks < kPbMaxPart ? blocks : kPbMaxPart);
    float* const xpart = ws;
    float* const rpart = ws + 2 * kPbMaxPart;
    hipLaunchKernelGGL(pb_range_kernel, dim3(grid), dim3(kBlock), 0, st, x, L, xpart);
    if (restore_scale) {
        hipLaunchKernelGGL(pb_result_range_kernel, dim3(grid), dim3(kBlock), 0, st, x, L, (const float*)xpart, grid, detail_scale, rpart);
        hipLaunchKernelGGL(pb_apply_kernel<true>, dim3(grid), dim3(kBlock), 0, st, x, out, L, (const float*)xpart, (const float*)rpart, grid, grid,
                           detail_scale, percentage, blend_mode, stats);
    } else {
        hipLaunchKernelGGL(pb_apply_kernel<false>, dim3(grid), dim3(kBlock), 0, st, x, out, L, (const float*)xpart, (const float*)rpart, grid, 0,
                           detail_scale, percentage, blend_mode, stats);
    }
    return check_launch(who);
}
