// Wave- and block-wide reductions of extremes, of the "a NaN was seen" flag and of any other associative, commutative op: the one home of
// the shuffle butterfly and of the per-wave LDS staging (the (sum, sumsq) pairs have theirs in common.h: wave_sum, block_sum2).
//
// Two NaN rules, one per site:
//   a NaN never wins   fold with fminf / fmaxf alone: they return the other operand, so the extremes are those of the remaining values
//                      (+inf / -inf when there are none).  sonar_minmax_rows_f32 and everything built on normalize_to_scale.
//   a NaN poisons      torch.amax / torch.max: the same fold with `nan |= v != v` kept beside it, the flag reduced with the values and
//                      nan_poisons(flag, v) at the end.
// Plain shuffles on purpose: no kernel here is bound by its reduction, and common.h's dpp_move feeds zeros into the rows a DPP control
// masks (old = 0, bound_ctrl) -- nothing to a sum, a wrong answer to an extreme.
#pragma once
#include "common.h"

namespace sonar {

// xor butterfly: the result in every lane
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ float wave_min(float v) { return wave_reduce(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max(float v) { return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ int wave_or(int v) { return wave_reduce(v, [](int a, int b) { return a | b; }); }

__device__ __forceinline__ float nan_poisons(bool nan, float v) { return nan ? NAN : v; }

// N values per thread, value k folded with op(k, a, b), over the THREADS threads of the workgroup; the totals in every thread, waves
// joined in ascending order.  `red`: N * THREADS / 64 elements of LDS.  Every thread must call.  The closing barrier is the one that
// protects `red`: on return nobody reads it any more, so the next call -- or any other use of that memory -- may follow at once.
template <int THREADS, int N, typename T, typename Op>
__device__ __forceinline__ void block_reduce(T (&v)[N], Op op, T* red) {
    constexpr int NW = THREADS / kWave;
    constexpr int kJoinUnroll = NW <= 4 ? NW : 2;  // 16 waves unrolled cost quantile_rows_kernel<1024, .> an occupancy step and scratch
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        v[k] = wave_reduce(v[k], [&](T a, T b) { return op(k, a, b); });
        if (lane == 0) red[k * NW + wid] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        T r = red[k * NW];
#pragma unroll kJoinUnroll
        for (int w = 1; w < NW; ++w) r = op(k, r, red[k * NW + w]);
        v[k] = r;
    }
    __syncthreads();
}
template <int THREADS, typename T, typename Op>  // one value, op(a, b)
__device__ __forceinline__ T block_reduce(T v, Op op, T* red) {
    T one[1] = {v};
    block_reduce<THREADS>(one, [&](int, T a, T b) { return op(a, b); }, red);
    return one[0];
}

// K (lo, hi) pairs, a NaN never wins.  `red`: 2 K THREADS / 64 floats
template <int THREADS, int K>
__device__ __forceinline__ void block_minmax(float (&lo)[K], float (&hi)[K], float* red) {
    float v[2 * K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[2 * k] = lo[k], v[2 * k + 1] = hi[k];
    block_reduce<THREADS>(v, [](int k, float a, float b) { return k & 1 ? fmaxf(a, b) : fminf(a, b); }, red);
#pragma unroll
    for (int k = 0; k < K; ++k) lo[k] = v[2 * k], hi[k] = v[2 * k + 1];
}
template <int THREADS>
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* red) {
    float l[1] = {lo}, h[1] = {hi};
    block_minmax<THREADS, 1>(l, h, red);
    lo = l[0], hi = h[0];
}

// (lo, hi) and the poison flag, which rides as one more value: 0 / 1 under fmaxf is the OR.  `red`: 3 THREADS / 64 floats
template <int THREADS>
__device__ __forceinline__ void block_minmax_nan(float& lo, float& hi, int& nan, float* red) {
    float v[3] = {lo, hi, nan ? 1.0f : 0.0f};
    block_reduce<THREADS>(v, [](int k, float a, float b) { return k == 0 ? fminf(a, b) : fmaxf(a, b); }, red);
    lo = v[0], hi = v[1], nan = v[2] != 0.0f;
}
// torch.amax / torch.max of the workgroup's values: the maximum, NaN if any thread's flag is set.  `red`: 2 THREADS / 64 floats
template <int THREADS>
__device__ __forceinline__ float block_max_poisoned(float hi, int nan, float* red) {
    float v[2] = {hi, nan ? 1.0f : 0.0f};
    block_reduce<THREADS>(v, [](int, float a, float b) { return fmaxf(a, b); }, red);
    return nan_poisons(v[1] != 0.0f, v[0]);
}

}  // namespace sonar
