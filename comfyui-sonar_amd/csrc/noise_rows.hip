// Row-keyed base generators: `rows` independent latents of `inner` elements from ONE launch, every row with its own (seed, stream id)
// and its own normalisation -- what a host loop of batch-1 fills (sonar_philox_normal_f32 / sonar_philox_uniform_f32 with partials, then
// sonar_scale_noise_f32 or the fused fill's final pass) computes row by row, to the bit.
//
// One workgroup of kBlock threads owns a row and plays, one after the other, the g = tile_grid(inner) workgroups the per-call fill would
// launch for `inner` elements: in turn b its wave w is the fill's wave 4 b + w -- the same tiles in the same order, the same per-thread
// (sum, sumsq) in fp64, the same block_sum2 -- and the block's pair lands in LDS slot b instead of partials[b].  The decision is then
// decide_norm's own reduction over those slots (thread t takes slots t, t + 256, ...; the slots no block owns are zeros there and add
// nothing), and the row is corrected by the thread that wrote each value, so no fence is needed between the passes.  A row that needs no
// correction (N(0,1) with factor 1 passes both thresholds 98.7 % of the time) is written once.
#include "noise_stream.h"

namespace sonar {

// beyond this a fill's waves take more than one tile per turn of kNPart blocks: still the same sums, but one workgroup per row is the
// wrong shape for such a latent
constexpr int64_t kRowsMaxInner = (int64_t)kNPart * 4 * kTileElems;

struct RowKeys {
    const uint64_t* seed;    // [rows]
    const uint64_t* stream;  // [rows] added to stream_id, or null
    uint64_t stream_id;
};

// NORM 0: v * factor (skipped for a factor of exactly 1)
//      1: scale_noise_kernel's sequence -- subtract, IEEE quotient, multiply (skipped for 1) -- each step only when its threshold asks
//      2: the fused fills' final pass (stream_fill_norm_kernel, NormFast): subtract, * (1 / std) * factor
template <Dist D, int NORM>
__global__ void __launch_bounds__(kBlock) philox_rows_kernel(float* out, int64_t rows, int64_t inner, RowKeys keys, int nvb, Affine aff,
                                                             float factor, float thr_sd) {
    kernarg_touch_for(out, rows, inner, keys, nvb, aff, factor, thr_sd);
    __shared__ double red[2 * kBlock / 64];
    __shared__ double part[NORM ? 2 * kNPart : 2];
    __shared__ NormDecision sh;
    const uint32_t lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int64_t last = (inner - 1) / kTileElems;
    const int64_t nwaves = (int64_t)nvb * (kBlock / 64);
    const bool mul_now = NORM == 0 && factor != 1.0f;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        float* const o = out + row * inner;
        const bool vec = (reinterpret_cast<uintptr_t>(o) & 15u) == 0;  // (a row of a length that is no multiple of four: every fourth one)
        const uint64_t seed = keys.seed[row];
        const uint64_t stream_id = keys.stream_id + (keys.stream ? keys.stream[row] : 0);
        // ---- the draw, with the fill's statistics (whole groups of four reduced in fp32 first, a ragged tail per element: store_group<true>)
        for (int b = 0; b < nvb; ++b) {
            double s = 0.0, q = 0.0;
            for (int64_t tile = (int64_t)b * (kBlock / 64) + w; tile <= last; tile += nwaves) {
                TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
                const int64_t base = tile * kTileElems + (int64_t)lane * 4;
#pragma unroll 4
                for (int it = 0; it < kTileIters; ++it) {
                    const int64_t e = base + it * 256;
                    float v[4];
                    if constexpr (D == Dist::Normal) rng.normal4(v); else rng.uniform4(v);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] = aff(v[k]);
                        if (mul_now) v[k] = v[k] * factor;
                    }
                    if (e + 4 <= inner) {
                        if (vec) *reinterpret_cast<float4*>(o + e) = make_float4(v[0], v[1], v[2], v[3]);
                        else {
#pragma unroll
                            for (int k = 0; k < 4; ++k) o[e + k] = v[k];
                        }
                        if constexpr (NORM != 0) group_stats(v, s, q);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (e + k < inner) {
                                o[e + k] = v[k];
                                if constexpr (NORM != 0) {
                                    s += (double)v[k];
                                    q += (double)v[k] * (double)v[k];
                                }
                            }
                    }
                }
            }
            if constexpr (NORM != 0) {
                block_sum2<kBlock>(s, q, red);
                if (threadIdx.x == 0) {
                    part[2 * b] = s;
                    part[2 * b + 1] = q;
                }
                __syncthreads();  // (red: the next turn's sums; part: the decision's reads)
            }
        }
        if constexpr (NORM != 0) {
            // ---- the decision: decide_norm over the row's own slots
            double s = 0.0, q = 0.0;
            for (int i = threadIdx.x; i < nvb; i += kBlock) {
                s += part[2 * i];
                q += part[2 * i + 1];
            }
            const NormDecision d = decide_from_sums<kBlock>(s, q, inner, thr_sd, red, &sh);
            const NormFast fast(d, factor);
            const bool do_mul = factor != 1.0f;
            const bool touch = NORM == 1 ? (d.do_sub || d.do_div || do_mul) : (fast.do_sub || fast.do_scale);
            __syncthreads();  // (sh, red, part: the next row's)
            if (!touch) continue;
            auto f = [&](float v) {
                if constexpr (NORM == 1) return apply_norm(v, d, factor, do_mul);
                else return fast(v);
            };
            // ---- the correction: every thread over the values it stored itself
            for (int b = 0; b < nvb; ++b)
                for (int64_t tile = (int64_t)b * (kBlock / 64) + w; tile <= last; tile += nwaves) {
                    const int64_t base = tile * kTileElems + (int64_t)lane * 4;
#pragma unroll 4
                    for (int it = 0; it < kTileIters; ++it) {
                        const int64_t e = base + it * 256;
                        if (vec && e + 4 <= inner) {
                            const float4 x = *reinterpret_cast<const float4*>(o + e);
                            *reinterpret_cast<float4*>(o + e) = make_float4(f(x.x), f(x.y), f(x.z), f(x.w));
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (e + k < inner) o[e + k] = f(o[e + k]);
                        }
                    }
                }
        }
    }
}

template <Dist D>
static int launch_rows(float* out, int64_t rows, int64_t inner, const RowKeys& keys, Affine aff, float factor, int normalized, float thr,
                       hipStream_t st) {
    const int nvb = tile_grid(inner, 0);
    const int g = (int)std::min<int64_t>(rows, 1 << 16);
#define SONAR_ROWS(N) hipLaunchKernelGGL((philox_rows_kernel<D, N>), dim3(g), dim3(kBlock), 0, st, out, rows, inner, keys, nvb, aff, factor, thr)
    if (normalized == SONAR_ROWS_NORM_NONE) SONAR_ROWS(0);
    else if (normalized == SONAR_ROWS_NORM_SCALE_NOISE) SONAR_ROWS(1);
    else SONAR_ROWS(2);
#undef SONAR_ROWS
    return check_launch("sonar_philox_rows_f32");
}

}  // namespace sonar

using namespace sonar;

extern "C" int64_t sonar_philox_rows_max_inner(void) { return kRowsMaxInner; }

extern "C" int sonar_philox_rows_f32(float* out, int64_t rows, int64_t inner, const uint64_t* row_seed, const uint64_t* row_stream,
                                     int uniform, uint64_t stream_id, float sub, float mul, float add, float factor, int normalized,
                                     float threshold_std_devs, void* stream) {
    SONAR_REQUIRE(rows >= 0 && inner > 0, SONAR_ERR_UNSUPPORTED, "sonar_philox_rows_f32: rows >= 0 and inner > 0 (got %lld x %lld)",
                  (long long)rows, (long long)inner);
    SONAR_REQUIRE(inner <= kRowsMaxInner, SONAR_ERR_UNSUPPORTED, "sonar_philox_rows_f32: at most %lld elements per row (got %lld)",
                  (long long)kRowsMaxInner, (long long)inner);
    SONAR_REQUIRE(row_seed || rows == 0, SONAR_ERR_UNSUPPORTED, "sonar_philox_rows_f32: rows without their seeds");
    SONAR_REQUIRE(normalized >= SONAR_ROWS_NORM_NONE && normalized <= SONAR_ROWS_NORM_FUSED, SONAR_ERR_ARG,
                  "sonar_philox_rows_f32: unknown normalisation %d", normalized);
    if (rows == 0) return SONAR_OK;
    SONAR_REQUIRE(out && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, SONAR_ERR_ARG, "sonar_philox_rows_f32: bad argument");
    const RowKeys keys{row_seed, row_stream, stream_id};
    if (uniform) {
        const int active = !(sub == 0.0f && mul == 1.0f && add == 0.0f);
        return launch_rows<Dist::Uniform>(out, rows, inner, keys, Affine{sub, mul, add, active}, factor, normalized, threshold_std_devs,
                                          (hipStream_t)stream);
    }
    return launch_rows<Dist::Normal>(out, rows, inner, keys, Affine{0.f, 1.f, 0.f, 0}, factor, normalized, threshold_std_devs,
                                     (hipStream_t)stream);
}
