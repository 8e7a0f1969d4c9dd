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

// ------------------------------------------------------------------------------------------------
// Row-keyed Perlin noise: per row what the loop's batch-1 PerlinOldNoiseGenerator call computes, to the bit.  The contract, read from
// py/noise_generation.py (_device_generate) and noise_perlin.hip (launch_perlin_generate, perlin_generate_kernel, perlin_fast_tiles):
//   keys     a generate-mode generator takes device_key(2): the values are drawn with (seed, stream), the lattice with (seed, stream + 1).
//            Here stream = stream_id + row_stream[row].
//   lattice  a batch shares one [C, H, W] lattice, a batch of ONE latent has its own: one per row, perlin_lattice_cells (the per-call
//            kernel's own function: a cell's value does not depend on which block computes it) into the row's slice of the workspace.
//   values   u / div_fac + lattice[e], element offset 0, ONE summed table: the route is a function of chw alone (a fresh batch-1 output is
//            16-byte aligned) -- chw % 4 != 0 scalar, else chw < 256 vector, else chw % 4096 != 0 fast, else tile-aligned.  The fast routes
//            convert the generator word with with_divider's WordScale / WordDivide, the general ones run uniform4 and Divider::operator()
//            and add the term (StepScale below; WordDivide's expression is already the general one for a divisor that is no power of two).
//   sums     (normalised: sonar_perlin_noise_f32's MODE 1 pass) g = tile_grid(chw, 0) workgroups, wave 4 b + w takes tiles 4 b + w,
//            4 b + w + 4 g, ...; fast routes: a tile's 64 values per lane in fp32 (ts, and tq through the fma chain that starts from tq),
//            added to the fp64 pair once per tile; vector: a group of four in fp32 (group_stats), then fp64; scalar: the same for a whole
//            group, per element in fp64 for the ragged one.  Then block_sum2 into slot b and decide_norm's walk t, t + 256, ... -- played
//            here turn by turn as philox_rows_kernel plays the fills.
//   final    MODE 2 draws the values again and stores NormFast(decision, factor) of them; so does this kernel (a second draw, not a
//            store and a correction: a Perlin row's mean is 0.5 / div_fac, the correction would run for nearly every row, and the second
//            draw costs the generator words and a cached lattice read where the correction costs a read and a second write of the row).
//            Unnormalised: the raw values, times `factor` when it is not 1 (a rounding of its own in the loop: scale_noise_).
// The address of a row inside `out` decides only how it is stored (16-byte stores on an aligned row), never the order of a sum.
enum PerlinRoute { kRouteScalar = 0, kRouteVector = 1, kRouteFast = 2, kRouteAligned = 3 };

struct StepScale {  // Divider::operator() with a power-of-two divisor, then the term: two rounded steps, as perlin_generate_kernel's general loop
    float inv;
    __device__ __forceinline__ float from_word(uint32_t r, float term) const { return u01(r) * inv + term; }
};
struct MulT {
    float factor;
    __device__ __forceinline__ float operator()(float v) const { return v * factor; }
};

struct PerlinRowsGeom {
    int64_t C;
    int H, W, iters, blend_mode;
};

// the tiles first, first + step, ... of one row: STATS adds this thread's share to (s, q) in the route's order, STORE writes fin(value)
template <int ROUTE, bool STATS, bool STORE, typename CONV, typename FIN>
__device__ __forceinline__ void perlin_row_tiles(const float* lat, float* o, bool vec, int64_t inner, uint64_t seed, uint64_t stream_id,
                                                 int64_t first, int64_t step, const CONV& cv, const FIN& fin, double& s, double& q) {
    const uint32_t lane = threadIdx.x & 63;
    const int64_t last = (inner - 1) / kTileElems;
    for (int64_t tile = first; tile <= last; tile += step) {
        TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4;
        float ts = 0.0f, tq = 0.0f;
#pragma unroll 4
        for (int it = 0; it < kTileIters; ++it) {
            uint32_t r[4];
            rng.words4_high(r);  // (uniform4 is u01 of the same four words)
            const int64_t e = base + it * 256;
            if constexpr (ROUTE != kRouteAligned) {
                if (e >= inner) continue;
            }
            const bool whole = ROUTE != kRouteScalar || e + 4 <= inner;
            float v[4];
            if constexpr (ROUTE != kRouteScalar) {
                const float4 t = *reinterpret_cast<const float4*>(lat + e);
                v[0] = cv.from_word(r[0], t.x); v[1] = cv.from_word(r[1], t.y);
                v[2] = cv.from_word(r[2], t.z); v[3] = cv.from_word(r[3], t.w);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = cv.from_word(r[k], e + k < inner ? lat[e + k] : 0.0f);
            }
            if constexpr (STATS) {
                if constexpr (ROUTE >= kRouteFast) {
                    ts += (v[0] + v[1]) + (v[2] + v[3]);
                    tq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[3], v[3], tq))));
                } else if (whole) {
                    group_stats(v, s, q);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k < inner) {
                            s += (double)v[k];
                            q += (double)v[k] * (double)v[k];
                        }
                }
            }
            if constexpr (STORE) {
                if (whole && vec) {
                    *reinterpret_cast<float4*>(o + e) = make_float4(fin(v[0]), fin(v[1]), fin(v[2]), fin(v[3]));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k < inner) o[e + k] = fin(v[k]);
                }
            }
        }
        if constexpr (STATS && ROUTE >= kRouteFast) {
            s += (double)ts;
            q += (double)tq;
        }
    }
}

template <int ROUTE, bool NORM, typename CONV>
__global__ void __launch_bounds__(kBlock) perlin_rows_kernel(float* out, float* lattice, int64_t rows, int64_t inner, PerlinRowsGeom geo,
                                                             RowKeys keys, int nvb, CONV cv, float factor, float thr_sd) {
    kernarg_touch_for(out, lattice, rows, inner, geo, keys, nvb, cv, factor, thr_sd);
    __shared__ double red[2 * kBlock / 64];
    __shared__ double part[NORM ? 2 * kNPart : 2];
    __shared__ NormDecision sh;
    const int w = threadIdx.x >> 6;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        float* const o = out + row * inner;
        float* const lat = lattice + row * inner;  // (16-byte aligned on the vector routes: the workspace is, and inner % 4 == 0 there)
        const bool vec = (reinterpret_cast<uintptr_t>(o) & 15u) == 0;
        const uint64_t seed = keys.seed[row];
        const uint64_t stream_id = keys.stream_id + (keys.stream ? keys.stream[row] : 0);
        // ---- the row's own lattice, as block 0 of 1; the barrier (with its workgroup-scope fences) lets every thread of the block read
        // what the others wrote: one compute unit, one vector cache
        perlin_lattice_cells(lat, geo.iters, geo.C, geo.H, geo.W, geo.blend_mode, seed, stream_id + 1, 0, 1);
        __syncthreads();
        double s = 0.0, q = 0.0;
        if constexpr (NORM) {
            // ---- the statistics pass, turn b the per-call launch's workgroup b
            for (int b = 0; b < nvb; ++b) {
                s = 0.0;
                q = 0.0;
                perlin_row_tiles<ROUTE, true, false>(lat, o, vec, inner, seed, stream_id, (int64_t)b * (kBlock / 64) + w,
                                                     (int64_t)nvb * (kBlock / 64), cv, MulT{1.0f}, s, q);
                block_sum2<kBlock>(s, q, red);
                if (threadIdx.x == 0) {
                    part[2 * b] = s;
                    part[2 * b + 1] = q;
                }
                __syncthreads();  // (red: the next turn's sums; part: the decision's reads)
            }
            // ---- the decision: decide_norm over the row's own slots
            s = 0.0;
            q = 0.0;
            for (int i = threadIdx.x; i < nvb; i += kBlock) {
                s += part[2 * i];
                q += part[2 * i + 1];
            }
            const NormDecision d = decide_from_sums<kBlock>(s, q, inner, thr_sd, red, &sh);
            const NormFast fast(d, factor);
            __syncthreads();  // (sh, red, part: the next row's)
            // ---- the final pass: the values drawn again, normalised, stored once
            with_norm_flags(fast, [&](auto nm) {
                perlin_row_tiles<ROUTE, false, true>(lat, o, vec, inner, seed, stream_id, w, kBlock / 64, cv, nm, s, q);
            });
        } else if (factor != 1.0f) {
            perlin_row_tiles<ROUTE, false, true>(lat, o, vec, inner, seed, stream_id, w, kBlock / 64, cv, MulT{factor}, s, q);
        } else {
            perlin_row_tiles<ROUTE, false, true>(lat, o, vec, inner, seed, stream_id, w, kBlock / 64, cv, NormT<false, false>{0.f, 1.f, 1.f}, s, q);
        }
    }
}

template <int ROUTE, typename CONV>
static void launch_perlin_rows_conv(float* out, float* lattice, int64_t rows, int64_t inner, const PerlinRowsGeom& geo, const RowKeys& keys,
                                    CONV cv, float factor, int normalized, float thr, hipStream_t st) {
    const int nvb = tile_grid(inner, 0);
    const int g = (int)std::min<int64_t>(rows, 1 << 16);
    if (normalized == SONAR_ROWS_NORM_NONE)
        hipLaunchKernelGGL((perlin_rows_kernel<ROUTE, false, CONV>), dim3(g), dim3(kBlock), 0, st, out, lattice, rows, inner, geo, keys, nvb, cv,
                           factor, thr);
    else
        hipLaunchKernelGGL((perlin_rows_kernel<ROUTE, true, CONV>), dim3(g), dim3(kBlock), 0, st, out, lattice, rows, inner, geo, keys, nvb, cv,
                           factor, thr);
}

template <int ROUTE>
static void launch_perlin_rows(float* out, float* lattice, int64_t rows, int64_t inner, const PerlinRowsGeom& geo, const RowKeys& keys,
                               float div_fac, float factor, int normalized, float thr, hipStream_t st) {
    const Divider divide(div_fac);
    if (!divide.exact) launch_perlin_rows_conv<ROUTE>(out, lattice, rows, inner, geo, keys, WordDivide{divide.d}, factor, normalized, thr, st);
    else if (ROUTE >= kRouteFast)
        launch_perlin_rows_conv<ROUTE>(out, lattice, rows, inner, geo, keys, WordScale{divide.inv * 0x1p-24f}, factor, normalized, thr, st);
    else launch_perlin_rows_conv<ROUTE>(out, lattice, rows, inner, geo, keys, StepScale{divide.inv}, factor, normalized, thr, st);
}

}  // namespace sonar

using namespace sonar;

extern "C" int sonar_perlin_rows_f32(float* out, float* lattice, int64_t rows, int64_t C, int64_t H, int64_t W, int64_t iters, int blend_mode,
                                     float div_fac, const uint64_t* row_seed, const uint64_t* row_stream, uint64_t stream_id, float factor,
                                     int normalized, float threshold_std_devs, void* stream) {
    const char* what = "sonar_perlin_rows_f32";
    SONAR_REQUIRE(C > 0 && H > 0 && W > 0 && iters >= 0 && iters < (1 << 20) && blend_mode >= 0 && blend_mode <= 2, SONAR_ERR_ARG,
                  "%s: bad argument (C, H, W > 0, 0 <= iters < 2^20, blend mode 0..2)", what);
    SONAR_REQUIRE(normalized == SONAR_ROWS_NORM_NONE || normalized == SONAR_ROWS_NORM_FUSED, SONAR_ERR_ARG,
                  "%s: unknown normalisation %d (SONAR_ROWS_NORM_NONE or SONAR_ROWS_NORM_FUSED)", what, normalized);
    SONAR_REQUIRE(rows >= 0, SONAR_ERR_UNSUPPORTED, "%s: rows >= 0 (got %lld)", what, (long long)rows);
    SONAR_REQUIRE(H < (1 << 20) && W < (1 << 20), SONAR_ERR_UNSUPPORTED, "%s: plane too large", what);
    SONAR_REQUIRE(C <= kRowsMaxInner && H * W <= kRowsMaxInner && C * H * W <= kRowsMaxInner, SONAR_ERR_UNSUPPORTED, "%s: at most %lld elements per row (got %lld x %lld x %lld)",
                  what, (long long)kRowsMaxInner, (long long)C, (long long)H, (long long)W);
    SONAR_REQUIRE(row_seed || rows == 0, SONAR_ERR_UNSUPPORTED, "%s: rows without their seeds", what);
    if (rows == 0) return SONAR_OK;
    SONAR_REQUIRE(out && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 && lattice && aligned16(lattice) && lattice != out, SONAR_ERR_ARG,
                  "%s: bad argument (out aligned to a float, a 16-byte aligned lattice workspace of its own)", what);
    const int64_t inner = C * H * W;
    const PerlinRowsGeom geo{C, (int)H, (int)W, (int)iters, blend_mode};
    const RowKeys keys{row_seed, row_stream, stream_id};
    hipStream_t st = (hipStream_t)stream;
    // launch_perlin_generate's choice for ONE latent of `inner` elements on 16-byte aligned tensors, one summed table, element offset 0
    if (inner % 4 != 0) launch_perlin_rows<kRouteScalar>(out, lattice, rows, inner, geo, keys, div_fac, factor, normalized, threshold_std_devs, st);
    else if (inner < 256) launch_perlin_rows<kRouteVector>(out, lattice, rows, inner, geo, keys, div_fac, factor, normalized, threshold_std_devs, st);
    else if (inner % kTileElems != 0) launch_perlin_rows<kRouteFast>(out, lattice, rows, inner, geo, keys, div_fac, factor, normalized, threshold_std_devs, st);
    else launch_perlin_rows<kRouteAligned>(out, lattice, rows, inner, geo, keys, div_fac, factor, normalized, threshold_std_devs, st);
    return check_launch(what);
}

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
