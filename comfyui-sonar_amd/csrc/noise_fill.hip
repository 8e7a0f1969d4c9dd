// Base generators (Philox normal / uniform): the stream fills, their normalising and look-ahead forms, and the pair fold that draws
// two tile-keyed chain items in one pass.  Output-write-bound: every kernel streams 16 B/lane stores of contiguous NCHW latents
// and, when asked, folds the whole-tensor (sum, sumsq) partials of the normaliser into the same pass.
#include "noise_stream.h"

namespace sonar {

// VEC: out 16-B aligned and elem_offset % 4 == 0 -> dwordx4 stores
// WHOLE (round 6): whole tiles only, a plain store (no running sum to fold into): no range checks, the affine map's switch decided once per
// launch (store_group's checks and the switch were a branch and a select per group: the fill of 134 MB was ~10 % instruction-bound).  The
// same values, the same per-thread sums in the same order.
template <Dist D, bool VEC, bool STATS, bool WHOLE = false>
__global__ void __launch_bounds__(kBlock) stream_fill_kernel(float* out, int64_t n, uint64_t seed, uint64_t stream_id,
                                                             int64_t elem_offset, Affine aff, double* partials, Accum acc) {
    kernarg_touch_for(out, n, seed, stream_id, elem_offset, aff, partials, acc);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    if constexpr (WHOLE) {
        const uint32_t lane = threadIdx.x & 63;
        const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
        const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
        const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
        auto tiles = [&](auto af) {
            for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
                TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
                float* const o = out + (tile * kTileElems + (int64_t)lane * 4 - elem_offset);
#pragma unroll 4
                for (int it = 0; it < kTileIters; ++it) {
                    float v[4];
                    if constexpr (D == Dist::Normal) rng.normal4(v); else rng.uniform4(v);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = af(v[k]);
                    *reinterpret_cast<float4*>(o + it * 256) = make_float4(v[0], v[1], v[2], v[3]);
                    if constexpr (STATS) {
                        const float ps = (v[0] + v[1]) + (v[2] + v[3]);
                        const float pq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], v[3] * v[3])));
                        s += (double)ps;
                        q += (double)pq;
                    }
                }
            }
        };
        if (aff.active) tiles(AffineT<true>{aff.sub, aff.mul, aff.add});
        else tiles(AffineT<false>{aff.sub, aff.mul, aff.add});
    } else {
        for_each_group<D>(n, seed, stream_id, elem_offset, [&](int64_t e, float (&v)[4]) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = aff(v[k]);
            accumulate_group<VEC>(acc, n, e, v);
            store_group<VEC>(out, n, e, v, s, q, STATS);
        });
    }
    if constexpr (STATS) write_partial<kBlock>(s, q, partials, red);
}

template <Dist D>
static int launch_fill(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset, Affine aff,
                       double* partials, hipStream_t st, const char* what, Accum acc = kNoAccum) {
    if (n == 0) return SONAR_OK;
    const bool vec = aligned16(out) && aligned16(acc.y) && (elem_offset & 3) == 0;
    const int g = tile_grid(n, elem_offset);
    if (vec && !acc.y && n % kTileElems == 0 && elem_offset % kTileElems == 0) {
        if (partials) hipLaunchKernelGGL((stream_fill_kernel<D, true, true, true>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials, acc);
        else hipLaunchKernelGGL((stream_fill_kernel<D, true, false, true>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials, acc);
        return check_launch(what);
    }
#define SONAR_FILL(A, S) \
    hipLaunchKernelGGL((stream_fill_kernel<D, A, S>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials, acc)
    if (vec) {
        if (partials) SONAR_FILL(true, true); else SONAR_FILL(true, false);
    } else {
        if (partials) SONAR_FILL(false, true); else SONAR_FILL(false, false);
    }
#undef SONAR_FILL
    return check_launch(what);
}

// Two tile-keyed generators in one pass over a chain's running sum: the HOST item (1 Gaussian draw, 2 Perlin) folds its values as its
// own accumulating kernel would, after the previous item (PRE, same kinds; `pre.fresh`: the chain's first) has been applied on the
// fly.  Whole groups of four only (n, elem_offset multiples of 4, 16-byte aligned tensors, Perlin latents of a multiple of 4).
template <int HOST, int PRE, bool STATS>
__global__ void __launch_bounds__(kBlock) pair_fold_kernel(Accum fold, int64_t n, int64_t elem_offset, Prefix host, Prefix pre, double* partials) {
    kernarg_touch_for(fold, n, elem_offset, host, pre, partials);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    const Accum pfold{fold.y, pre.ya, pre.f};
    const Divider hdiv(HOST == 2 ? host.div_fac : 1.0f), pdiv(PRE == 2 ? pre.div_fac : 1.0f);
    for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
        TileRng hrng = rng_stream(host.seed, host.stream_id, (uint64_t)tile, lane);
        TileRng prng = rng_stream(pre.seed, pre.stream_id, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
        // positions inside the latent (the lattices repeat per latent; shards start on a latent boundary), kept incrementally
        int rh = HOST == 2 ? (int)(((base % host.chw) + host.chw) % host.chw) : 0;
        int rp = PRE == 2 ? (int)(((base % pre.chw) + pre.chw) % pre.chw) : 0;
#pragma unroll 4
        for (int it = 0; it < kTileIters; ++it) {
            const int64_t e = base + it * 256;
            const bool ours = e >= 0 && e < n;
            float4 th = make_float4(0.0f, 0.0f, 0.0f, 0.0f), tp = th;
            if constexpr (HOST == 2) {
                if (ours) th = *reinterpret_cast<const float4*>(host.terms + rh);
                rh += 256;
                while (rh >= host.chw) rh -= host.chw;
            }
            if constexpr (PRE == 2) {
                if (ours) tp = *reinterpret_cast<const float4*>(pre.terms + rp);
                rp += 256;
                while (rp >= pre.chw) rp -= pre.chw;
            }
            float v[4], x[4];
            prefix_draw<HOST>(hrng, hdiv, th, v);
            prefix_draw<PRE>(prng, pdiv, tp, x);
            if (!ours) continue;
            prefix_fold(pre, pfold, fold, e, x, v);
            store_group<true>(const_cast<float*>(fold.y), n, e, v, s, q, STATS);
        }
    }
    if constexpr (STATS) write_partial<kBlock>(s, q, partials, red);
}

int launch_pair_fold(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int host_kind, const Prefix& host, int64_t n,
                     int64_t elem_offset, hipStream_t st, const char* what) {
    SONAR_REQUIRE(acc && acc->y && pre && n >= 0 && elem_offset >= 0, SONAR_ERR_ARG, "%s: bad argument", what);
    Prefix px;
    const int rc = make_prefix(pre, px, what);
    if (rc != SONAR_OK) return rc;
    SONAR_REQUIRE(n % 4 == 0 && elem_offset % 4 == 0 && aligned16(acc->y) && (host_kind != SONAR_PREFIX_PERLIN || host.chw % 4 == 0) &&
                      (pre->kind != SONAR_PREFIX_PERLIN || pre->chw % 4 == 0),
                  SONAR_ERR_UNSUPPORTED, "%s: hosting a fold prefix needs whole 4-element groups and 16-byte aligned tensors", what);
    if (n == 0) return SONAR_OK;
    const Accum fold{acc->y, acc->y_mul, acc->x_mul};
    const int g = tile_grid(n, elem_offset);
#define SONAR_PF(H, P) \
    do { \
        if (acc->partials) hipLaunchKernelGGL((pair_fold_kernel<H, P, true>), dim3(g), dim3(kBlock), 0, st, fold, n, elem_offset, host, px, acc->partials); \
        else hipLaunchKernelGGL((pair_fold_kernel<H, P, false>), dim3(g), dim3(kBlock), 0, st, fold, n, elem_offset, host, px, acc->partials); \
    } while (0)
    const bool hp = host_kind == SONAR_PREFIX_PERLIN, pp = pre->kind == SONAR_PREFIX_PERLIN;
    if (hp && pp) SONAR_PF(2, 2); else if (hp) SONAR_PF(2, 1); else if (pp) SONAR_PF(1, 2); else SONAR_PF(1, 1);
#undef SONAR_PF
    return check_launch(what);
}

// Normalised fill without a second sweep: MODE 1 re-draws the values and only reduces their statistics (no stores), MODE 2
// re-draws them again, normalises with the decision derived from those statistics and stores -- the tensor is written once
// (GaussianNoiseGenerator / UniformNoiseGenerator followed by scale_noise(normalized=True), py/noise_generation.py:252-260,496-514)
template <Dist D, bool VEC, int MODE>
__global__ void __launch_bounds__(kBlock) stream_fill_norm_kernel(float* out, int64_t n, uint64_t seed, uint64_t stream_id,
                                                                  int64_t elem_offset, Affine aff, double* partials, NormArgs na) {
    kernarg_touch_for(out, n, seed, stream_id, elem_offset, aff, partials, na);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    NormDecision dec{0.f, 1.f, 0, 0};
    if constexpr (MODE == 2) dec = decide_norm<kBlock>(na.partials, kNPart, na.n_total, na.thr_sd, red, &sh);
    const NormFast norm(dec, na.factor);
    double s = 0.0, q = 0.0;
    for_each_group<D>(n, seed, stream_id, elem_offset, [&](int64_t e, float (&v)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = aff(v[k]);
        if constexpr (MODE == 1) {
            if (e >= 0 && e + 4 <= n) {
                const float ps = (v[0] + v[1]) + (v[2] + v[3]);
                const float pq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], v[3] * v[3])));
                s += (double)ps;
                q += (double)pq;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k >= 0 && e + k < n) {
                        s += (double)v[k];
                        q += (double)v[k] * (double)v[k];
                    }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = norm(v[k]);
            store_group<VEC>(out, n, e, v, s, q, false);
        }
    });
    if constexpr (MODE == 1) write_partial<kBlock>(s, q, partials, red);
}

template <Dist D>
static int launch_fill_norm(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset, Affine aff, float factor,
                            float thr, double* partials, hipStream_t st, const char* what) {
    if (n == 0) return SONAR_OK;
    const bool vec = aligned16(out) && (elem_offset & 3) == 0;
    const int g = tile_grid(n, elem_offset);
    const NormArgs na{partials, n, factor, thr};
    hipLaunchKernelGGL((stream_fill_norm_kernel<D, true, 1>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials,
                       NormArgs{nullptr, 0, 1.0f, 0.0f});
    if (vec)
        hipLaunchKernelGGL((stream_fill_norm_kernel<D, true, 2>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials, na);
    else
        hipLaunchKernelGGL((stream_fill_norm_kernel<D, false, 2>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials, na);
    return check_launch(what);
}

// A sampler's steady state inside a prepared plan (the stream id of the call that follows is known): the final pass of THIS call and
// the statistics pass of the NEXT call as ONE launch (round 6; sonar_philox_noise_ahead_f32).  The final pass is store-bound (a 134 MB
// tensor: 24 us, 21 of them the write itself) with the vector ALUs idle most of the time; the statistics pass is nothing but vector-ALU
// work (15 us as a launch of its own).  A wave draws the next call's tile right behind this call's -- its statistics arithmetic issues
// while the stores of the step before are in flight.  Same grid, same tile -> wave -> step order, same per-thread sums and block
// reduction as stream_fill_norm_kernel<D, VEC, 1>: the partials left for the next call are the bits its own statistics pass would write.
// ALIGNED: whole tiles only (n and elem_offset multiples of kTileElems, 16-byte aligned output): no range checks at all
// EXACT: N(0,1) with factor 1, whose ordinary route stores the raw draws and leaves the (rare) correction to scale_noise_kernel
template <Dist D, bool VEC, bool ALIGNED, bool EXACT = false>
__global__ void __launch_bounds__(kBlock) stream_fill_ahead_kernel(float* out, int64_t n, uint64_t seed, uint64_t stream_id, uint64_t next_stream,
                                                                   int64_t elem_offset, Affine aff, NormArgs na, double* partials_next) {
    kernarg_touch_for(out, n, seed, stream_id, next_stream, elem_offset, aff, na, partials_next);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    const NormDecision dec = decide_norm<kBlock>(na.partials, kNPart, na.n_total, na.thr_sd, red, &sh);
    const NormFast norm(dec, na.factor);
    double s = 0.0, q = 0.0;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    if constexpr (ALIGNED) {
        auto tiles = [&](auto af, auto nm) {
            for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
                TileRng now = rng_stream(seed, stream_id, (uint64_t)tile, lane);
                TileRng nxt = rng_stream(seed, next_stream, (uint64_t)tile, lane);
                float* const o = out + (tile * kTileElems + (int64_t)lane * 4 - elem_offset);
#pragma unroll 4
                for (int it = 0; it < kTileIters; ++it) {
                    float v[4], u[4];
                    if constexpr (D == Dist::Normal) now.normal4(v); else now.uniform4(v);
                    *reinterpret_cast<float4*>(o + it * 256) = make_float4(nm(af(v[0])), nm(af(v[1])), nm(af(v[2])), nm(af(v[3])));
                    if constexpr (D == Dist::Normal) nxt.normal4(u); else nxt.uniform4(u);
#pragma unroll
                    for (int k = 0; k < 4; ++k) u[k] = af(u[k]);
                    const float ps = (u[0] + u[1]) + (u[2] + u[3]);
                    const float pq = __builtin_fmaf(u[0], u[0], __builtin_fmaf(u[1], u[1], __builtin_fmaf(u[2], u[2], u[3] * u[3])));
                    s += (double)ps;
                    q += (double)pq;
                }
            }
        };
        if constexpr (EXACT) with_exact_norm(dec, [&](auto nm) { tiles(AffineT<false>{0.0f, 1.0f, 0.0f}, nm); });
        else with_affine_norm(aff, norm, tiles);
    } else {
        double unused_s = 0.0, unused_q = 0.0;
        for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
            TileRng now = rng_stream(seed, stream_id, (uint64_t)tile, lane);
            TileRng nxt = rng_stream(seed, next_stream, (uint64_t)tile, lane);
            const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
#pragma unroll 4
            for (int it = 0; it < kTileIters; ++it) {
                const int64_t e = base + it * 256;
                float v[4], u[4];
                if constexpr (D == Dist::Normal) now.normal4(v); else now.uniform4(v);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = EXACT ? apply_norm(v[k], dec, 1.0f, false) : norm(aff(v[k]));
                store_group<VEC>(out, n, e, v, unused_s, unused_q, false);
                if constexpr (D == Dist::Normal) nxt.normal4(u); else nxt.uniform4(u);
#pragma unroll
                for (int k = 0; k < 4; ++k) u[k] = aff(u[k]);
                // (EXACT: the statistics the next call's own launch would leave are store_group<VEC>'s -- per element when the shape has no
                // vector path; the other shapes' statistics pass always takes whole groups where it can)
                if ((VEC || !EXACT) && e >= 0 && e + 4 <= n) {
                    const float ps = (u[0] + u[1]) + (u[2] + u[3]);
                    const float pq = __builtin_fmaf(u[0], u[0], __builtin_fmaf(u[1], u[1], __builtin_fmaf(u[2], u[2], u[3] * u[3])));
                    s += (double)ps;
                    q += (double)pq;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (e + k >= 0 && e + k < n) {
                            s += (double)u[k];
                            q += (double)u[k] * (double)u[k];
                        }
                }
            }
        }
    }
    __syncthreads();  // (red: the decision's reduction above, the partial's below)
    write_partial<kBlock>(s, q, partials_next, red);
}

template <Dist D>
static int launch_fill_ahead(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset, Affine aff, float factor, float thr,
                             double* partials, int have_stats, uint64_t next_stream, double* partials_next, hipStream_t st, const char* what) {
    if (n == 0) return SONAR_OK;
    const bool vec = aligned16(out) && (elem_offset & 3) == 0;
    const int g = tile_grid(n, elem_offset);
    const NormArgs na{partials, n, factor, thr};
    const bool unit_normal = D == Dist::Normal && factor == 1.0f;
    if (!have_stats) {  // nobody left this call's statistics (the first call, a reseed, another generator drew in between): its own pass
        if (unit_normal) {
            // the ordinary route's first launch (raw draws stored with their statistics; the stores are repeated below): its partials
            const int rc = launch_fill<D>(out, n, seed, stream_id, elem_offset, aff, partials, st, what);
            if (rc != SONAR_OK) return rc;
        } else {
            hipLaunchKernelGGL((stream_fill_norm_kernel<D, true, 1>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, elem_offset, aff, partials,
                               NormArgs{nullptr, 0, 1.0f, 0.0f});
        }
    }
    const bool whole = vec && n % kTileElems == 0 && elem_offset % kTileElems == 0;
#define SONAR_FA(V, AL) \
    hipLaunchKernelGGL((stream_fill_ahead_kernel<D, V, AL>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, next_stream, elem_offset, aff, na, partials_next)
    if (unit_normal) {
#define SONAR_FAE(V, AL) \
    hipLaunchKernelGGL((stream_fill_ahead_kernel<Dist::Normal, V, AL, true>), dim3(g), dim3(kBlock), 0, st, out, n, seed, stream_id, next_stream, elem_offset, aff, na, partials_next)
        if (whole) SONAR_FAE(true, true);
        else if (vec) SONAR_FAE(true, false);
        else SONAR_FAE(false, false);
#undef SONAR_FAE
    } else if (whole) SONAR_FA(true, true);
    else if (vec) SONAR_FA(true, false);
    else SONAR_FA(false, false);
#undef SONAR_FA
    return check_launch(what);
}

}  // namespace sonar

using namespace sonar;

// ================================================================================================
extern "C" int sonar_philox_normal_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                       double* partials, void* stream) {
    SONAR_REQUIRE(out && n >= 0 && elem_offset >= 0, SONAR_ERR_ARG, "sonar_philox_normal_f32: bad argument");
    return launch_fill<Dist::Normal>(out, n, seed, stream_id, elem_offset, Affine{0.f, 1.f, 0.f, 0}, partials,
                                     (hipStream_t)stream, "sonar_philox_normal_f32");
}

extern "C" int sonar_philox_uniform_f32(float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                        float sub, float mul, float add, double* partials, void* stream) {
    SONAR_REQUIRE(out && n >= 0 && elem_offset >= 0, SONAR_ERR_ARG, "sonar_philox_uniform_f32: bad argument");
    const int active = !(sub == 0.0f && mul == 1.0f && add == 0.0f);
    return launch_fill<Dist::Uniform>(out, n, seed, stream_id, elem_offset, Affine{sub, mul, add, active}, partials,
                                      (hipStream_t)stream, "sonar_philox_uniform_f32");
}

extern "C" int sonar_philox_noise_f32(int uniform, float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                      float sub, float mul, float add, float factor, float threshold_std_devs, double* partials,
                                      void* stream) {
    SONAR_REQUIRE(out && partials && n >= 0 && elem_offset >= 0, SONAR_ERR_ARG, "sonar_philox_noise_f32: bad argument");
    const int active = !(sub == 0.0f && mul == 1.0f && add == 0.0f);
    const Affine aff{sub, mul, add, uniform ? active : 0};
    if (uniform)
        return launch_fill_norm<Dist::Uniform>(out, n, seed, stream_id, elem_offset, aff, factor, threshold_std_devs, partials,
                                               (hipStream_t)stream, "sonar_philox_noise_f32");
    if (factor == 1.0f) {
        // N(0,1) draws with factor 1 almost never need the normalisation: the thresholds sit at 2.5 standard errors of the mean and
        // 3.5 of the standard deviation (98.7 % of tensors pass both).  So: ONE pass that stores the draws and reduces their
        // statistics, then scale_noise's own kernel, which takes the decision on the device and returns at once when there is
        // nothing to do -- instead of drawing everything twice (statistics pass + final pass: 26 + 32 us per 512 SDXL latents).
        const int rc = launch_fill<Dist::Normal>(out, n, seed, stream_id, elem_offset, aff, partials, (hipStream_t)stream, "sonar_philox_noise_f32");
        if (rc != SONAR_OK || n == 0) return rc;
        return sonar_scale_noise_f32(out, n, 1.0f, 1, threshold_std_devs, partials, kNPart, n, stream);
    }
    return launch_fill_norm<Dist::Normal>(out, n, seed, stream_id, elem_offset, aff, factor, threshold_std_devs, partials,
                                          (hipStream_t)stream, "sonar_philox_noise_f32");
}

extern "C" int sonar_philox_noise_ahead_ok(int uniform, int64_t n, float factor) {
    // N(0,1) with factor 1 has a one-pass route (draw once, store with statistics, a no-op scale_noise launch): drawing every normal twice
    // only pays while the call is launch-bound (batch 64: 12.4 -> 9.7 us; batch 512: 31.3 -> 35.8 us, the vector ALUs become the bound)
    if (!uniform && factor == 1.0f) return n > 0 && n <= kNtMaxElems ? 1 : 0;
    return n > 0 ? 1 : 0;
}

extern "C" int sonar_philox_noise_ahead_f32(int uniform, float* out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                            float sub, float mul, float add, float factor, float threshold_std_devs, double* partials,
                                            int have_stats, uint64_t next_stream_id, double* partials_next, void* stream) {
    SONAR_REQUIRE(out && partials && partials_next && partials != partials_next && n >= 0 && elem_offset >= 0, SONAR_ERR_ARG,
                  "sonar_philox_noise_ahead_f32: bad argument");
    const int active = !(sub == 0.0f && mul == 1.0f && add == 0.0f);
    const Affine aff{sub, mul, add, uniform ? active : 0};
    if (uniform)
        return launch_fill_ahead<Dist::Uniform>(out, n, seed, stream_id, elem_offset, aff, factor, threshold_std_devs, partials, have_stats,
                                                next_stream_id, partials_next, (hipStream_t)stream, "sonar_philox_noise_ahead_f32");
    return launch_fill_ahead<Dist::Normal>(out, n, seed, stream_id, elem_offset, aff, factor, threshold_std_devs, partials, have_stats,
                                           next_stream_id, partials_next, (hipStream_t)stream, "sonar_philox_noise_ahead_f32");
}

extern "C" int sonar_philox_normal_acc_f32(const sonar_accumulate* acc, int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                           void* stream) {
    SONAR_REQUIRE(accum_ok(acc) && n >= 0 && elem_offset >= 0, SONAR_ERR_ARG, "sonar_philox_normal_acc_f32: bad argument");
    return launch_fill<Dist::Normal>(acc->y, n, seed, stream_id, elem_offset, Affine{0.f, 1.f, 0.f, 0}, acc->partials, (hipStream_t)stream,
                                     "sonar_philox_normal_acc_f32", Accum{acc->y, acc->y_mul, acc->x_mul});
}

// the accumulating forms with the chain's previous item riding along (sonar_fold_prefix, see sonar_hip.h)
extern "C" int sonar_philox_normal_chain_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t n, uint64_t seed,
                                             uint64_t stream_id, int64_t elem_offset, void* stream) {
    return launch_pair_fold(acc, pre, SONAR_PREFIX_NORMAL, Prefix{1.0f, 1.0f, 1.0f, seed, stream_id, nullptr, 1, 0}, n, elem_offset,
                            (hipStream_t)stream, "sonar_philox_normal_chain_f32");
}
