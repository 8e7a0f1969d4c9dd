// Perlin lattice noise: terms, lattice, apply (replay) and generate kernels, the fast tile loops and the look-ahead launch of a
// prepared plan.  The generate kernels stream 16 B/lane stores like the fills (noise_stream.h) and fold the normaliser's partials.
#include "noise_stream.h"

namespace sonar {

// ------------------------------------------------------------------------------------------------
// Perlin: lattice term at cell centre (py/noise_generation.py:388-405 with positions == (0.5, 0.5)).
__global__ void __launch_bounds__(kBlock) perlin_terms_kernel(const float* __restrict__ angles, float* terms,
                                                               int64_t planes /*iters*C*/, int H, int W, int blend_mode) {
    kernarg_touch_for(angles, terms, planes, H, W, blend_mode);
    const int64_t total = planes * H * W;
    const int gw = W + 1;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int64_t p = i / ((int64_t)W * H);
        const float* a = angles + p * (int64_t)(H + 1) * gw + (int64_t)y * gw + x;
        const float a00 = a[0], a01 = a[1], a10 = a[gw], a11 = a[gw + 1];
        // gradient = (cos, sin); corner dot products with (pos - corner), pos = (0.5, 0.5)
        const float d0 = cosf(a00) * 0.5f + sinf(a00) * 0.5f;      // TL: ( 0.5,  0.5)
        const float d1 = cosf(a01) * -0.5f + sinf(a01) * 0.5f;     // TR: (-0.5,  0.5)
        const float d2 = cosf(a10) * 0.5f + sinf(a10) * -0.5f;     // BL: ( 0.5, -0.5)
        const float d3 = cosf(a11) * -0.5f + sinf(a11) * -0.5f;    // BR: (-0.5, -0.5)
        // smooth_step(0.5) = 0.5*0.5*(3 - 2*0.5) = 0.5 exactly
        const float row0 = blend<float>(blend_mode, d0, d1, 0.5f);
        const float row1 = blend<float>(blend_mode, d2, d3, 0.5f);
        terms[i] = blend<float>(blend_mode, row0, row1, 0.5f);
    }
}

__global__ void __launch_bounds__(kBlock) perlin_lattice_kernel(float* terms_sum, int iters, int64_t C, int H, int W, int blend_mode,
                                                                uint64_t seed, uint64_t stream_id) {
    kernarg_touch_for(terms_sum, iters, C, H, W, blend_mode, seed, stream_id);
    perlin_lattice_cells(terms_sum, iters, C, H, W, blend_mode, seed, stream_id, blockIdx.x, gridDim.x);
}

// out[b][i] = base[b][i]/div + terms[0][i] + terms[1][i] + ...   (terms broadcast over batch)
// replay: base read from memory.  One float4 per lane; chw % 4 == 0 on the vector path.
template <bool STATS, int V>
__global__ void __launch_bounds__(kBlock) perlin_apply_kernel(const float* __restrict__ base,
                                                               const float* __restrict__ terms, float* out, int64_t B,
                                                               int64_t chw, int iters, float div_fac, double* partials) {
    kernarg_touch_for(base, terms, out, B, chw, iters, div_fac, partials);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    const int64_t n = B * chw;
    const int64_t nv = n / V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nv; i += stride) {
        const int64_t e = i * V;
        const int64_t r = e % chw;
        float v[V];
        if constexpr (V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(base + e);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = base[e];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = v[k] / div_fac;
        for (int it = 0; it < iters; ++it) {
            const float* t = terms + (int64_t)it * chw + r;
            if constexpr (V == 4) {
                const float4 tt = *reinterpret_cast<const float4*>(t);
                v[0] += tt.x; v[1] += tt.y; v[2] += tt.z; v[3] += tt.w;
            } else {
                v[0] += t[0];
            }
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            out[e] = v[0];
        }
        if constexpr (STATS) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const double d = v[k];
                s += d; q += d * d;
            }
        }
    }
    if constexpr (STATS) write_partial<kBlock>(s, q, partials, red);
}

// The fast path's tile loop (device-drawn calls: ONE summed term table, vector-aligned latents): wave `wave` of `nwaves` takes the tiles
// first + wave, first + wave + nwaves, ...  MODE as in perlin_generate_kernel.  Shared by that kernel and perlin_ahead_kernel.
template <int MODE, bool STATS, bool ALIGNED, typename DIV, typename NORM>
__device__ __forceinline__ void perlin_fast_tiles(const float* __restrict__ terms, float* out, int64_t n, int64_t chw, uint64_t seed,
                                                  uint64_t stream_id, int64_t elem_offset, const NORM& norm, const DIV& divide,
                                                  const Accum& acc, int64_t wave, int64_t nwaves, double& s, double& q) {
    const uint32_t lane = threadIdx.x & 63;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    const int ichw = (int)chw;
    for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
        TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
        // position of the tile's first vector inside the latent; the prefetch cursor walks on in steps of 256 elements and wraps
        // at the latent's end (a tile may straddle two latents when chw is not a multiple of the tile)
        int rp = (int)(((base % chw) + chw) % chw);
        const float4* const trow = reinterpret_cast<const float4*>(terms + rp);  // ALIGNED: the tile's vectors sit at trow[it * 64]
        int fetched = 0;
        auto next_terms = [&]() {
            if constexpr (ALIGNED) return trow[64 * fetched++];  // unrolled callers: constant offsets in the load instructions
            const float4 t = *reinterpret_cast<const float4*>(terms + rp);
            rp += 256;
            rp -= rp >= ichw ? ichw : 0;  // chw >= 256 (launcher)
            return t;
        };
        float4 cur[4], nxt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = next_terms();
        float ts = 0.0f, tq = 0.0f;  // the tile's 64 values per lane in fp32, folded into the fp64 sums once per tile
#pragma unroll
        for (int g = 0; g < kTileIters / 4; ++g) {
            if (g + 1 < kTileIters / 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) nxt[j] = next_terms();
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[4];
                uint32_t r[4];
                rng.words4_high(r);
                const int64_t e = base + (4 * g + j) * 256;
                if constexpr (!ALIGNED) {
                    if (e < 0 || e >= n) continue;  // the two ends of a shard that does not start / end on a tile (whole groups of 4)
                }
                v[0] = divide.from_word(r[0], cur[j].x); v[1] = divide.from_word(r[1], cur[j].y);
                v[2] = divide.from_word(r[2], cur[j].z); v[3] = divide.from_word(r[3], cur[j].w);
                if constexpr (MODE == 2) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = norm(v[k]);
                }
                if constexpr (MODE != 1) {
                    if constexpr (MODE == 0) accumulate_group<true>(acc, n, e, v);
                    if constexpr (ALIGNED) {  // whole tiles inside the shard: no range checks (store_group's were a branch per group)
                        *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
                        double unused_s = 0.0, unused_q = 0.0;
                        store_group<true>(out, n, e, v, unused_s, unused_q, false);
                    }
                }
                if constexpr (STATS || MODE == 1) {
                    ts += (v[0] + v[1]) + (v[2] + v[3]);
                    tq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], __builtin_fmaf(v[3], v[3], tq))));
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
        }
        if constexpr (STATS || MODE == 1) {
            s += (double)ts;
            q += (double)tq;
        }
    }
}

// The final pass of one call (MODE 2: `terms`, `stream_id`, normalised, stored) and the statistics pass of the next (MODE 1: `terms_next`,
// `next_stream`, summed) for the same tiles in ONE wave, step by step (round 6): the statistics arithmetic issues while the stores of the
// steps before are in flight.  Per tile and lane the same values in the same order as the two separate loops above -- the stored bits and
// the (sum, sumsq) this thread adds up are theirs.  Whole tiles per latent only (ALIGNED).
template <typename DIV, typename NORM>
__device__ __forceinline__ void perlin_fast_tiles_pair(const float* __restrict__ terms, const float* __restrict__ terms_next, float* out, int64_t n,
                                                       int64_t chw, uint64_t seed, uint64_t stream_id, uint64_t next_stream, int64_t elem_offset,
                                                       const NORM& norm, const DIV& divide, int64_t wave, int64_t nwaves, double& s, double& q) {
    const uint32_t lane = threadIdx.x & 63;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
        TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
        TileRng rnx = rng_stream(seed, next_stream, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
        const int rp = (int)(((base % chw) + chw) % chw);
        const float4* const trow = reinterpret_cast<const float4*>(terms + rp);
        const float4* const tnxt = reinterpret_cast<const float4*>(terms_next + rp);
        float4 cur[4], nxt[4], curn[4], nxtn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cur[j] = trow[64 * j];
            curn[j] = tnxt[64 * j];
        }
        float ts = 0.0f, tq = 0.0f;
#pragma unroll
        for (int g = 0; g < kTileIters / 4; ++g) {
            if (g + 1 < kTileIters / 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    nxt[j] = trow[64 * (4 * (g + 1) + j)];
                    nxtn[j] = tnxt[64 * (4 * (g + 1) + j)];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t r[4];
                rng.words4_high(r);
                *reinterpret_cast<float4*>(out + base + (4 * g + j) * 256) =
                    make_float4(norm(divide.from_word(r[0], cur[j].x)), norm(divide.from_word(r[1], cur[j].y)),
                                norm(divide.from_word(r[2], cur[j].z)), norm(divide.from_word(r[3], cur[j].w)));
                uint32_t w[4];
                rnx.words4_high(w);
                const float v0 = divide.from_word(w[0], curn[j].x), v1 = divide.from_word(w[1], curn[j].y);
                const float v2 = divide.from_word(w[2], curn[j].z), v3 = divide.from_word(w[3], curn[j].w);
                ts += (v0 + v1) + (v2 + v3);
                tq = __builtin_fmaf(v0, v0, __builtin_fmaf(v1, v1, __builtin_fmaf(v2, v2, __builtin_fmaf(v3, v3, tq))));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cur[j] = nxt[j];
                curn[j] = nxtn[j];
            }
        }
        s += (double)ts;
        q += (double)tq;
    }
}

// Normalisation folded into the generating pass (SURVEY.md §8d "stats-before-write"): MODE 0 writes the
// raw values (+ optional statistics), MODE 1 only reduces the statistics (no stores), MODE 2 re-draws the
// same values, normalises them with the decision derived from `norm_partials` and writes the final tensor.
// generate: base u ~ U[0,1) drawn on device.  VEC: chw % 4 == 0, aligned pointers, elem_offset % 4 == 0.
// FAST (what every device-drawn call has: ONE summed term table, vector-aligned latents): the tile's 16 term vectors are requested
// four iterations ahead of their use by a cursor of their own (the general loop below waits for each load right where it issues it:
// at 4 waves per SIMD that wait, not the arithmetic, set the kernel's time), and there is no per-element tail path.
template <int MODE, bool VEC, bool STATS, bool FAST = false, bool ALIGNED = false>
__global__ void __launch_bounds__(kBlock) perlin_generate_kernel(const float* __restrict__ terms, float* out, int64_t B,
                                                                  int64_t chw, int iters, float div_fac, uint64_t seed,
                                                                  uint64_t stream_id, int64_t elem_offset, double* partials,
                                                                  NormArgs na, Accum acc) {
    kernarg_touch_for(terms, out, B, chw, iters, div_fac, seed, stream_id, elem_offset, partials, na, acc);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    NormDecision dec{0.f, 1.f, 0, 0};
    if constexpr (MODE == 2) dec = decide_norm<kBlock>(na.partials, kNPart, na.n_total, na.thr_sd, red, &sh);
    const NormFast norm(dec, na.factor);
    const Divider divide(div_fac);
    double s = 0.0, q = 0.0;
    const int64_t n = B * chw;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    const int ichw = (int)chw;  // launcher guarantees chw < 2^31
    if constexpr (FAST) {
        static_assert(VEC, "the fast path is a vector path");
        with_divider(divide, [&](auto dv) {
            if constexpr (MODE == 2) {  // the normalisation's switches decided once per launch, not per value
                with_norm_flags(norm, [&](auto nm) {
                    perlin_fast_tiles<MODE, STATS, ALIGNED>(terms, out, n, chw, seed, stream_id, elem_offset, nm, dv, acc, wave, nwaves, s, q);
                });
            } else {
                perlin_fast_tiles<MODE, STATS, ALIGNED>(terms, out, n, chw, seed, stream_id, elem_offset, norm, dv, acc, wave, nwaves, s, q);
            }
        });
        if constexpr (STATS || MODE == 1) write_partial<kBlock>(s, q, partials, red);
        return;
    }
    for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
        TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
        // position inside the latent (terms repeat per latent; shards start on a latent boundary), kept incrementally
        int r = (int)(((base % chw) + chw) % chw);
#pragma unroll 4
        for (int it = 0; it < kTileIters; ++it) {
            float v[4];
            rng.uniform4(v);
            const int64_t e = base + it * 256;
            const int rr = r;
            r += 256;
            while (r >= ichw) r -= ichw;
            if (e + 4 <= 0 || e >= n) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = divide(v[k]);
            for (int t_i = 0; t_i < iters; ++t_i) {
                const float* t = terms + (int64_t)t_i * chw;
                if (VEC) {
                    const float4 tt = *reinterpret_cast<const float4*>(t + rr);
                    v[0] += tt.x; v[1] += tt.y; v[2] += tt.z; v[3] += tt.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += t[(rr + k) % ichw];
                }
            }
            if constexpr (MODE == 2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = norm(v[k]);
            }
            if constexpr (MODE == 1) {
                if (VEC || (e >= 0 && e + 4 <= n)) {
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
                if constexpr (MODE == 0) accumulate_group<VEC>(acc, n, e, v);
                store_group<VEC>(out, n, e, v, s, q, STATS);
            }
        }
    }
    if constexpr (STATS || MODE == 1) write_partial<kBlock>(s, q, partials, red);
}

static int launch_perlin_apply(const float* base, const float* terms, float* out, int64_t B, int64_t chw, int64_t iters,
                               float div_fac, double* partials, hipStream_t st, const char* what) {
    const int64_t n = B * chw;
    if (n == 0) return SONAR_OK;
    const bool vec = (chw % 4 == 0) && aligned16(out) && aligned16(terms) && aligned16(base);
    const int g = (int)std::min<int64_t>(kNPart, grid_for(vec ? n / 4 : n, kBlock));
#define SONAR_PA(S, V) \
    hipLaunchKernelGGL((perlin_apply_kernel<S, V>), dim3(g), dim3(kBlock), 0, st, base, terms, out, B, chw, (int)iters, div_fac, partials)
    if (vec) {
        if (partials) SONAR_PA(true, 4); else SONAR_PA(false, 4);
    } else {
        if (partials) SONAR_PA(true, 1); else SONAR_PA(false, 1);
    }
#undef SONAR_PA
    return check_launch(what);
}

template <int MODE>
static int launch_perlin_generate(const float* terms, float* out, int64_t B, int64_t chw, int64_t iters, float div_fac,
                                  uint64_t seed, uint64_t stream_id, int64_t elem_offset, double* partials, NormArgs na,
                                  hipStream_t st, const char* what, Accum acc = kNoAccum) {
    const int64_t n = B * chw;
    if (n == 0) return SONAR_OK;
    const bool vec = (chw % 4 == 0) && (MODE == 1 || aligned16(out)) && (iters == 0 || aligned16(terms)) && (elem_offset % 4 == 0) &&
                     aligned16(acc.y);
    const int g = tile_grid(n, elem_offset);
    const bool fast = vec && iters == 1 && chw >= 256;
    const bool aligned = fast && chw % kTileElems == 0 && elem_offset % kTileElems == 0;  // every tile inside one latent and inside the shard
#define SONAR_PG(V, S) \
    hipLaunchKernelGGL((perlin_generate_kernel<MODE, V, S>), dim3(g), dim3(kBlock), 0, st, terms, out, B, chw, (int)iters, div_fac, seed, stream_id, elem_offset, partials, na, acc)
#define SONAR_PGF(S, AL) \
    hipLaunchKernelGGL((perlin_generate_kernel<MODE, true, S, true, AL>), dim3(g), dim3(kBlock), 0, st, terms, out, B, chw, (int)iters, div_fac, seed, stream_id, elem_offset, partials, na, acc)
    if (aligned) {
        if (partials && MODE == 0) SONAR_PGF(true, true); else SONAR_PGF(false, true);
    } else if (fast) {
        if (partials && MODE == 0) SONAR_PGF(true, false); else SONAR_PGF(false, false);
    } else if (vec) {
        if (partials && MODE == 0) SONAR_PG(true, true); else SONAR_PG(true, false);
    } else {
        if (partials && MODE == 0) SONAR_PG(false, true); else SONAR_PG(false, false);
    }
#undef SONAR_PG
#undef SONAR_PGF
    return check_launch(what);
}

// A sampler's steady state at launch-bound batch sizes (prepared plans: the stream ids of the calls that follow are known): the three
// dependent launches of a normalised Perlin call -- lattice, statistics pass, final pass -- become ONE, with nothing inside the launch
// depending on anything else inside it.  Blocks [lat_blocks, ...) run the final pass of THIS call (lattice `terms`, statistics `partials`:
// both left by earlier launches) and then the statistics pass of the NEXT call (its lattice `terms_next` left by the previous launch) into
// `partials_next`; blocks [0, lat_blocks) compute a lattice for a LATER call into `lattice_out`.  Same tile -> wave -> slot mapping, same
// arithmetic as perlin_generate_kernel<1 / 2, FAST, ALIGNED> and perlin_lattice_kernel: the same bits.
struct PerlinAhead {
    const float* terms;
    float* out;
    int64_t n, chw;
    float div_fac;
    uint64_t seed, stream_id;
    int64_t elem_offset;
    NormArgs na;                  // this call's statistics (complete before the launch) and its normalisation
    uint64_t next_stream_id;      // statistics of the next call: tiles drawn with this stream id against terms_next
    const float* terms_next;      // nullable: no statistics ahead
    double* partials_next;
    float* lattice_out;           // nullable: no lattice ahead
    int lat_blocks, tile_blocks, lat_iters, blend_mode;
    int fused;                    // one wave runs both passes for its tiles (the bandwidth-bound sizes); 0: separate, interleaved blocks
    int64_t C;
    int H, W;
    uint64_t lattice_stream_id;
};

__global__ void __launch_bounds__(kBlock) perlin_ahead_kernel(PerlinAhead a) {
    kernarg_touch_for(a);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    if ((int)blockIdx.x < a.lat_blocks) {
        perlin_lattice_cells(a.lattice_out, a.lat_iters, a.C, a.H, a.W, a.blend_mode, a.seed, a.lattice_stream_id, blockIdx.x, a.lat_blocks);
        return;
    }
    // the final pass of this call and the statistics pass of the next one are independent: separate blocks, so that at the launch-bound
    // sizes a wave runs ONE tile's chain, not two back to back -- and INTERLEAVED block by block (round 5), so that at the bandwidth-bound
    // sizes the two kinds are resident side by side: the final pass waits for its stores (a 134 MB tensor: 29 us, 21 of them the
    // write itself) with the vector ALUs idle, the statistics pass is nothing but vector ALU work (13 us as a launch of its own)
    const int nb = a.tile_blocks;
    const int blk = (int)blockIdx.x - a.lat_blocks;
    const Divider divide(a.div_fac);
    double s = 0.0, q = 0.0;
    if (a.fused) {
        // bandwidth-bound sizes (round 6): ONE wave runs this call's final pass and the next call's statistics pass for its tiles, step by
        // step -- the interleaved blocks below left the statistics waves done after 13 us and the storing waves on their own for the rest
        const int64_t wave = ((int64_t)blk * kBlock + threadIdx.x) >> 6, nwaves = ((int64_t)nb * kBlock) >> 6;
        const NormDecision dec = decide_norm<kBlock>(a.na.partials, kNPart, a.na.n_total, a.na.thr_sd, red, &sh);
        const NormFast norm(dec, a.na.factor);
        with_divider(divide, [&](auto dv) {
            with_norm_flags(norm, [&](auto nm) {
                perlin_fast_tiles_pair(a.terms, a.terms_next, a.out, a.n, a.chw, a.seed, a.stream_id, a.next_stream_id, a.elem_offset, nm, dv, wave, nwaves,
                                       s, q);
            });
        });
        __syncthreads();  // (red: the decision's reduction above, the partial's below)
        write_partial_at<kBlock>(s, q, a.partials_next, red, blk, nb);
        return;
    }
    const bool ahead = a.terms_next != nullptr && (blk & 1);
    const int bid = a.terms_next != nullptr ? blk >> 1 : blk;
    const int64_t wave = ((int64_t)bid * kBlock + threadIdx.x) >> 6, nwaves = ((int64_t)nb * kBlock) >> 6;
    if (!ahead) {
        const NormDecision dec = decide_norm<kBlock>(a.na.partials, kNPart, a.na.n_total, a.na.thr_sd, red, &sh);
        const NormFast norm(dec, a.na.factor);
        with_divider(divide, [&](auto dv) {
            with_norm_flags(norm, [&](auto nm) {
                perlin_fast_tiles<2, false, true>(a.terms, a.out, a.n, a.chw, a.seed, a.stream_id, a.elem_offset, nm, dv, kNoAccum, wave, nwaves, s, q);
            });
        });
    } else {
        const NormFast norm(NormDecision{0.f, 1.f, 0, 0}, 1.0f);
        with_divider(divide, [&](auto dv) {
            perlin_fast_tiles<1, false, true>(a.terms_next, nullptr, a.n, a.chw, a.seed, a.next_stream_id, a.elem_offset, norm, dv, kNoAccum, wave,
                                              nwaves, s, q);
        });
        write_partial_at<kBlock>(s, q, a.partials_next, red, bid, nb);
    }
}

}  // namespace sonar

using namespace sonar;

// ================================================================================================
extern "C" int sonar_perlin_generate_acc_f32(const sonar_accumulate* acc, const float* terms, int64_t B, int64_t chw, int64_t iters,
                                             float div_fac, uint64_t seed, uint64_t stream_id, int64_t elem_offset, void* stream) {
    SONAR_REQUIRE(accum_ok(acc) && (terms || iters == 0) && B >= 0 && chw > 0 && chw < (1LL << 31) && iters >= 0 && elem_offset >= 0,
                  SONAR_ERR_ARG, "sonar_perlin_generate_acc_f32: bad argument");
    return launch_perlin_generate<0>(terms, acc->y, B, chw, iters, div_fac, seed, stream_id, elem_offset, acc->partials, NormArgs{},
                                     (hipStream_t)stream, "sonar_perlin_generate_acc_f32", Accum{acc->y, acc->y_mul, acc->x_mul});
}

extern "C" int sonar_perlin_generate_chain_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, const float* terms, int64_t B,
                                               int64_t chw, float div_fac, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                               void* stream) {
    SONAR_REQUIRE(terms && aligned16(terms) && B >= 0 && chw > 0 && chw < (1LL << 31), SONAR_ERR_ARG,
                  "sonar_perlin_generate_chain_f32: bad argument (the summed, 16-byte aligned lattice is required)");
    return launch_pair_fold(acc, pre, SONAR_PREFIX_PERLIN, Prefix{1.0f, 1.0f, div_fac, seed, stream_id, terms, (int)chw, 0}, B * chw, elem_offset,
                            (hipStream_t)stream, "sonar_perlin_generate_chain_f32");
}

extern "C" int sonar_perlin_terms_f32(const float* angles, float* terms, int64_t iters, int64_t C, int64_t H, int64_t W,
                                      int blend_mode, void* stream) {
    SONAR_REQUIRE(angles && terms && iters >= 0 && C > 0 && H > 0 && W > 0 && blend_mode >= 0 && blend_mode <= 2,
                  SONAR_ERR_ARG, "sonar_perlin_terms_f32: bad argument");
    SONAR_REQUIRE(H < (1 << 20) && W < (1 << 20), SONAR_ERR_UNSUPPORTED, "sonar_perlin_terms_f32: plane too large");
    if (iters == 0) return SONAR_OK;
    const int64_t total = iters * C * H * W;
    hipLaunchKernelGGL(perlin_terms_kernel, dim3(grid_for(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, angles,
                       terms, iters * C, (int)H, (int)W, blend_mode);
    return check_launch("sonar_perlin_terms_f32");
}

extern "C" int sonar_perlin_lattice_f32(float* terms_sum, int64_t iters, int64_t C, int64_t H, int64_t W, int blend_mode, uint64_t seed,
                                        uint64_t stream_id, void* stream) {
    SONAR_REQUIRE(terms_sum && iters >= 0 && iters < (1 << 20) && C > 0 && H > 0 && W > 0 && blend_mode >= 0 && blend_mode <= 2,
                  SONAR_ERR_ARG, "sonar_perlin_lattice_f32: bad argument");
    SONAR_REQUIRE(H < (1 << 20) && W < (1 << 20), SONAR_ERR_UNSUPPORTED, "sonar_perlin_lattice_f32: plane too large");
    hipLaunchKernelGGL(perlin_lattice_kernel, dim3(grid_for(C * H * W, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, terms_sum,
                       (int)iters, C, (int)H, (int)W, blend_mode, seed, stream_id);
    return check_launch("sonar_perlin_lattice_f32");
}

extern "C" int sonar_perlin_apply_f32(const float* base, const float* terms, float* out, int64_t B, int64_t chw,
                                      int64_t iters, float div_fac, double* partials, void* stream) {
    SONAR_REQUIRE(base && out && (terms || iters == 0) && B >= 0 && chw > 0 && iters >= 0, SONAR_ERR_ARG,
                  "sonar_perlin_apply_f32: bad argument");
    return launch_perlin_apply(base, terms, out, B, chw, iters, div_fac, partials, (hipStream_t)stream, "sonar_perlin_apply_f32");
}

extern "C" int sonar_perlin_generate_f32(const float* terms, float* out, int64_t B, int64_t chw, int64_t iters,
                                         float div_fac, uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                         double* partials, void* stream) {
    SONAR_REQUIRE(out && (terms || iters == 0) && B >= 0 && chw > 0 && chw < (1LL << 31) && iters >= 0 && elem_offset >= 0, SONAR_ERR_ARG,
                  "sonar_perlin_generate_f32: bad argument");
    return launch_perlin_generate<0>(terms, out, B, chw, iters, div_fac, seed, stream_id, elem_offset, partials, NormArgs{},
                                     (hipStream_t)stream, "sonar_perlin_generate_f32");
}

extern "C" int sonar_perlin_noise_f32(const float* terms, float* out, int64_t B, int64_t chw, int64_t iters, float div_fac,
                                      uint64_t seed, uint64_t stream_id, int64_t elem_offset, float factor,
                                      float threshold_std_devs, double* partials, void* stream) {
    SONAR_REQUIRE(out && partials && (terms || iters == 0) && B >= 0 && chw > 0 && chw < (1LL << 31) && iters >= 0 && elem_offset >= 0, SONAR_ERR_ARG,
                  "sonar_perlin_noise_f32: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const NormArgs na{partials, B * chw, factor, threshold_std_devs};
    int rc = launch_perlin_generate<1>(terms, out, B, chw, iters, div_fac, seed, stream_id, elem_offset, partials, NormArgs{}, st,
                                       "sonar_perlin_noise_f32(stats)");
    if (rc != SONAR_OK) return rc;
    return launch_perlin_generate<2>(terms, out, B, chw, iters, div_fac, seed, stream_id, elem_offset, nullptr, na, st,
                                     "sonar_perlin_noise_f32(write)");
}

extern "C" int sonar_perlin_noise_ahead_ok(int64_t B, int64_t chw, int64_t elem_offset) {
    // the fast, tile-aligned shape of the device-drawn call (whole RNG tiles per latent, shards on tile boundaries).  (Up to round 4 also
    // "at most 4096 tiles": the launch-bound sizes only.  At 512 SDXL latents the statistics of the next call ride under the final pass's
    // stores: 41.9 -> see profiles/r05_fill_rates.txt.)
    const int64_t n = B * chw;
    return (n > 0 && chw >= 256 && chw < (1LL << 31) && chw % kTileElems == 0 && elem_offset >= 0 && elem_offset % kTileElems == 0 &&
            n / kTileElems <= (1 << 20)) ? 1 : 0;
}

extern "C" int sonar_perlin_noise_ahead_f32(const float* terms, float* out, int64_t B, int64_t chw, float div_fac, uint64_t seed, uint64_t stream_id,
                                            int64_t elem_offset, float factor, float threshold_std_devs, double* partials, int have_stats,
                                            uint64_t next_stream_id, const float* terms_next, double* partials_next, float* lattice_out,
                                            int64_t lattice_iters, int64_t C, int64_t H, int64_t W, int blend_mode, uint64_t lattice_stream_id,
                                            void* stream) {
    const char* what = "sonar_perlin_noise_ahead_f32";
    SONAR_REQUIRE(terms && out && partials && B >= 0 && chw > 0 && elem_offset >= 0 && (!terms_next || partials_next) &&
                      partials_next != partials, SONAR_ERR_ARG, "%s: bad argument", what);
    SONAR_REQUIRE(!lattice_out || (lattice_iters >= 0 && lattice_iters < (1 << 20) && C > 0 && H > 0 && W > 0 && H < (1 << 20) && W < (1 << 20) &&
                                   C * H * W == chw && blend_mode >= 0 && blend_mode <= 2 && lattice_out != terms && lattice_out != terms_next),
                  SONAR_ERR_ARG, "%s: bad lattice request", what);
    SONAR_REQUIRE(sonar_perlin_noise_ahead_ok(B, chw, elem_offset) && aligned16(out) && aligned16(terms) && (!terms_next || aligned16(terms_next)),
                  SONAR_ERR_UNSUPPORTED, "%s: whole 4096-element tiles per latent, 16-byte aligned tensors", what);
    if (B == 0) return SONAR_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!have_stats) {
        const int rc = launch_perlin_generate<1>(terms, out, B, chw, 1, div_fac, seed, stream_id, elem_offset, partials, NormArgs{}, st, what);
        if (rc != SONAR_OK) return rc;
    }
    PerlinAhead a{};
    a.terms = terms;
    a.out = out;
    a.n = B * chw;
    a.chw = chw;
    a.div_fac = div_fac;
    a.seed = seed;
    a.stream_id = stream_id;
    a.elem_offset = elem_offset;
    a.na = NormArgs{partials, B * chw, factor, threshold_std_devs};
    a.next_stream_id = next_stream_id;
    a.terms_next = terms_next;
    a.partials_next = partials_next;
    a.lattice_out = lattice_out;
    a.lat_blocks = lattice_out ? grid_for(chw, kBlock) : 0;
    a.lat_iters = (int)lattice_iters;
    a.blend_mode = blend_mode;
    a.C = C;
    a.H = (int)H;
    a.W = (int)W;
    a.lattice_stream_id = lattice_stream_id;
    a.tile_blocks = tile_grid(a.n, elem_offset);
    // a wave with a tile or more of its own to store has stores in flight to hide the next call's statistics behind (batch >= 256 SDXL
    // latents: the capped grid); below that the two passes go to separate blocks, twice as many waves with one short chain each
    a.fused = terms_next && a.tile_blocks == kNPart ? 1 : 0;
    hipLaunchKernelGGL(perlin_ahead_kernel, dim3(a.lat_blocks + a.tile_blocks * (terms_next && !a.fused ? 2 : 1)), dim3(kBlock), 0, st, a);
    return check_launch(what);
}
