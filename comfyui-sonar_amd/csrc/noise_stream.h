// Shared by the four generator units (noise_fill.hip, noise_perlin.hip, noise_pyramid.hip, noise_brownian.hip): the tile draw loop
// and its 16 B/lane group stores with the (sum, sumsq) partials of the normaliser, the accumulating and prefix folds of a chain, the
// affine / normalisation switches decided once per launch, and the Perlin lattice that the Perlin and the pyramid plane kernels both host.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "ew_driver.h"  // aligned16

namespace sonar {

#ifdef SONAR_NG_TRACE  // profiling builds: cycle stamps of thread 0 of the first 256 workgroups at the phase boundaries (scratch/ng_trace.py)
extern __device__ unsigned long long g_ng_trace[256 * 16];  // defined in noise_pyramid.hip, the one unit that stamps
#define SONAR_NG_STAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x < 256) g_ng_trace[blockIdx.x * 16 + (slot)] = __builtin_readcyclecounter(); } while (0)
#define SONAR_NG_STAMP_T(thread, slot) do { if ((int)threadIdx.x == (thread) && blockIdx.x < 256) g_ng_trace[blockIdx.x * 16 + (slot)] = __builtin_readcyclecounter(); } while (0)
#else
#define SONAR_NG_STAMP(slot) do { } while (0)
#define SONAR_NG_STAMP_T(thread, slot) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------------
// Draw loop shared by every generator: one wave per tile (common.h: kTileElems elements), each lane
// runs its own Philox-seeded multiply-with-carry burst (common.h, Mwc) and hands 4 consecutive elements per step to `f`.
// `f(e, v)` receives the LOCAL index e (may be < 0 or >= n at the two ends of a shard) of v[0].
enum class Dist { Normal, Uniform };

template <Dist D, typename F>
__device__ __forceinline__ void for_each_group(int64_t n, uint64_t seed, uint64_t stream_id, int64_t elem_offset, F&& f) {
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
        TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
#pragma unroll 4
        for (int it = 0; it < kTileIters; ++it) {
            float v[4];
            if constexpr (D == Dist::Normal) rng.normal4(v); else rng.uniform4(v);
            f(base + it * 256, v);
        }
    }
}

// (sum, sumsq) of one whole group of four values, as the 16-byte store paths reduce them
__device__ __forceinline__ void group_stats(const float (&v)[4], double& s, double& q) {
    const float ps = (v[0] + v[1]) + (v[2] + v[3]);
    const float pq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], v[3] * v[3])));
    s += (double)ps;
    q += (double)pq;
}

// store 4 values at local index e with range / alignment handling; returns how many were in range
template <bool VEC>
__device__ __forceinline__ void store_group(float* out, int64_t n, int64_t e, const float (&v)[4], double& s, double& q, bool stats) {
    if (VEC && e >= 0 && e + 4 <= n) {
        *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
        if (stats) group_stats(v, s, q);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e + k >= 0 && e + k < n) {
                out[e + k] = v[k];
                if (stats) {
                    s += (double)v[k];
                    q += (double)v[k] * (double)v[k];
                }
            }
        }
    }
}

// Accumulating epilogue of the generators: instead of writing a fresh tensor that a chain then folds into its running sum with
// sonar_axpby_f32 (read 8N, write 4N), the generator reads the sum and writes it back: v <- y * ya + v * f with the products
// rounded on their own and skipped when the multiplier is exactly 1, as AxpbyOp does (elementwise.hip), so the chain's value does
// not change by a bit.  y == nullptr: plain store.  y may be the output itself (in place).
struct Accum {
    const float* y;
    float ya, f;
    __device__ __forceinline__ float operator()(float yv, float v) const {
        const float yy = ya != 1.0f ? yv * ya : yv;
        const float xx = f != 1.0f ? v * f : v;
        return yy + xx;
    }
};
template <bool VEC>
__device__ __forceinline__ void accumulate_group(const Accum& acc, int64_t n, int64_t e, float (&v)[4]) {
    if (!acc.y) return;
    if (VEC && e >= 0 && e + 4 <= n) {
        const float4 y = *reinterpret_cast<const float4*>(acc.y + e);
        v[0] = acc(y.x, v[0]);
        v[1] = acc(y.y, v[1]);
        v[2] = acc(y.z, v[2]);
        v[3] = acc(y.w, v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k >= 0 && e + k < n) v[k] = acc(acc.y[e + k], v[k]);
    }
}
static constexpr Accum kNoAccum{nullptr, 1.0f, 1.0f};

// A tile-keyed generator's fold y <- y * ya + x * f riding in ANOTHER generator's pass over y (sonar_fold_prefix): the chain's previous
// item (Gaussian draw or Perlin) is evaluated on the fly and applied BEFORE the hosting kernel's own fold, so its read + write of the
// running sum disappears.  Same stream keys, same operations in the same order as its own kernel -> the same bits.  fresh: that item
// is the chain's first, the sum holds nothing yet: y1 = x, no read at all.
struct Prefix {
    float ya, f, div_fac;
    uint64_t seed, stream_id;
    const float* terms;
    int chw;
    int fresh;
};
// kind: 0 none, 1 Gaussian draw, 2 Perlin (summed lattice).  One group of four values: x drawn by the caller's copy of the prefix's
// generator (`rng`, advanced here), `term` the lattice vector of these four elements (Perlin).
template <int PRE, typename DIV>
__device__ __forceinline__ void prefix_draw(TileRng& rng, const DIV& div, const float4& term, float (&x)[4]) {
    if constexpr (PRE == 1) {
        rng.normal4(x);
    } else {
        uint32_t r[4];
        rng.words4_high(r);
        x[0] = div.from_word(r[0], term.x); x[1] = div.from_word(r[1], term.y);
        x[2] = div.from_word(r[2], term.z); x[3] = div.from_word(r[3], term.w);
    }
}
// v <- fold(y1, v) with y1 = x (fresh) or y * ya + x * f, y read from the running sum
__device__ __forceinline__ void prefix_fold(const Prefix& pre, const Accum& pfold, const Accum& fold, int64_t e, const float (&x)[4], float (&v)[4]) {
    if (pre.fresh) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fold(x[k], v[k]);
    } else {
        const float4 y = *reinterpret_cast<const float4*>(fold.y + e);
        v[0] = fold(pfold(y.x, x[0]), v[0]);
        v[1] = fold(pfold(y.y, x[1]), v[1]);
        v[2] = fold(pfold(y.z, x[2]), v[2]);
        v[3] = fold(pfold(y.w, x[3]), v[3]);
    }
}
static int make_prefix(const sonar_fold_prefix* pre, Prefix& px, const char* what) {
    SONAR_REQUIRE(pre->kind == SONAR_PREFIX_NORMAL || pre->kind == SONAR_PREFIX_PERLIN, SONAR_ERR_ARG, "%s: unknown prefix kind", what);
    const bool perlin = pre->kind == SONAR_PREFIX_PERLIN;
    SONAR_REQUIRE(!perlin || (pre->terms && pre->chw > 0 && pre->chw < (1LL << 31) && (reinterpret_cast<uintptr_t>(pre->terms) & 15u) == 0),
                  SONAR_ERR_ARG, "%s: a Perlin prefix needs its 16-byte aligned lattice", what);
    SONAR_REQUIRE(!pre->fresh || pre->x_mul == 1.0f, SONAR_ERR_ARG, "%s: a fresh prefix is the first item's raw values (x_mul 1)", what);
    px = Prefix{pre->y_mul, pre->x_mul, perlin ? pre->div_fac : 1.0f, pre->seed, pre->stream_id, pre->terms, perlin ? (int)pre->chw : 1,
                pre->fresh ? 1 : 0};
    return SONAR_OK;
}

struct Affine {
    float sub, mul, add;
    int active;
    __device__ __forceinline__ float operator()(float u) const { return active ? (u - sub) * mul + add : u; }
};

// the affine map and the normalisation with their run-time switches decided ONCE per launch (template flags): inside the tile loop every
// switch was a v_cndmask per value, and the range checks of a shard's ragged ends a branch per group -- 220 instructions per step of
// eight values where the arithmetic needs 90 (the launch was instruction-bound: 33 us against the 24 us of its stores)
template <bool ACTIVE>
struct AffineT {
    float sub, mul, add;
    __device__ __forceinline__ float operator()(float u) const {
        if constexpr (ACTIVE) return (u - sub) * mul + add;
        else return u;
    }
};
template <bool SUB, bool SCALE>
struct NormT {
    float mean, inv_std, factor;
    __device__ __forceinline__ float operator()(float v) const {
        if constexpr (SUB) v = v - mean;
        if constexpr (SCALE) v = v * inv_std * factor;
        return v;
    }
};

// scale_noise_kernel's own sequence (subtract, IEEE division; factor 1): what the one-pass N(0,1) route applies when a threshold fails
template <bool SUB, bool DIV>
struct NormExactT {
    float mean, stdv;
    __device__ __forceinline__ float operator()(float v) const {
        if constexpr (SUB) v = v - mean;
        if constexpr (DIV) v = v / stdv;
        return v;
    }
};
template <typename F>
__device__ __forceinline__ void with_exact_norm(const NormDecision& d, F&& f) {
    if (d.do_sub) {
        if (d.do_div) f(NormExactT<true, true>{d.mean, d.stdv});
        else f(NormExactT<true, false>{d.mean, d.stdv});
    } else {
        if (d.do_div) f(NormExactT<false, true>{d.mean, d.stdv});
        else f(NormExactT<false, false>{d.mean, d.stdv});
    }
}
template <typename F>
__device__ __forceinline__ void with_norm_flags(const NormFast& nf, F&& f) {
    if (nf.do_sub) {
        if (nf.do_scale) f(NormT<true, true>{nf.mean, nf.inv_std, nf.factor});
        else f(NormT<true, false>{nf.mean, nf.inv_std, nf.factor});
    } else {
        if (nf.do_scale) f(NormT<false, true>{nf.mean, nf.inv_std, nf.factor});
        else f(NormT<false, false>{nf.mean, nf.inv_std, nf.factor});
    }
}
template <typename F>
__device__ __forceinline__ void with_affine_norm(const Affine& aff, const NormFast& nf, F&& f) {
    auto with_norm = [&](auto a) { with_norm_flags(nf, [&](auto n) { f(a, n); }); };
    if (aff.active) with_norm(AffineT<true>{aff.sub, aff.mul, aff.add});
    else with_norm(AffineT<false>{aff.sub, aff.mul, aff.add});
}

static inline int tile_grid(int64_t n, int64_t elem_offset) {
    const int64_t tiles = (elem_offset + n - 1) / kTileElems - elem_offset / kTileElems + 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(kNPart, (tiles + 3) / 4));  // 4 waves (tiles) per block
}

// Generate mode: the lattice angles are drawn where they are used.  angle(iteration, c, gy, gx) = 2 pi u with u a
// counter-based uniform (Philox4x32-10, counter = (lattice point, iteration group), key = seed; word `it % 4`), so the four
// corners of a cell are random-access and a neighbouring cell recomputes the same values.  Writes the SUM over iterations
// of the cell-centre terms: one launch instead of angle fill + terms + pre-add.
// block `bid` of `nb` blocks of the lattice's work (perlin_lattice_kernel: the whole grid; perlin_ahead_kernel and pyramid_plane_kernel:
// their leading blocks)
template <int BLOCK = kBlock>
__device__ __forceinline__ void perlin_lattice_cells(float* terms_sum, int iters, int64_t C, int H, int W, int blend_mode, uint64_t seed,
                                                     uint64_t stream_id, int64_t bid, int64_t nb) {
    const int64_t total = C * H * W;
    const int gw = W + 1;
    for (int64_t i = bid * BLOCK + threadIdx.x; i < total; i += nb * BLOCK) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int64_t c = i / ((int64_t)W * H);
        const int64_t p00 = (c * (H + 1) + y) * gw + x;  // lattice point index of the top-left corner
        float acc = 0.0f;
        for (int g = 0; g < iters; g += 4) {
            auto words = [&](int64_t pt) { return philox4x32_10((uint32_t)pt, (uint32_t)(pt >> 32), (uint32_t)(g >> 2), (uint32_t)stream_id,
                                                                (uint32_t)seed, (uint32_t)(seed >> 32)); };
            const Philox4 w00 = words(p00), w01 = words(p00 + 1), w10 = words(p00 + gw), w11 = words(p00 + gw + 1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // fully unrolled: the word index must be a compile-time constant (registers, not LDS)
                if (g + k >= iters) break;
                // v_sin / v_cos take revolutions: the angle 2 pi u is never formed
                const float u00 = u01(w00.v[k]), u01_ = u01(w01.v[k]), u10 = u01(w10.v[k]), u11 = u01(w11.v[k]);
                const float d0 = __builtin_amdgcn_cosf(u00) * 0.5f + __builtin_amdgcn_sinf(u00) * 0.5f;
                const float d1 = __builtin_amdgcn_cosf(u01_) * -0.5f + __builtin_amdgcn_sinf(u01_) * 0.5f;
                const float d2 = __builtin_amdgcn_cosf(u10) * 0.5f + __builtin_amdgcn_sinf(u10) * -0.5f;
                const float d3 = __builtin_amdgcn_cosf(u11) * -0.5f + __builtin_amdgcn_sinf(u11) * -0.5f;
                const float row0 = blend<float>(blend_mode, d0, d1, 0.5f);
                const float row1 = blend<float>(blend_mode, d2, d3, 0.5f);
                acc += blend<float>(blend_mode, row0, row1, 0.5f);
            }
        }
        terms_sum[i] = acc;
    }
}

// accumulating forms: y <- y * y_mul + x * x_mul with x the generator's values (never stored), partials (nullable) <- statistics of y
static bool accum_ok(const sonar_accumulate* a) { return a && a->y; }

// noise_fill.hip (pair_fold_kernel); sonar_perlin_generate_chain_f32 launches it from noise_perlin.hip.  Hidden: the library's dynamic
// symbols that carry a sonar_ name (here through the argument types) stay the C ABI's.
__attribute__((visibility("hidden"))) int launch_pair_fold(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int host_kind, const Prefix& host, int64_t n,
                     int64_t elem_offset, hipStream_t st, const char* what);

}  // namespace sonar
