// Brownian-interval noise: the burst kernel (multiply-with-carry bursts per node, optionally hosting a chain's previous item) and the
// plain Philox kernel, one launcher for the point, bridge, accumulating and chain entry points.
#include "noise_stream.h"

namespace sonar {

// ------------------------------------------------------------------------------------------------
// Brownian-interval noise (the reference wraps ComfyUI's BrownianTreeNoiseSampler -> torchsde, un-vendored:
// py/noise_generation.py:262-286, py/nodes/powernoise.py:383-393).  One Brownian path per element over [t_lo, t_hi], defined
// point by point as the sampler asks for times (torchsde's BrownianInterval grows its tree the same way): a new time t between
// the nearest known times a < t < b is the Brownian bridge
//   W(t) = ((b - t) W(a) + (t - a) W(b)) / (b - a) + sqrt((t - a)(b - t) / (b - a)) z(node_t),
// z(node, element) a counter-based N(0,1) keyed by (seed, node id, global element index).  So every W(t) is a LINEAR combination
// of node normals (the host keeps the coefficients in fp64) and can be evaluated two ways with the same value up to fp32
// rounding: from the cached tensors W(a), W(b) plus ONE fresh normal per element (`base_a` / `base_b` below: the sampler's
// case, a step starts where the last one ended), or from its expansion out[e] = sum_k coef[k] * z(node[k], e).  Values depend on
// (seed, node, global element index) only: repeated / nested / abutting intervals are consistent, batches shard bit-identically.
constexpr int kMaxBrownianNodes = 96;
struct BrownianTerms {
    unsigned long long node[kMaxBrownianNodes];
    float coef[kMaxBrownianNodes];
    int count;
};

// Burst variant (latents of a multiple of kTileElems elements, one seed): a wave owns a sub-tile of 4 steps x 64 lanes x 4 = 1024
// elements and keeps its 4 x 4 partial sums in registers over the nodes; z(node, .) on the sub-tile is a multiply-with-carry burst
// (common.h, Mwc) of 12 words per lane.
// Round 6 (the virtual Brownian tree made a call 25 of these bursts per element, 354 us on cfg5's shard -- 22 ns of SIMD time per
// wave-normal, a fifth of it the Philox block that seeded every (node, sub-tile, lane) burst):
//  * ONE Philox block per (sub-tile, lane) and call -- the sub-tile's base state, keyed by (seed, kBrownStream, sub-tile, lane) -- and per
//    node a burst seeded by hashing the base with the node: x = fmix32(base.x ^ hx(node)), c = fmix32(base.c ^ hc(node)), where
//    (hx, hc) = splitmix64(node id) comes from the host and fmix32 is MurmurHash3's 32-bit finaliser (full avalanche: bursts of different
//    nodes start at unrelated points of the generator's one cycle, as Philox-seeded ones do): 16 instructions instead of ~60;
//  * the conversions of the power-law draw (common.h): 23 radius bits through the mantissa of a float in [1, 2), 16 angle bits per value
//    as a fraction of a revolution, one angle word for two Box-Muller pairs: 12 words and 20 conversion instructions per 16 normals
//    instead of 16 and 56;
//  * the coefficient rides under the radius' square root (c r = sqrt(-2 ln2 c^2 log2 u)) and its sign on the accumulating FMA's operand:
//    one multiply per pair instead of three.
// 230 -> ~150 instructions per node and sub-tile.  Every Brownian value changed with it (they were never pinned: torchsde is absent).
constexpr int kBrownIters = 4;
constexpr int kBrownTile = kBrownIters * 256;
// eight waves per workgroup where the expansion is long: a launch that reduces statistics has at most kNPart workgroups (one partial
// slot each), and with four waves each that left a compute-bound kernel at four waves per SIMD where it has the registers for eight
// (tree call on cfg5's shard 264 -> 244 us); the bridge route (one term, HBM-bound) keeps four (89 us; 101 with eight)
constexpr int kBrownBlock = 512;
constexpr int kBrownLongTerms = 4;
constexpr uint64_t kBrownStream = 0xB0B000000001ull;  // the base states' stream id (48 bits; node ids no longer are stream ids)
struct BrownianBurstTerms {
    uint32_t hx[kMaxBrownianNodes], hc[kMaxBrownianNodes];
    float coef[kMaxBrownianNodes];
    int count;
};
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
// acc[it][j] += c z(node)[4 it + j] for the sub-tile's 16 values of one lane: w = -2 ln2 c^2, NEG = (c < 0)
template <bool NEG>
__device__ __forceinline__ void brownian_burst_add(Mwc rng, float w, float (&acc)[kBrownIters][4]) {
#pragma unroll
    for (int it = 0; it < kBrownIters; ++it) {
        const uint32_t ra = rng.next(), rb = rng.next(), t = rng.next();
        float r0 = __builtin_amdgcn_sqrtf(w * __builtin_amdgcn_logf(2.0f - unit_mantissa(ra)));
        float r1 = __builtin_amdgcn_sqrtf(w * __builtin_amdgcn_logf(2.0f - unit_mantissa(rb)));
        if constexpr (NEG) {
            r0 = -r0;  // (folds into the FMAs as an operand modifier)
            r1 = -r1;
        }
        const float a0 = angle_lo(t), a1 = angle_hi(t);
        acc[it][0] = __builtin_fmaf(r0, __builtin_amdgcn_cosf(a0), acc[it][0]);
        acc[it][1] = __builtin_fmaf(r0, __builtin_amdgcn_sinf(a0), acc[it][1]);
        acc[it][2] = __builtin_fmaf(r1, __builtin_amdgcn_cosf(a1), acc[it][2]);
        acc[it][3] = __builtin_fmaf(r1, __builtin_amdgcn_sinf(a1), acc[it][3]);
    }
}
// Both kernels: acc = fa base_a + fb base_b + sum_k coef_k z(node_k) (either base may be null); out = scale * (acc - prev) (prev
// may be null), w_out = acc (may be null) -- ONE path point W(t), differenced against a cached W(t') (sonar_brownian_point_f32 /
// sonar_brownian_bridge_f32).  No __restrict__ on the inputs: prev is usually one of the bases.
struct BrownianBase {
    const float* a;
    const float* b;
    float fa, fb;
};
// PRE: 0 none, 1 Gaussian draw, 2 Perlin (summed lattice, tile-aligned latents).  With a prefix a wave walks the kBrownPerTile
// consecutive Brownian tiles of one generator tile, carrying the prefix's generator state across them.
// VEC = false: some buffer is only 4-byte aligned (a view at an odd storage offset) -- four 4-byte accesses where the kernel would
// make one 16-byte one, the same arithmetic and statistics order: the value family is a function of the shape, never of an address.
constexpr int kBrownPerTile = kTileElems / (4 * 256);
template <bool VEC>
__device__ __forceinline__ float4 brown_ld4(const float* p) {
    if constexpr (VEC) return *reinterpret_cast<const float4*>(p);
    else return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void brown_st4(float* p, const float4& v) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(p) = v;
    } else {
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}
template <int PRE, int BLOCK, bool VEC = true>
__global__ void __launch_bounds__(BLOCK) brownian_burst_kernel(float* out, int64_t n, int64_t elem_offset, BrownianBurstTerms terms,
                                                                uint64_t seed, const float* prev, float* w_out, float scale,
                                                                BrownianBase base, Accum fold, double* partials, Prefix pre) {
    static_assert(VEC || PRE == 0, "a hosted prefix reads the running sum 16 bytes at a time");
    kernarg_touch_for(out, n, elem_offset, terms, seed, prev, w_out, scale, base, fold, partials, pre);
    __shared__ double red[2 * BLOCK / 64];
    double s = 0.0, q = 0.0;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * BLOCK) >> 6;
    const int64_t first = elem_offset / kBrownTile, tiles = n / kBrownTile;  // both aligned (launcher)
    constexpr int SUB = PRE ? kBrownPerTile : 1;
    const Accum pfold{fold.y, pre.ya, pre.f};
    const Divider pdiv(PRE == 2 ? pre.div_fac : 1.0f);
    auto tiles_loop = [&](const auto& dv) {  // dv: a hosted Perlin item's word-to-value converter (with_divider: its kind decided once)
    for (int64_t T = wave; T < tiles / SUB; T += nwaves) {
        TileRng prng;
        const float4* trow = nullptr;
        if constexpr (PRE != 0) {
            prng = rng_stream(pre.seed, pre.stream_id, (uint64_t)(elem_offset / kTileElems + T), lane);
            // shards start on a latent boundary and latents are whole tiles (launcher): the tile's vectors sit at trow[64 * iteration]
            if constexpr (PRE == 2) trow = reinterpret_cast<const float4*>(pre.terms + (int)((T * kTileElems + (int64_t)lane * 4) % pre.chw));
        }
#pragma unroll 1
        for (int sub = 0; sub < SUB; ++sub) {
            const int64_t t = T * SUB + sub;
            float acc[kBrownIters][4];
            const int64_t o = t * kBrownTile + (int64_t)lane * 4;
#pragma unroll
            for (int it = 0; it < kBrownIters; ++it) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (base.a) {
                    const float4 p = brown_ld4<VEC>(base.a + o + it * 256);
                    v = make_float4(base.fa * p.x, base.fa * p.y, base.fa * p.z, base.fa * p.w);
                }
                if (base.b) {
                    const float4 p = brown_ld4<VEC>(base.b + o + it * 256);
                    v = make_float4(__builtin_fmaf(base.fb, p.x, v.x), __builtin_fmaf(base.fb, p.y, v.y), __builtin_fmaf(base.fb, p.z, v.z),
                                    __builtin_fmaf(base.fb, p.w, v.w));
                }
                acc[it][0] = v.x; acc[it][1] = v.y; acc[it][2] = v.z; acc[it][3] = v.w;
            }
            if (terms.count > 0) {
                const Mwc seedpoint = rng_stream(seed, kBrownStream, (uint64_t)(first + t), lane);
                for (int k = 0; k < terms.count; ++k) {
                    const Mwc rng = Mwc::seeded(fmix32(seedpoint.x ^ terms.hx[k]), fmix32(seedpoint.c ^ terms.hc[k]));
                    const float c = terms.coef[k];
                    const float w = -1.3862943611198906f * (c * c);
                    if (c < 0.0f) brownian_burst_add<true>(rng, w, acc);  // (uniform: a kernel argument)
                    else brownian_burst_add<false>(rng, w, acc);
                }
            }
#pragma unroll
            for (int it = 0; it < kBrownIters; ++it) {
                float4 a = make_float4(acc[it][0], acc[it][1], acc[it][2], acc[it][3]);
                if (w_out) brown_st4<VEC>(w_out + o + it * 256, a);
                if (out) {
                    if (prev) {
                        const float4 p = brown_ld4<VEC>(prev + o + it * 256);
                        a = make_float4(a.x - p.x, a.y - p.y, a.z - p.z, a.w - p.w);
                    }
                    float v[4] = {a.x * scale, a.y * scale, a.z * scale, a.w * scale};
                    if constexpr (PRE != 0) {
                        // the previous item's values for these four elements, folded into y first: y1 = y * ya + x * f (its own kernel's
                        // arithmetic), then this item's fold on y1
                        float x[4];
                        float4 tv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        if constexpr (PRE == 2) tv = trow[64 * (sub * kBrownIters + it)];
                        prefix_draw<PRE>(prng, dv, tv, x);
                        prefix_fold(pre, pfold, fold, o + it * 256, x, v);
                    } else {
                        accumulate_group<VEC>(fold, n, o + it * 256, v);  // (whole tiles: every element in range)
                    }
                    if constexpr (VEC) {
                        store_group<true>(out, n, o + it * 256, v, s, q, partials != nullptr);
                    } else {
                        brown_st4<false>(out + o + it * 256, make_float4(v[0], v[1], v[2], v[3]));
                        if (partials) group_stats(v, s, q);
                    }
                }
            }
        }
    }
    };
    if constexpr (PRE == 2) with_divider(pdiv, tiles_loop);
    else tiles_loop(pdiv);
    if (partials) write_partial<BLOCK>(s, q, partials, red);  // uniform branch (kernel argument)
}

__global__ void __launch_bounds__(kBlock) brownian_kernel(float* out, int64_t n, int64_t elem_offset, BrownianTerms terms,
                                                          uint64_t seed, const unsigned long long* __restrict__ latent_seeds,
                                                          int64_t latent_elems, const float* prev, float* w_out, float scale,
                                                          BrownianBase base, Accum fold, double* partials) {
    kernarg_touch_for(out, n, elem_offset, terms, seed, latent_seeds, latent_elems, prev, w_out, scale, base, fold, partials);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    // a thread owns one GLOBAL group of four elements (the counter of its draws): a shard whose first element is not a multiple of
    // four (odd latent sizes) starts and ends inside a group and keeps its part of it
    const int shift = latent_seeds ? 0 : (int)(elem_offset & 3);
    const int64_t groups = (n + shift + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t e = g * 4 - shift;               // local element index of the group's first element (< 0: before the shard)
        uint64_t key = seed;
        uint64_t ctr = (uint64_t)(elem_offset + e) >> 2;  // global 4-group
        if (latent_seeds) {                            // one seed per latent: counters restart inside each latent
            const int64_t lat = e / latent_elems;
            key = latent_seeds[lat];
            ctr = (uint64_t)(e - lat * latent_elems) >> 2;
        }
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < 4; ++j) {
            if (e + j < 0 || e + j >= n) continue;
            if (base.a) acc[j] = base.fa * base.a[e + j];
            if (base.b) acc[j] = __builtin_fmaf(base.fb, base.b[e + j], acc[j]);
        }
        for (int k = 0; k < terms.count; ++k) {
            const unsigned long long node = terms.node[k];
            const Philox4 p = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)node, (uint32_t)(node >> 32), (uint32_t)key,
                                            (uint32_t)(key >> 32));
            float z[4];
            box_muller(p.v[0], p.v[1], z[0], z[1]);
            box_muller(p.v[2], p.v[3], z[2], z[3]);
            const float c = terms.coef[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(c, z[j], acc[j]);
        }
        for (int j = 0; j < 4; ++j) {
            if (e + j < 0 || e + j >= n) continue;
            if (w_out) w_out[e + j] = acc[j];
            if (out) {
                float v = (prev ? acc[j] - prev[e + j] : acc[j]) * scale;
                if (fold.y) v = fold(fold.y[e + j], v);
                out[e + j] = v;
                s += (double)v;
                q += (double)v * (double)v;
            }
        }
    }
    if (partials) write_partial<kBlock>(s, q, partials, red);
}

}  // namespace sonar

using namespace sonar;

// ================================================================================================
static int brownian_launch(float* out, float* w_out, const float* prev, float scale, int64_t n, int64_t elem_offset,
                           const uint64_t* node_ids, const float* coefs, int nnodes, uint64_t seed, const uint64_t* latent_seeds,
                           int64_t latent_elems, void* stream, const char* what, BrownianBase base = BrownianBase{nullptr, nullptr, 0.0f, 0.0f},
                           Accum acc = kNoAccum, double* partials = nullptr, const sonar_fold_prefix* pre = nullptr) {
    SONAR_REQUIRE((out || w_out) && n >= 0 && elem_offset >= 0 && nnodes >= 0 && (nnodes == 0 || (node_ids && coefs)), SONAR_ERR_ARG,
                  "%s: bad argument", what);
    SONAR_REQUIRE(!latent_seeds || (elem_offset & 3) == 0, SONAR_ERR_ARG, "%s: per-latent seeds need an element offset of whole 4-element groups", what);
    SONAR_REQUIRE(nnodes <= kMaxBrownianNodes, SONAR_ERR_UNSUPPORTED, "%s: more than %d path nodes", what, kMaxBrownianNodes);
    SONAR_REQUIRE(!latent_seeds || (latent_elems > 0 && latent_elems % 4 == 0 && n % latent_elems == 0), SONAR_ERR_ARG,
                  "%s: per-latent seeds need whole latents of a multiple of 4 elements", what);
    for (int k = 0; k < nnodes; ++k) SONAR_REQUIRE((node_ids[k] >> 48) == 0, SONAR_ERR_ARG, "%s: node ids are 48-bit", what);
    if (n == 0) return SONAR_OK;
    BrownianTerms t;
    BrownianBurstTerms bt;
    t.count = bt.count = nnodes;
    for (int k = 0; k < nnodes; ++k) {
        t.node[k] = node_ids[k];
        t.coef[k] = bt.coef[k] = coefs[k];
        uint64_t h = node_ids[k] + 0x9E3779B97F4A7C15ull;  // splitmix64 of the node id
        h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
        h ^= h >> 31;
        bt.hx[k] = (uint32_t)h;
        bt.hc[k] = (uint32_t)(h >> 32);
    }
    auto al = [](const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    // the variant is a function of the latent size and the seed kind only, so every shard of a batch picks the same one; buffer
    // addresses choose only how the burst kernel accesses memory (a 4-byte-aligned buffer once switched the call to the Philox family:
    // other values for the same seed, node and element)
    const bool burst = !latent_seeds && latent_elems > 0 && latent_elems % kTileElems == 0 && n % latent_elems == 0 &&
                       elem_offset % latent_elems == 0;
    const bool vec = al(out) && al(w_out) && al(prev) && al(base.a) && al(base.b) && al(acc.y);
    SONAR_REQUIRE(!partials || out, SONAR_ERR_ARG, "%s: statistics need an output tensor", what);
    // statistics: one (sum, sumsq) pair per block, at most kNPart blocks
    const int cap = partials ? kNPart : kMaxGrid;
    Prefix px{1.0f, 1.0f, 1.0f, 0, 0, nullptr, 1, 0};
    if (pre) {
        // the previous chain item rides along only in the tile kernel, on the same running sum, with whole generator tiles per latent
        const int prc = make_prefix(pre, px, what);
        if (prc != SONAR_OK) return prc;
        SONAR_REQUIRE(burst && vec && acc.y && out == acc.y && (pre->kind != SONAR_PREFIX_PERLIN || pre->chw == latent_elems), SONAR_ERR_UNSUPPORTED,
                      "%s: this shape cannot host a fold prefix (apply it with its own entry point)", what);
    }
#define SONAR_BBL(P, BL, V) \
    hipLaunchKernelGGL((brownian_burst_kernel<P, BL, V>), dim3(std::min(cap, grid_for(n / (kBrownTile * (P ? kBrownPerTile : 1)), BL / 64))), dim3(BL), 0, \
                       (hipStream_t)stream, out, n, elem_offset, bt, seed, prev, w_out, scale, base, acc, partials, px)
#define SONAR_BB(P, V) \
    do { \
        if (nnodes >= kBrownLongTerms) SONAR_BBL(P, kBrownBlock, V); \
        else SONAR_BBL(P, kBlock, V); \
    } while (0)
    if (burst && pre && pre->kind == SONAR_PREFIX_NORMAL)
        SONAR_BB(1, true);
    else if (burst && pre)
        SONAR_BB(2, true);
    else if (burst && vec)
        SONAR_BB(0, true);
    else if (burst)
        SONAR_BB(0, false);
#undef SONAR_BBL
#undef SONAR_BB
    else
        hipLaunchKernelGGL(brownian_kernel, dim3(std::min(cap, grid_for((n + 6) / 4, kBlock))), dim3(kBlock), 0, (hipStream_t)stream, out, n,
                           elem_offset, t, seed, reinterpret_cast<const unsigned long long*>(latent_seeds), latent_elems, prev, w_out, scale,
                           base, acc, partials);
    return check_launch(what);
}

extern "C" int sonar_brownian_f32(float* out, int64_t n, int64_t elem_offset, const uint64_t* node_ids, const float* coefs,
                                  int nnodes, uint64_t seed, const uint64_t* latent_seeds, int64_t latent_elems, void* stream) {
    SONAR_REQUIRE(out, SONAR_ERR_ARG, "sonar_brownian_f32: bad argument");
    return brownian_launch(out, nullptr, nullptr, 1.0f, n, elem_offset, node_ids, coefs, nnodes, seed, latent_seeds, latent_elems, stream,
                           "sonar_brownian_f32");
}

extern "C" int sonar_brownian_point_f32(float* out, float* w_out, const float* prev, float scale, int64_t n, int64_t elem_offset,
                                        const uint64_t* node_ids, const float* coefs, int nnodes, uint64_t seed,
                                        const uint64_t* latent_seeds, int64_t latent_elems, void* stream) {
    return brownian_launch(out, w_out, prev, scale, n, elem_offset, node_ids, coefs, nnodes, seed, latent_seeds, latent_elems, stream,
                           "sonar_brownian_point_f32");
}

extern "C" int sonar_brownian_bridge_f32(float* out, float* w_out, const float* prev, float scale, const float* base_a, float fa,
                                         const float* base_b, float fb, int64_t n, int64_t elem_offset, const uint64_t* node_ids,
                                         const float* coefs, int nnodes, uint64_t seed, const uint64_t* latent_seeds,
                                         int64_t latent_elems, double* partials, void* stream) {
    return brownian_launch(out, w_out, prev, scale, n, elem_offset, node_ids, coefs, nnodes, seed, latent_seeds, latent_elems, stream,
                           "sonar_brownian_bridge_f32", BrownianBase{base_a, base_b, fa, fb}, kNoAccum, partials);
}

extern "C" int sonar_brownian_bridge_acc_f32(const sonar_accumulate* acc, float* w_out, const float* prev, float scale, const float* base_a,
                                             float fa, const float* base_b, float fb, int64_t n, int64_t elem_offset,
                                             const uint64_t* node_ids, const float* coefs, int nnodes, uint64_t seed,
                                             const uint64_t* latent_seeds, int64_t latent_elems, void* stream) {
    SONAR_REQUIRE(accum_ok(acc), SONAR_ERR_ARG, "sonar_brownian_bridge_acc_f32: bad argument");
    return brownian_launch(acc->y, w_out, prev, scale, n, elem_offset, node_ids, coefs, nnodes, seed, latent_seeds, latent_elems, stream,
                           "sonar_brownian_bridge_acc_f32", BrownianBase{base_a, base_b, fa, fb}, Accum{acc->y, acc->y_mul, acc->x_mul},
                           acc->partials);
}

extern "C" int sonar_brownian_bridge_chain_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, float* w_out, const float* prev,
                                               float scale, const float* base_a, float fa, const float* base_b, float fb, int64_t n,
                                               int64_t elem_offset, const uint64_t* node_ids, const float* coefs, int nnodes, uint64_t seed,
                                               int64_t latent_elems, void* stream) {
    SONAR_REQUIRE(accum_ok(acc) && pre, SONAR_ERR_ARG, "sonar_brownian_bridge_chain_f32: bad argument");
    return brownian_launch(acc->y, w_out, prev, scale, n, elem_offset, node_ids, coefs, nnodes, seed, nullptr, latent_elems, stream,
                           "sonar_brownian_bridge_chain_f32", BrownianBase{base_a, base_b, fa, fb}, Accum{acc->y, acc->y_mul, acc->x_mul},
                           acc->partials, pre);
}
