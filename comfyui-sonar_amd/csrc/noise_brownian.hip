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
// One burst step (3 words -> 4 normals of one node) in the two halves a coefficient splits it into: the draw itself -- the radii's
// logarithms and the angles' cosines / sines, the same for every path point the node belongs to -- and the coefficient's share,
// acc[j] += c z[j] with w = -2 ln2 c^2, NEG = (c < 0).  The pair kernels draw once and apply the second half per point.
struct BurstDraw {
    float l0, l1, c0, s0, c1, s1;
};
__device__ __forceinline__ BurstDraw brownian_burst_draw(Mwc& rng) {
    const uint32_t ra = rng.next(), rb = rng.next(), t = rng.next();
    const float a0 = angle_lo(t), a1 = angle_hi(t);
    return BurstDraw{__builtin_amdgcn_logf(2.0f - unit_mantissa(ra)), __builtin_amdgcn_logf(2.0f - unit_mantissa(rb)),
                     __builtin_amdgcn_cosf(a0), __builtin_amdgcn_sinf(a0), __builtin_amdgcn_cosf(a1), __builtin_amdgcn_sinf(a1)};
}
template <bool NEG>
__device__ __forceinline__ void brownian_burst_fma(const BurstDraw& d, float w, float (&acc)[4]) {
    float r0 = __builtin_amdgcn_sqrtf(w * d.l0);
    float r1 = __builtin_amdgcn_sqrtf(w * d.l1);
    if constexpr (NEG) {
        r0 = -r0;  // (folds into the FMAs as an operand modifier)
        r1 = -r1;
    }
    acc[0] = __builtin_fmaf(r0, d.c0, acc[0]);
    acc[1] = __builtin_fmaf(r0, d.s0, acc[1]);
    acc[2] = __builtin_fmaf(r1, d.c1, acc[2]);
    acc[3] = __builtin_fmaf(r1, d.s1, acc[3]);
}
// acc[it][j] += c z(node)[4 it + j] for the sub-tile's 16 values of one lane
template <bool NEG>
__device__ __forceinline__ void brownian_burst_add(Mwc rng, float w, float (&acc)[kBrownIters][4]) {
#pragma unroll
    for (int it = 0; it < kBrownIters; ++it) {
        const BurstDraw d = brownian_burst_draw(rng);
        brownian_burst_fma<NEG>(d, w, acc[it]);
    }
}
// ... and for the two points of a pair query: P = 0 the node is not in that point's expansion, 1 / 2 its coefficient is >= 0 / < 0
template <int P1, int P2>
__device__ __forceinline__ void brownian_burst_add2(Mwc rng, float w1, float w2, float (&acc1)[kBrownIters][4], float (&acc2)[kBrownIters][4]) {
#pragma unroll
    for (int it = 0; it < kBrownIters; ++it) {
        const BurstDraw d = brownian_burst_draw(rng);
        if constexpr (P1 != 0) brownian_burst_fma<P1 == 2>(d, w1, acc1[it]);
        if constexpr (P2 != 0) brownian_burst_fma<P2 == 2>(d, w2, acc2[it]);
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
// acc = fa base_a + fb base_b for one lane's 16 values of the sub-tile at local element o (either base may be null)
template <bool VEC>
__device__ __forceinline__ void brown_base_init(const BrownianBase& base, int64_t o, float (&acc)[kBrownIters][4]) {
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
            brown_base_init<VEC>(base, o, acc);
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

// Two points W_1, W_2 of the same path from one launch (sonar_brownian_pair_f32): the launcher merges the two points' expansions by node
// id, a wave draws each node's burst ONCE and adds its share to the accumulators of the points that hold the node, each with that point's
// own coefficient.  A point's accumulator sees its base and then its own nodes in ascending id order -- exactly the single-point kernel's
// operation sequence, so W_i, the increments and their statistics are that kernel's bits (same grid, same block size, same slot per block).
// out_i = scale_i (W_i - prev): both increments are differenced against the same kept W, read once.
constexpr unsigned char kPairIn1 = 1, kPairIn2 = 2;
struct BrownianPairBurstTerms {
    uint32_t hx[kMaxBrownianNodes], hc[kMaxBrownianNodes];
    float coef1[kMaxBrownianNodes], coef2[kMaxBrownianNodes];
    unsigned char in[kMaxBrownianNodes];  // kPairIn1 | kPairIn2
    int count;
};
struct BrownianPairTerms {
    unsigned long long node[kMaxBrownianNodes];
    float coef1[kMaxBrownianNodes], coef2[kMaxBrownianNodes];
    unsigned char in[kMaxBrownianNodes];
    int count;
};
template <int BLOCK, bool VEC>
__global__ void __launch_bounds__(BLOCK) brownian_pair_burst_kernel(float* out1, float* out2, int64_t n, int64_t elem_offset,
                                                                     BrownianPairBurstTerms terms, uint64_t seed, const float* prev,
                                                                     float* w_out1, float* w_out2, float scale1, float scale2,
                                                                     BrownianBase base1, BrownianBase base2, double* partials1,
                                                                     double* partials2) {
    kernarg_touch_for(out1, out2, n, elem_offset, terms, seed, prev, w_out1, w_out2, scale1, scale2, base1, base2, partials1, partials2);
    __shared__ double red1[2 * BLOCK / 64], red2[2 * BLOCK / 64];
    double s1 = 0.0, q1 = 0.0, s2 = 0.0, q2 = 0.0;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * BLOCK) >> 6;
    const int64_t first = elem_offset / kBrownTile, tiles = n / kBrownTile;  // both aligned (launcher)
    for (int64_t t = wave; t < tiles; t += nwaves) {
        float acc1[kBrownIters][4], acc2[kBrownIters][4];
        const int64_t o = t * kBrownTile + (int64_t)lane * 4;
        brown_base_init<VEC>(base1, o, acc1);
        brown_base_init<VEC>(base2, o, acc2);
        if (terms.count > 0) {
            const Mwc seedpoint = rng_stream(seed, kBrownStream, (uint64_t)(first + t), lane);
            for (int k = 0; k < terms.count; ++k) {
                const Mwc rng = Mwc::seeded(fmix32(seedpoint.x ^ terms.hx[k]), fmix32(seedpoint.c ^ terms.hc[k]));
                const float c1 = terms.coef1[k], c2 = terms.coef2[k];
                const float w1 = -1.3862943611198906f * (c1 * c1), w2 = -1.3862943611198906f * (c2 * c2);
                const int in = terms.in[k];
                // (uniform: kernel arguments) 0 absent, 1 coefficient >= 0, 2 coefficient < 0
                const int p1 = (in & kPairIn1) ? (c1 < 0.0f ? 2 : 1) : 0, p2 = (in & kPairIn2) ? (c2 < 0.0f ? 2 : 1) : 0;
                switch (p1 * 3 + p2) {
#define SONAR_PAIR_CASE(A, B) \
    case A * 3 + B: brownian_burst_add2<A, B>(rng, w1, w2, acc1, acc2); break;
                    SONAR_PAIR_CASE(0, 1) SONAR_PAIR_CASE(0, 2) SONAR_PAIR_CASE(1, 0) SONAR_PAIR_CASE(1, 1)
                    SONAR_PAIR_CASE(1, 2) SONAR_PAIR_CASE(2, 0) SONAR_PAIR_CASE(2, 1) SONAR_PAIR_CASE(2, 2)
#undef SONAR_PAIR_CASE
                    default: break;
                }
            }
        }
#pragma unroll
        for (int it = 0; it < kBrownIters; ++it) {
            const int64_t e = o + it * 256;
            float4 a1 = make_float4(acc1[it][0], acc1[it][1], acc1[it][2], acc1[it][3]);
            float4 a2 = make_float4(acc2[it][0], acc2[it][1], acc2[it][2], acc2[it][3]);
            if (w_out1) brown_st4<VEC>(w_out1 + e, a1);
            if (w_out2) brown_st4<VEC>(w_out2 + e, a2);
            if (prev) {
                const float4 p = brown_ld4<VEC>(prev + e);
                a1 = make_float4(a1.x - p.x, a1.y - p.y, a1.z - p.z, a1.w - p.w);
                a2 = make_float4(a2.x - p.x, a2.y - p.y, a2.z - p.z, a2.w - p.w);
            }
            const float v1[4] = {a1.x * scale1, a1.y * scale1, a1.z * scale1, a1.w * scale1};
            const float v2[4] = {a2.x * scale2, a2.y * scale2, a2.z * scale2, a2.w * scale2};
            brown_st4<VEC>(out1 + e, make_float4(v1[0], v1[1], v1[2], v1[3]));  // (whole tiles: every element in range)
            brown_st4<VEC>(out2 + e, make_float4(v2[0], v2[1], v2[2], v2[3]));
            if (partials1) group_stats(v1, s1, q1);
            if (partials2) group_stats(v2, s2, q2);
        }
    }
    if (partials1) write_partial<BLOCK>(s1, q1, partials1, red1);  // uniform branches (kernel arguments)
    if (partials2) write_partial<BLOCK>(s2, q2, partials2, red2);
}

// The plain Philox kernel's addressing and draw: a group's key and counter, and the four normals of (node, group)
__device__ __forceinline__ void brownian_group_key(int64_t e, int64_t elem_offset, uint64_t seed, const unsigned long long* latent_seeds,
                                                   int64_t latent_elems, uint64_t& key, uint64_t& ctr) {
    key = seed;
    ctr = (uint64_t)(elem_offset + e) >> 2;  // global 4-group
    if (latent_seeds) {                      // one seed per latent: counters restart inside each latent
        const int64_t lat = e / latent_elems;
        key = latent_seeds[lat];
        ctr = (uint64_t)(e - lat * latent_elems) >> 2;
    }
}
__device__ __forceinline__ void brownian_group_normals(uint64_t ctr, unsigned long long node, uint64_t key, float (&z)[4]) {
    const Philox4 p = philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)node, (uint32_t)(node >> 32), (uint32_t)key,
                                    (uint32_t)(key >> 32));
    box_muller(p.v[0], p.v[1], z[0], z[1]);
    box_muller(p.v[2], p.v[3], z[2], z[3]);
}

__global__ void __launch_bounds__(kBlock) brownian_pair_kernel(float* out1, float* out2, int64_t n, int64_t elem_offset, BrownianPairTerms terms,
                                                               uint64_t seed, const unsigned long long* __restrict__ latent_seeds,
                                                               int64_t latent_elems, const float* prev, float* w_out1, float* w_out2,
                                                               float scale1, float scale2, BrownianBase base1, BrownianBase base2,
                                                               double* partials1, double* partials2) {
    kernarg_touch_for(out1, out2, n, elem_offset, terms, seed, latent_seeds, latent_elems, prev, w_out1, w_out2, scale1, scale2, base1, base2,
                      partials1, partials2);
    __shared__ double red1[2 * kBlock / 64], red2[2 * kBlock / 64];
    double s1 = 0.0, q1 = 0.0, s2 = 0.0, q2 = 0.0;
    const int shift = latent_seeds ? 0 : (int)(elem_offset & 3);  // (brownian_kernel: a thread owns one GLOBAL group of four elements)
    const int64_t groups = (n + shift + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t e = g * 4 - shift;
        uint64_t key, ctr;
        brownian_group_key(e, elem_offset, seed, latent_seeds, latent_elems, key, ctr);
        float acc1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < 4; ++j) {
            if (e + j < 0 || e + j >= n) continue;
            if (base1.a) acc1[j] = base1.fa * base1.a[e + j];
            if (base1.b) acc1[j] = __builtin_fmaf(base1.fb, base1.b[e + j], acc1[j]);
            if (base2.a) acc2[j] = base2.fa * base2.a[e + j];
            if (base2.b) acc2[j] = __builtin_fmaf(base2.fb, base2.b[e + j], acc2[j]);
        }
        for (int k = 0; k < terms.count; ++k) {
            float z[4];
            brownian_group_normals(ctr, terms.node[k], key, z);
            const float c1 = terms.coef1[k], c2 = terms.coef2[k];
            const int in = terms.in[k];
            if (in & kPairIn1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc1[j] = __builtin_fmaf(c1, z[j], acc1[j]);
            }
            if (in & kPairIn2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc2[j] = __builtin_fmaf(c2, z[j], acc2[j]);
            }
        }
        for (int j = 0; j < 4; ++j) {
            if (e + j < 0 || e + j >= n) continue;
            if (w_out1) w_out1[e + j] = acc1[j];
            if (w_out2) w_out2[e + j] = acc2[j];
            const float p = prev ? prev[e + j] : 0.0f;
            const float v1 = (prev ? acc1[j] - p : acc1[j]) * scale1, v2 = (prev ? acc2[j] - p : acc2[j]) * scale2;
            out1[e + j] = v1;
            out2[e + j] = v2;
            s1 += (double)v1;
            q1 += (double)v1 * (double)v1;
            s2 += (double)v2;
            q2 += (double)v2 * (double)v2;
        }
    }
    if (partials1) write_partial<kBlock>(s1, q1, partials1, red1);
    if (partials2) write_partial<kBlock>(s2, q2, partials2, red2);
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
        uint64_t key, ctr;
        brownian_group_key(e, elem_offset, seed, latent_seeds, latent_elems, key, ctr);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < 4; ++j) {
            if (e + j < 0 || e + j >= n) continue;
            if (base.a) acc[j] = base.fa * base.a[e + j];
            if (base.b) acc[j] = __builtin_fmaf(base.fb, base.b[e + j], acc[j]);
        }
        for (int k = 0; k < terms.count; ++k) {
            float z[4];
            brownian_group_normals(ctr, terms.node[k], key, z);
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
// (hx, hc) of the burst kernels: splitmix64 of the node id
static void brownian_node_hash(uint64_t node, uint32_t& hx, uint32_t& hc) {
    uint64_t h = node + 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    h ^= h >> 31;
    hx = (uint32_t)h;
    hc = (uint32_t)(h >> 32);
}

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
        brownian_node_hash(node_ids[k], bt.hx[k], bt.hc[k]);
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

// One sorted term list of the pair entry point: strictly ascending 48-bit node ids (the merge below and the single-point order rely on it)
static int pair_list_ok(const uint64_t* ids, const float* coefs, int count, const char* which) {
    SONAR_REQUIRE(count >= 0 && (count == 0 || (ids && coefs)), SONAR_ERR_ARG, "sonar_brownian_pair_f32: bad %s term list", which);
    for (int k = 0; k < count; ++k) {
        SONAR_REQUIRE((ids[k] >> 48) == 0, SONAR_ERR_ARG, "sonar_brownian_pair_f32: node ids are 48-bit");
        SONAR_REQUIRE(k == 0 || ids[k - 1] < ids[k], SONAR_ERR_ARG, "sonar_brownian_pair_f32: the %s node ids must ascend", which);
    }
    return SONAR_OK;
}

extern "C" int sonar_brownian_pair_f32(float* out_1, float* out_2, float* w_out_1, float* w_out_2, const float* prev, float scale_1,
                                       float scale_2, const float* base_a_1, float fa_1, const float* base_b_1, float fb_1,
                                       const float* base_a_2, float fa_2, const float* base_b_2, float fb_2, int64_t n, int64_t elem_offset,
                                       const uint64_t* shared_ids, const float* shared_coefs, int nshared, const uint64_t* ids_1,
                                       const float* coefs_1, int n_1, const uint64_t* ids_2, const float* coefs_2, int n_2, uint64_t seed,
                                       const uint64_t* latent_seeds, int64_t latent_elems, double* partials_1, double* partials_2,
                                       void* stream) {
    const char* what = "sonar_brownian_pair_f32";
    SONAR_REQUIRE(out_1 && out_2, SONAR_ERR_ARG, "%s: both outputs are required", what);
    float* const outs[4] = {out_1, out_2, w_out_1, w_out_2};
    const float* const ins[5] = {prev, base_a_1, base_b_1, base_a_2, base_b_2};
    for (int i = 0; i < 4; ++i) {
        if (!outs[i]) continue;
        for (int j = i + 1; j < 4; ++j) SONAR_REQUIRE(outs[i] != outs[j], SONAR_ERR_ARG, "%s: two outputs share a buffer", what);
        for (int j = 0; j < 5; ++j) SONAR_REQUIRE(outs[i] != ins[j], SONAR_ERR_ARG, "%s: an output aliases a base or prev", what);
    }
    SONAR_REQUIRE(n >= 0 && n < (1LL << 31) && elem_offset >= 0, SONAR_ERR_ARG, "%s: 0 <= n < 2^31 elements, offset >= 0", what);
    for (int rc : {pair_list_ok(shared_ids, shared_coefs, nshared, "shared"), pair_list_ok(ids_1, coefs_1, n_1, "first point's"),
                   pair_list_ok(ids_2, coefs_2, n_2, "second point's")})
        if (rc != SONAR_OK) return rc;
    SONAR_REQUIRE((int64_t)nshared + n_1 + n_2 <= kMaxBrownianNodes, SONAR_ERR_UNSUPPORTED,
                  "%s: more than %d path nodes over the three lists (make two single-point queries)", what, kMaxBrownianNodes);
    SONAR_REQUIRE(!latent_seeds || (elem_offset & 3) == 0, SONAR_ERR_ARG, "%s: per-latent seeds need an element offset of whole 4-element groups", what);
    SONAR_REQUIRE(!latent_seeds || (latent_elems > 0 && latent_elems % 4 == 0 && n % latent_elems == 0), SONAR_ERR_ARG,
                  "%s: per-latent seeds need whole latents of a multiple of 4 elements", what);
    // the block size follows the single-point rule (kBrownLongTerms); a block owns one statistics slot, so the two points' statistics are the
    // single-point launches' bits only when that rule picks the same size for both
    const bool long_1 = nshared + n_1 >= kBrownLongTerms, long_2 = nshared + n_2 >= kBrownLongTerms;
    SONAR_REQUIRE(!(partials_1 || partials_2) || long_1 == long_2, SONAR_ERR_UNSUPPORTED,
                  "%s: statistics need both expansions on the same side of %d terms (make two single-point queries)", what, kBrownLongTerms);
    // merge by node id: a node of the shared list carries one coefficient for both points, a node on both private lists one for each
    BrownianPairTerms t;
    BrownianPairBurstTerms bt;
    int is = 0, i1 = 0, i2 = 0, count = 0;
    const uint64_t kEnd = ~0ull;
    while (is < nshared || i1 < n_1 || i2 < n_2) {
        const uint64_t ks = is < nshared ? shared_ids[is] : kEnd, k1 = i1 < n_1 ? ids_1[i1] : kEnd, k2 = i2 < n_2 ? ids_2[i2] : kEnd;
        const uint64_t node = std::min(ks, std::min(k1, k2));
        SONAR_REQUIRE(ks != node || (k1 != node && k2 != node), SONAR_ERR_ARG, "%s: a shared node is on a private list too", what);
        t.node[count] = node;
        t.coef1[count] = t.coef2[count] = 0.0f;
        t.in[count] = 0;
        if (ks == node) {
            t.coef1[count] = t.coef2[count] = shared_coefs[is++];
            t.in[count] = kPairIn1 | kPairIn2;
        }
        if (k1 == node) {
            t.coef1[count] = coefs_1[i1++];
            t.in[count] |= kPairIn1;
        }
        if (k2 == node) {
            t.coef2[count] = coefs_2[i2++];
            t.in[count] |= kPairIn2;
        }
        ++count;
    }
    if (n == 0) return SONAR_OK;
    t.count = bt.count = count;
    for (int k = 0; k < count; ++k) {
        bt.coef1[k] = t.coef1[k];
        bt.coef2[k] = t.coef2[k];
        bt.in[k] = t.in[k];
        brownian_node_hash(t.node[k], bt.hx[k], bt.hc[k]);
    }
    auto al = [](const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    // the routes of brownian_launch: the family from the shape and the seed kind, the access width from the addresses
    const bool burst = !latent_seeds && latent_elems > 0 && latent_elems % kTileElems == 0 && n % latent_elems == 0 &&
                       elem_offset % latent_elems == 0;
    bool vec = al(prev);
    for (float* p : outs) vec = vec && al(p);
    for (const float* p : ins) vec = vec && al(p);
    const int cap = (partials_1 || partials_2) ? kNPart : kMaxGrid;
    const BrownianBase b1{base_a_1, base_b_1, fa_1, fb_1}, b2{base_a_2, base_b_2, fa_2, fb_2};
#define SONAR_BPL(BL, V) \
    hipLaunchKernelGGL((brownian_pair_burst_kernel<BL, V>), dim3(std::min(cap, grid_for(n / kBrownTile, BL / 64))), dim3(BL), 0, (hipStream_t)stream, \
                       out_1, out_2, n, elem_offset, bt, seed, prev, w_out_1, w_out_2, scale_1, scale_2, b1, b2, partials_1, partials_2)
    if (burst && (long_1 || long_2)) {
        if (vec) SONAR_BPL(kBrownBlock, true);
        else SONAR_BPL(kBrownBlock, false);
    } else if (burst) {
        if (vec) SONAR_BPL(kBlock, true);
        else SONAR_BPL(kBlock, false);
    }
#undef SONAR_BPL
    else
        hipLaunchKernelGGL(brownian_pair_kernel, dim3(std::min(cap, grid_for((n + 6) / 4, kBlock))), dim3(kBlock), 0, (hipStream_t)stream, out_1,
                           out_2, n, elem_offset, t, seed, reinterpret_cast<const unsigned long long*>(latent_seeds), latent_elems, prev, w_out_1,
                           w_out_2, scale_1, scale_2, b1, b2, partials_1, partials_2);
    return check_launch(what);
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
