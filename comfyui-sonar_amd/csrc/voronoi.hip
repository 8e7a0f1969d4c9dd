// VoronoiNoiseGenerator.generate_octave (py/noise_generation.py:1847-1869): one octave is one launch, accumulated into the output.
//   voronoi_octave_kernel  one thread per pixel, a workgroup inside one (b, c) plane.  The plane's feature points pass through LDS
//                          SONAR_VORONOI_CHUNK at a time, already scaled and wrapped ((f * scale) % 1, the staging thread's work); every lane
//                          of a wave reads the same point, a broadcast.  Per point the toroidal difference d = (g - f + 0.5) % 1 - 0.5, the
//                          distance program on d and, per result term, a branch-free insertion into the four smallest distances (plus the
//                          index of the smallest and, for softmin, the online-softmax sums) -- registers only, every array below is indexed
//                          by an unrolled constant.  The epilogue evaluates the result terms and does out = out + result * amplitude (and
//                          the generator's final division after the last octave).
//   voronoi_rank_kernel    the rank route (sonar_voronoi_rank_octave_f32): the same pixel, staging and distance program, but any order
//                          statistic of the row -- the k-th smallest by a bit-by-bit search on the ordered-integer image of the floats,
//                          32 counting sweeps over the points -- and softmin:use_sorted on a row held in LDS.
// The grid, the two `% 1` and the wrap are the reference's fp32 operations one rounding each (__fmul_rn / __fadd_rn / __fdiv_rn and the
// library's -ffp-contract=off), so a difference lands on the side of the wrap where the reference's lands.  Square roots are sqrtf, the
// correctly rounded one (the __fsqrt_rn of this toolchain is the native instruction, 1 ulp).
#include "common.h"
#include "range_reduce.h"

namespace sonar {

namespace {

constexpr int kChunk = SONAR_VORONOI_CHUNK;
constexpr int kTerms = SONAR_VORONOI_MAX_TERMS;
constexpr int kChain = SONAR_VORONOI_MAX_CHAIN;
static_assert(kChunk == kBlock, "one staging thread per point of a chunk");

// torch.remainder(x, 1): fmod, then the divisor's sign
__device__ __forceinline__ float rem1(float x) {
    float r = fmodf(x, 1.0f);
    if (r != 0.0f && r < 0.0f) r = __fadd_rn(r, 1.0f);
    return r;
}

__device__ __forceinline__ float wrap_diff(float g, float f) { return __fsub_rn(rem1(__fadd_rn(__fsub_rn(g, f), 0.5f)), 0.5f); }

__device__ __forceinline__ float pick3(float a, float b, float c, int idx) { return idx == 0 ? a : idx == 1 ? b : c; }

// SIMPLE: no transforms (a compile-time fact of the kernel's plain instantiation)
template <bool SIMPLE>
__device__ __forceinline__ float distance_term(const sonar_voronoi_dterm& t, float d0, float d1, float d2) {
#pragma unroll
    for (int k = 0; k < (SIMPLE ? 0 : kChain); ++k) {
        if (k >= t.n_xform) break;
        const float a = t.xa[k], b = t.xb[k];
        if (t.xform[k] == SONAR_VORONOI_X_WEIGHT) {
            d0 = __fmul_rn(d0, a), d1 = __fmul_rn(d1, b), d2 = __fmul_rn(d2, t.xc[k]);
        } else if (t.xform[k] == SONAR_VORONOI_X_FRACTAL_SIN) {
            d0 = __fadd_rn(d0, __fmul_rn(a, sinf(__fmul_rn(d0, b))));
            d1 = __fadd_rn(d1, __fmul_rn(a, sinf(__fmul_rn(d1, b))));
            d2 = __fadd_rn(d2, __fmul_rn(a, sinf(__fmul_rn(d2, b))));
        } else {
            d0 = __fadd_rn(d0, __fmul_rn(a, cosf(__fmul_rn(d0, b))));
            d1 = __fadd_rn(d1, __fmul_rn(a, cosf(__fmul_rn(d1, b))));
            d2 = __fadd_rn(d2, __fmul_rn(a, cosf(__fmul_rn(d2, b))));
        }
    }
    float v;
    switch (t.metric) {
        case SONAR_VORONOI_D_CHEBYSHEV:
            v = fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fabsf(d2));
            break;
        case SONAR_VORONOI_D_MINKOWSKI:
            v = powf(__fadd_rn(__fadd_rn(powf(fabsf(d0), t.p), powf(fabsf(d1), t.p)), powf(fabsf(d2), t.p)), t.inv_p);
            break;
        default: {
            const float sq = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
            if (t.metric == SONAR_VORONOI_D_QUADRATIC) {
                v = sq;
            } else if (t.metric <= SONAR_VORONOI_D_MANHATTEN) {
                v = sqrtf(sq);
            } else {
                const float c = __fdiv_rn(pick3(d0, d1, d2, t.idx), fmaxf(sqrtf(sq), 1e-12f));  // F.normalize
                if (t.metric == SONAR_VORONOI_D_ANGLE) v = acosf(fminf(fmaxf(c, -1.0f), 1.0f));
                else if (t.metric == SONAR_VORONOI_D_ANGLE_TANH) v = acosf(tanhf(c));
                else v = acosf(__fsub_rn(__fmul_rn(__fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-c))), 2.0f), 1.0f));
            }
        }
    }
    return v;  // (the caller applies the term's scale)
}

// ---- the fuzz distance mode (py/noise_generation.py:1586-1603): three launches of the kernel below
struct FuzzArgs {
    const float* u;      // replay: the drawn uniforms [B][C][H][W][N]; NULL: the Philox stream element of the same flat index
    uint32_t* stats;     // ordered-integer images: [0] / [1] the inner distance's whole-tensor min / max, [2 + 2 r] / [3 + 2 r] row r = (b, c, y)
    double fuzz;
    int term;
    uint64_t seed, stream_id;
    int64_t elem_offset;
};
// floats as unsigned integers of the same order, for atomicMin / atomicMax
__device__ __forceinline__ uint32_t ordered(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float unordered(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? e ^ 0x80000000u : ~e); }
// elements e4 .. e4 + 3 (e4 a multiple of 4) of the flat uniform stream sonar_philox_uniform_f32 fills: tile e / kTileElems, burst step
// (e % kTileElems) / 256, lane (e % 256) / 4, slot e % 4 (common.h)
__device__ __forceinline__ void stream_uniform4(uint64_t seed, uint64_t stream_id, int64_t e4, float& u0, float& u1, float& u2, float& u3) {
    const int64_t tile = e4 / kTileElems;
    const int within = (int)(e4 - tile * kTileElems), it = within >> 8;
    TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, (uint32_t)((within & 255) >> 2));
    for (int k = 0; k < 4 * it; ++k) rng.next();
    u0 = u01(rng.next()), u1 = u01(rng.next()), u2 = u01(rng.next()), u3 = u01(rng.next());
}

// PASS: -1 no fuzz term; 0 reduces the fuzz term's inner distance over the whole tensor into stats[0..1]; 1 reduces the fuzzed distance
// per (b, c, y) row into the row slots; 2 is the real pass, the fuzzed distance rescaled between its row's extremes to the whole tensor's
// SIMPLE: one distance term without transforms and one result term without a fractal_norm (both presets' octaves): the chains' counts are
// compile-time facts and the program's few live fields stay in scalar registers
template <bool SIMPLE, int PASS>
__global__ void __launch_bounds__(kBlock) voronoi_octave_kernel(const float* __restrict__ fp, float* __restrict__ out, const float* __restrict__ aux,
                                                                int64_t planes, int H, int W, int N, float scale, float z_norm, float amplitude,
                                                                float final_div, int flags, sonar_voronoi_program prog, FuzzArgs fz) {
    __shared__ float pts[3 * kChunk];
    const int hw = H * W;
    const int tiles = (hw + kBlock - 1) / kBlock;
    const int64_t work = planes * tiles;
    const float gz = rem1(__fmul_rn(z_norm, scale));
    const int n_d = SIMPLE ? 1 : prog.n_d, n_r = SIMPLE ? 1 : prog.n_r;
    float gmin = 0.0f, gmax = 0.0f, span = 0.0f, fz1 = 0.0f, fz2 = 0.0f;  // the fuzz term: rmin, rmax, fp32(rmax - rmin), fuzz, 2 fuzz
    if constexpr (PASS >= 1) {
        gmin = unordered(fz.stats[0]), gmax = unordered(fz.stats[1]);
        const double f = fmax(fabs((double)gmin), fabs((double)gmax)) * fz.fuzz;  // max(abs(rmin.item()), abs(rmax.item())) * fuzz
        fz1 = (float)f, fz2 = (float)(f * 2.0);
        span = (float)((double)gmax - (double)gmin);
    }
    for (int64_t unit = blockIdx.x; unit < work; unit += gridDim.x) {  // (uniform: every thread reaches the barriers below)
        const int64_t plane = unit / tiles;
        const int pix = (int)(unit - plane * tiles) * kBlock + (int)threadIdx.x;
        const bool live = pix < hw;
        const int y = live ? pix / W : 0, x = live ? pix - y * W : 0;
        const float gy = rem1(__fmul_rn(__fdiv_rn((float)y, (float)H), scale));
        const float gx = rem1(__fmul_rn(__fdiv_rn((float)x, (float)W), scale));
        float m0[kTerms], m1[kTerms], m2[kTerms], m3[kTerms], smax[kTerms], ssum[kTerms], sacc[kTerms];
        int arg[kTerms];
#pragma unroll
        for (int t = 0; t < kTerms; ++t) {
            m0[t] = m1[t] = m2[t] = m3[t] = INFINITY;
            smax[t] = -INFINITY, ssum[t] = 0.0f, sacc[t] = 0.0f, arg[t] = 0;
        }
        const float* plane_pts = fp + plane * (int64_t)N * 3;
        float tmin = INFINITY, tmax = -INFINITY, rlo = 0.0f, rhi = 0.0f, u0 = 0.0f, u1 = 0.0f, u2 = 0.0f, u3 = 0.0f;
        int64_t have = -1;  // the group of four stream elements u0..u3 hold
        const int64_t row = plane * H + y, flat = (plane * hw + pix) * (int64_t)N;
        if constexpr (PASS == 2)
            if (live) rlo = unordered(fz.stats[2 + 2 * row]), rhi = unordered(fz.stats[3 + 2 * row]);
        for (int base = 0; base < N; base += kChunk) {
            const int cnt = N - base < kChunk ? N - base : kChunk;
            __syncthreads();  // the previous chunk has been read
            if ((int)threadIdx.x < cnt) {
                const float* p = plane_pts + (int64_t)(base + (int)threadIdx.x) * 3;
                pts[3 * threadIdx.x + 0] = rem1(__fmul_rn(p[0], scale));
                pts[3 * threadIdx.x + 1] = rem1(__fmul_rn(p[1], scale));
                pts[3 * threadIdx.x + 2] = rem1(__fmul_rn(p[2], scale));
            }
            __syncthreads();
            for (int j = 0; j < cnt; ++j) {
                const float d0 = wrap_diff(gy, pts[3 * j + 0]), d1 = wrap_diff(gx, pts[3 * j + 1]), d2 = wrap_diff(gz, pts[3 * j + 2]);
                float dist = 0.0f;
#pragma unroll
                for (int t = 0; t < (SIMPLE ? 1 : kTerms); ++t) {
                    if (t >= n_d) break;
                    float v = distance_term<SIMPLE>(prog.d[t], d0, d1, d2);
                    if constexpr (PASS >= 0) {
                        if (t == fz.term && live) {
                            if constexpr (PASS >= 1) {
                                float u;
                                if (fz.u != nullptr) {
                                    u = fz.u[flat + base + j];
                                } else {
                                    const int64_t e = fz.elem_offset + flat + base + j;
                                    if ((e >> 2) != have) have = e >> 2, stream_uniform4(fz.seed, fz.stream_id, e & ~(int64_t)3, u0, u1, u2, u3);
                                    const int slot = (int)(e & 3);
                                    u = slot == 0 ? u0 : slot == 1 ? u1 : slot == 2 ? u2 : u3;
                                }
                                v = __fadd_rn(v, __fsub_rn(__fmul_rn(u, fz2), fz1));
                            }
                            if constexpr (PASS <= 1) tmin = fminf(tmin, v), tmax = fmaxf(tmax, v);
                            else v = minmax_rescale_value(v, rlo, rhi, 1e-07f, gmin, gmax, span);
                        }
                    }
                    v = __fmul_rn(v, prog.d[t].scale);
                    dist = t == 0 ? v : __fadd_rn(dist, v);
                }
                if constexpr (PASS == 0 || PASS == 1) continue;  // the reducing passes need the fuzz term alone
#pragma unroll
                for (int t = 0; t < (SIMPLE ? 1 : kTerms); ++t) {
                    if (t >= n_r) break;
                    const sonar_voronoi_rterm& r = prog.r[t];
                    float e = dist;
#pragma unroll
                    for (int k = 0; k < (SIMPLE ? 0 : kChain); ++k) {
                        if (k >= r.n_fn) break;
                        const float a = __fmul_rn(e, r.fb[k]);
                        e = __fmul_rn(r.fa[k], r.fn[k] == SONAR_VORONOI_X_FRACTAL_SIN ? sinf(a) : cosf(a));
                    }
                    if (r.op == SONAR_VORONOI_R_SOFTMIN) {
                        const float norm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
                        const float logit = __fmul_rn(-norm, r.temperature);
                        const float top = fmaxf(smax[t], logit);
                        const float keep = expf(__fsub_rn(smax[t], top)), w = expf(__fsub_rn(logit, top));  // the first point: exp(-inf) = 0
                        ssum[t] = __fadd_rn(__fmul_rn(ssum[t], keep), w);
                        sacc[t] = __fadd_rn(__fmul_rn(sacc[t], keep), __fmul_rn(e, w));
                        smax[t] = top;
                    } else {  // the four smallest, ascending, and the first index of the smallest
                        m3[t] = fminf(m3[t], fmaxf(m2[t], e));
                        m2[t] = fminf(m2[t], fmaxf(m1[t], e));
                        m1[t] = fminf(m1[t], fmaxf(m0[t], e));
                        arg[t] = e < m0[t] ? base + j : arg[t];
                        m0[t] = fminf(m0[t], e);
                    }
                }
            }
        }
        if constexpr (PASS == 0 || PASS == 1) {
            // one atomic pair per wave where its lanes share the slot (always in pass 0; in pass 1 when the wave lies inside one row)
            const int64_t slot = PASS == 0 ? 0 : 1 + __shfl(row, 0);
            const bool mine = PASS == 0 || !live || row == slot - 1;
            if (__all(mine)) {
                tmin = wave_min(tmin), tmax = wave_max(tmax);  // a NaN never wins
                if ((threadIdx.x & 63) == 0 && tmin <= tmax) atomicMin(fz.stats + 2 * slot, ordered(tmin)), atomicMax(fz.stats + 2 * slot + 1, ordered(tmax));
            } else if (live && tmin <= tmax) {
                atomicMin(fz.stats + 2 + 2 * row, ordered(tmin)), atomicMax(fz.stats + 3 + 2 * row, ordered(tmax));
            }
            continue;
        }
        // The reference scales and sums the terms in place, and a bare f term is a VIEW of the sorted tensor the plain terms (no result
        // fractal_norm: that one sorts a tensor of its own) of an expression share: its `.mul_(scale)` lands in that column for every later
        // plain term, and a sum that starts with one keeps accumulating into the column (`alias`).  s0..s3 are that shared tensor.
        float result = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        bool shared = false;
        int alias = -1;
#pragma unroll
        for (int t = 0; t < (SIMPLE ? 1 : kTerms); ++t) {
            if (t >= n_r) break;
            const sonar_voronoi_rterm& r = prog.r[t];
            const bool plain = r.n_fn == 0;
            if (plain && !shared) s0 = m0[t], s1 = m1[t], s2 = m2[t], s3 = m3[t], shared = true;
            const float a0 = plain ? s0 : m0[t], a1 = plain ? s1 : m1[t], a2 = plain ? s2 : m2[t], a3 = plain ? s3 : m3[t];
            const float v1 = r.idx1 == 0 ? a0 : r.idx1 == 1 ? a1 : r.idx1 == 2 ? a2 : a3;
            const float v2 = r.idx2 == 0 ? a0 : r.idx2 == 1 ? a1 : r.idx2 == 2 ? a2 : a3;
            float v;
            switch (r.op) {
                case SONAR_VORONOI_R_F: v = v1; break;
                case SONAR_VORONOI_R_INV_F: v = __fdiv_rn(1.0f, __fadd_rn(v1, r.eps)); break;
                case SONAR_VORONOI_R_DIFF: v = __fsub_rn(v2, v1); break;
                case SONAR_VORONOI_R_DIFF2: v = __fdiv_rn(__fsub_rn(v2, v1), __fadd_rn(__fadd_rn(v2, v1), 1e-06f)); break;
                case SONAR_VORONOI_R_SOFTMIN: v = __fdiv_rn(sacc[t], ssum[t]); break;
                case SONAR_VORONOI_R_CELLID: v = __fadd_rn(__fdiv_rn((float)arg[t], aux[t]), 1.0f); break;
                default: v = (float)arg[t]; break;
            }
#pragma unroll
            for (int k = 0; k < kChain; ++k) {
                if (k >= r.n_ridge) break;
                v = __fsub_rn(1.0f, __fmul_rn(r.ridge[k], v));
            }
            v = __fmul_rn(v, r.scale);
            const bool view = !SIMPLE && plain && r.op == SONAR_VORONOI_R_F && r.n_ridge == 0;
            if (view) {
                if (alias == r.idx1) result = v;  // the running sum IS this column
                if (t == 0) alias = r.idx1;
            }
            result = t == 0 ? v : __fadd_rn(result, v);
            if (!SIMPLE) {
                const int col = t > 0 && alias >= 0 ? alias : view ? r.idx1 : -1;  // what the term's mul_ / the sum's add_ wrote through
                const float w = t > 0 && alias >= 0 ? result : v;
                if (view && col != r.idx1) s0 = r.idx1 == 0 ? v : s0, s1 = r.idx1 == 1 ? v : s1, s2 = r.idx1 == 2 ? v : s2, s3 = r.idx1 == 3 ? v : s3;
                s0 = col == 0 ? w : s0, s1 = col == 1 ? w : s1, s2 = col == 2 ? w : s2, s3 = col == 3 ? w : s3;
            }
        }
        if (live) {
            const int64_t at = plane * hw + pix;
            float o = __fadd_rn(out[at], __fmul_rn(result, amplitude));
            if (flags & SONAR_VORONOI_FINAL_DIV) o = __fdiv_rn(o, final_div);
            out[at] = o;
        }
    }
}

// ---- the rank route: order statistics anywhere in the sorted row (py/noise_generation.py:1606-1704)
constexpr int kRowLanes = 64;                       // the ROW instantiation's workgroup: one wave, its distance rows side by side in LDS
constexpr int kRowN = SONAR_VORONOI_RANK_ROW_N;     // the longest row softmin:use_sorted is built for
static_assert(kRowN <= kChunk, "the ROW instantiation reads every point of the plane from one staged chunk");
static_assert((3 * kChunk + kRowLanes * kRowN) * sizeof(float) <= 160 * 1024, "the staged points and a wave's rows fit the CU's LDS");

struct FuzzPixel {  // what voronoi_octave_kernel's pass 2 keeps per launch and per pixel
    float gmin = 0.0f, gmax = 0.0f, span = 0.0f, fz1 = 0.0f, fz2 = 0.0f, rlo = 0.0f, rhi = 0.0f;
};

// the distance expression of one point, voronoi_octave_kernel's own steps (PASS -1 without a fuzz term, PASS 2 with one)
template <bool FUZZ>
__device__ __forceinline__ float rank_distance(const sonar_voronoi_program& prog, int n_d, const FuzzArgs& fz, const FuzzPixel px, float& u0, float& u1,
                                               float& u2, float& u3, int64_t& have, float d0, float d1, float d2, int64_t elem, bool live) {
    float dist = 0.0f;
#pragma unroll
    for (int t = 0; t < kTerms; ++t) {
        if (t >= n_d) break;
        float v = distance_term<false>(prog.d[t], d0, d1, d2);
        if constexpr (FUZZ) {
            if (t == fz.term && live) {
                float u;
                if (fz.u != nullptr) {
                    u = fz.u[elem];
                } else {
                    const int64_t e = fz.elem_offset + elem;
                    if ((e >> 2) != have) have = e >> 2, stream_uniform4(fz.seed, fz.stream_id, e & ~(int64_t)3, u0, u1, u2, u3);
                    const float lo = (e & 1) ? u1 : u0, hi = (e & 1) ? u3 : u2;  // (two selects: a chain over the slot becomes an indexed array)
                    u = (e & 2) ? hi : lo;
                }
                v = __fadd_rn(v, __fsub_rn(__fmul_rn(u, px.fz2), px.fz1));
                v = minmax_rescale_value(v, px.rlo, px.rhi, 1e-07f, px.gmin, px.gmax, px.span);
            }
        }
        v = __fmul_rn(v, prog.d[t].scale);
        dist = t == 0 ? v : __fadd_rn(dist, v);
    }
    return dist;
}

// the result fractal_norm chain of term r on the distance
__device__ __forceinline__ float rank_value(const sonar_voronoi_rterm& r, float e) {
#pragma unroll
    for (int k = 0; k < kChain; ++k) {
        if (k >= r.n_fn) break;
        const float a = __fmul_rn(e, r.fb[k]);
        e = __fmul_rn(r.fa[k], r.fn[k] == SONAR_VORONOI_X_FRACTAL_SIN ? sinf(a) : cosf(a));
    }
    return e;
}

__device__ __forceinline__ float softmin_logit(float gy, float gx, float gz, const float* p, float temperature) {
    const float d0 = wrap_diff(gy, p[0]), d1 = wrap_diff(gx, p[1]), d2 = wrap_diff(gz, p[2]);
    return __fmul_rn(-sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2))), temperature);
}

// One thread per pixel as above, but the selection is exact for any rank: the k-th smallest value of a pixel's row is the largest v with
// #{e_j < v} <= k, found bit by bit on the ordered-integer image of the floats -- 32 sweeps over the points, each counting for both
// ranks of every term at once, registers only (tied values are equal, so ties need no rule).  A sweep before them (`stats`) keeps what
// the other ops need: softmin's online sums, the index of the smallest, the largest logit.  Terms do not share a sorted tensor here: an F
// term is a value (the median is one), and the host keeps sums that hold a bare f view of the reference on the top-four route.
// ROW (a workgroup of one wave, N <= kRowN): softmin:use_sorted pairs the weight of point j with the j-th smallest value, which is
// sum_i e_i w[rank(i)], rank(i) = #{j : e_j < e_i or (e_j == e_i and j < i)}.  The pixel's row of e lies in LDS lane-major (row[j * 64 +
// lane]: a wave's 64 lanes read 64 consecutive words), the weights are recomputed from the staged points.
template <bool ROW, bool FUZZ>
__global__ void __launch_bounds__(ROW ? kRowLanes : kBlock) voronoi_rank_kernel(const float* __restrict__ fp, float* __restrict__ out,
                                                                                const float* __restrict__ aux, int64_t planes, int H, int W, int N,
                                                                                float scale, float z_norm, float amplitude, float final_div,
                                                                                int flags, sonar_voronoi_program prog, FuzzArgs fz) {
    constexpr int BLOCK = ROW ? kRowLanes : kBlock;
    extern __shared__ float rank_lds[];
    float* pts = rank_lds;               // 3 * kChunk
    float* row = rank_lds + 3 * kChunk;  // ROW: kRowLanes * N
    const int hw = H * W;
    const int tiles = (hw + BLOCK - 1) / BLOCK;
    const int64_t work = planes * tiles;
    const float gz = rem1(__fmul_rn(z_norm, scale));
    const int n_d = prog.n_d, n_r = prog.n_r;
    bool stats = false, select = false;
#pragma unroll
    for (int t = 0; t < kTerms; ++t) {
        if (t >= n_r) break;
        if (prog.r[t].op <= SONAR_VORONOI_R_DIFF2) select = true;
        else stats = true;
    }
    FuzzPixel px;
    if constexpr (FUZZ) {
        px.gmin = unordered(fz.stats[0]), px.gmax = unordered(fz.stats[1]);
        const double f = fmax(fabs((double)px.gmin), fabs((double)px.gmax)) * fz.fuzz;
        px.fz1 = (float)f, px.fz2 = (float)(f * 2.0);
        px.span = (float)((double)px.gmax - (double)px.gmin);
    }
    for (int64_t unit = blockIdx.x; unit < work; unit += gridDim.x) {  // (uniform: every thread reaches the barriers below)
        const int64_t plane = unit / tiles;
        const int pix = (int)(unit - plane * tiles) * BLOCK + (int)threadIdx.x;
        const bool live = pix < hw;
        const int y = live ? pix / W : 0, x = live ? pix - y * W : 0;
        const float gy = rem1(__fmul_rn(__fdiv_rn((float)y, (float)H), scale));
        const float gx = rem1(__fmul_rn(__fdiv_rn((float)x, (float)W), scale));
        const float* plane_pts = fp + plane * (int64_t)N * 3;
        const int64_t flat = (plane * hw + pix) * (int64_t)N;
        float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f, u3 = 0.0f;
        int64_t have = -1;  // the group of four stream elements u0..u3 hold
        if constexpr (FUZZ) {
            const int64_t r = plane * H + y;
            if (live) px.rlo = unordered(fz.stats[2 + 2 * r]), px.rhi = unordered(fz.stats[3 + 2 * r]);
        }
        uint32_t c1[kTerms], c2[kTerms];  // the ordered images of the idx1-th and idx2-th smallest, built from the top bit down
        float m0[kTerms], smax[kTerms], ssum[kTerms], sacc[kTerms];
        int arg[kTerms];
#pragma unroll
        for (int t = 0; t < kTerms; ++t) c1[t] = c2[t] = 0u, m0[t] = INFINITY, smax[t] = -INFINITY, ssum[t] = 0.0f, sacc[t] = 0.0f, arg[t] = 0;
        for (int sweep = stats ? -1 : 0; sweep < (select ? 32 : 0); ++sweep) {
            const uint32_t bit = sweep < 0 ? 0u : 0x80000000u >> sweep;
            int n1[kTerms], n2[kTerms];
#pragma unroll
            for (int t = 0; t < kTerms; ++t) n1[t] = n2[t] = 0;
            for (int base = 0; base < N; base += kChunk) {
                const int cnt = N - base < kChunk ? N - base : kChunk;
                __syncthreads();  // the previous chunk has been read
                for (int i = (int)threadIdx.x; i < cnt; i += BLOCK) {
                    const float* p = plane_pts + (int64_t)(base + i) * 3;
                    pts[3 * i + 0] = rem1(__fmul_rn(p[0], scale));
                    pts[3 * i + 1] = rem1(__fmul_rn(p[1], scale));
                    pts[3 * i + 2] = rem1(__fmul_rn(p[2], scale));
                }
                __syncthreads();
                for (int j = 0; j < cnt; ++j) {
                    const float d0 = wrap_diff(gy, pts[3 * j + 0]), d1 = wrap_diff(gx, pts[3 * j + 1]), d2 = wrap_diff(gz, pts[3 * j + 2]);
                    const float dist = rank_distance<FUZZ>(prog, n_d, fz, px, u0, u1, u2, u3, have, d0, d1, d2, flat + base + j, live);
#pragma unroll
                    for (int t = 0; t < kTerms; ++t) {
                        if (t >= n_r) break;
                        const sonar_voronoi_rterm& r = prog.r[t];
                        const float e = rank_value(r, dist);
                        if (sweep >= 0) {
                            const uint32_t key = ordered(e);
                            n1[t] += key < (c1[t] | bit) ? 1 : 0;
                            n2[t] += key < (c2[t] | bit) ? 1 : 0;
                        } else if (r.op == SONAR_VORONOI_R_SOFTMIN || r.op == SONAR_VORONOI_R_SOFTMIN_SORTED) {
                            const float norm = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
                            const float logit = __fmul_rn(-norm, r.temperature);
                            const float top = fmaxf(smax[t], logit);
                            const float keep = expf(__fsub_rn(smax[t], top)), w = expf(__fsub_rn(logit, top));  // the first point: exp(-inf) = 0
                            ssum[t] = __fadd_rn(__fmul_rn(ssum[t], keep), w);
                            sacc[t] = __fadd_rn(__fmul_rn(sacc[t], keep), __fmul_rn(e, w));
                            smax[t] = top;
                        } else {  // the first index of the smallest
                            arg[t] = e < m0[t] ? base + j : arg[t];
                            m0[t] = fminf(m0[t], e);
                        }
                    }
                }
            }
            if (sweep >= 0) {
#pragma unroll
                for (int t = 0; t < kTerms; ++t) {
                    if (t >= n_r) break;
                    c1[t] |= n1[t] <= prog.r[t].idx1 ? bit : 0u;
                    c2[t] |= n2[t] <= prog.r[t].idx2 ? bit : 0u;
                }
            }
        }
        if constexpr (ROW) {  // (N <= kChunk: the last sweep left every point of the plane staged)
#pragma unroll
            for (int t = 0; t < kTerms; ++t) {
                if (t >= n_r) break;
                const sonar_voronoi_rterm& r = prog.r[t];
                if (r.op != SONAR_VORONOI_R_SOFTMIN_SORTED) continue;
                float* mine = row + threadIdx.x;
                float total = 0.0f;  // the softmax denominator, the weights' exponentials in index order
                for (int j = 0; j < N; ++j) {
                    const float d0 = wrap_diff(gy, pts[3 * j + 0]), d1 = wrap_diff(gx, pts[3 * j + 1]), d2 = wrap_diff(gz, pts[3 * j + 2]);
                    mine[j * kRowLanes] = rank_value(r, rank_distance<FUZZ>(prog, n_d, fz, px, u0, u1, u2, u3, have, d0, d1, d2, flat + j, live));
                    total = __fadd_rn(total, expf(__fsub_rn(softmin_logit(gy, gx, gz, pts + 3 * j, r.temperature), smax[t])));
                }
                float acc = 0.0f;
                for (int i = 0; i < N; ++i) {
                    const float ei = mine[i * kRowLanes];
                    int rank = 0;
                    for (int j = 0; j < N; ++j) {
                        const float ej = mine[j * kRowLanes];
                        rank += (ej < ei || (ej == ei && j < i)) ? 1 : 0;
                    }
                    const float w = __fdiv_rn(expf(__fsub_rn(softmin_logit(gy, gx, gz, pts + 3 * rank, r.temperature), smax[t])), total);
                    acc = __fadd_rn(acc, __fmul_rn(ei, w));
                }
                sacc[t] = acc, ssum[t] = 1.0f;
            }
        }
        float result = 0.0f;
#pragma unroll
        for (int t = 0; t < kTerms; ++t) {
            if (t >= n_r) break;
            const sonar_voronoi_rterm& r = prog.r[t];
            const float v1 = unordered(c1[t]), v2 = unordered(c2[t]);
            float v;
            switch (r.op) {
                case SONAR_VORONOI_R_F: v = v1; break;
                case SONAR_VORONOI_R_INV_F: v = __fdiv_rn(1.0f, __fadd_rn(v1, r.eps)); break;
                case SONAR_VORONOI_R_DIFF: v = __fsub_rn(v2, v1); break;
                case SONAR_VORONOI_R_DIFF2: v = __fdiv_rn(__fsub_rn(v2, v1), __fadd_rn(__fadd_rn(v2, v1), 1e-06f)); break;
                case SONAR_VORONOI_R_SOFTMIN:
                case SONAR_VORONOI_R_SOFTMIN_SORTED: v = __fdiv_rn(sacc[t], ssum[t]); break;
                case SONAR_VORONOI_R_CELLID: v = __fadd_rn(__fdiv_rn((float)arg[t], aux[t]), 1.0f); break;
                default: v = (float)arg[t]; break;
            }
#pragma unroll
            for (int k = 0; k < kChain; ++k) {
                if (k >= r.n_ridge) break;
                v = __fsub_rn(1.0f, __fmul_rn(r.ridge[k], v));
            }
            v = __fmul_rn(v, r.scale);
            result = t == 0 ? v : __fadd_rn(result, v);
        }
        if (live) {
            const int64_t at = plane * hw + pix;
            float o = __fadd_rn(out[at], __fmul_rn(result, amplitude));
            if (flags & SONAR_VORONOI_FINAL_DIV) o = __fdiv_rn(o, final_div);
            out[at] = o;
        }
    }
}

// gradient_magnitude (py/noise_generation.py:1706-1724) on two planes of inner results, replicate padding by clamped indices:
// acc += sqrt(dx^2 + dy^2) * scale, dx = r1[y][x + 1] - r2[y][x - 1], dy = r1[y + 1][x] - r2[y - 1][x]
__global__ void __launch_bounds__(kBlock) voronoi_gradient_kernel(const float* __restrict__ r1, const float* __restrict__ r2, float* __restrict__ acc,
                                                                  int64_t total, int H, int W, float scale) {
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < total; f += (int64_t)gridDim.x * kBlock) {
        const int64_t row = f / W, plane = row / H;
        const int x = (int)(f - row * W), y = (int)(row - plane * H);
        const int64_t base = plane * H * W;
        const int xl = x > 0 ? x - 1 : 0, xr = x < W - 1 ? x + 1 : W - 1, yu = y > 0 ? y - 1 : 0, yd = y < H - 1 ? y + 1 : H - 1;
        const float dx = __fsub_rn(r1[base + (int64_t)y * W + xr], r2[base + (int64_t)y * W + xl]);
        const float dy = __fsub_rn(r1[base + (int64_t)yd * W + x], r2[base + (int64_t)yu * W + x]);
        const float gm = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
        acc[f] = __fadd_rn(acc[f], __fmul_rn(gm, scale));
    }
}

// the result fuzz's `result += rand.mul_(fuzz * 2).sub_(fuzz)` (py/noise_generation.py:1772-1777)
__global__ void __launch_bounds__(kBlock) voronoi_fuzz_add_kernel(float* __restrict__ x, const float* __restrict__ u, int64_t n, float twice, float fuzz) {
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < n; f += (int64_t)gridDim.x * kBlock)
        x[f] = __fadd_rn(x[f], __fsub_rn(__fmul_rn(u[f], twice), fuzz));
}

// acc = acc + x * scale, then / final_div with SONAR_VORONOI_FINAL_DIV: a term into its octave, an octave into the output
__global__ void __launch_bounds__(kBlock) voronoi_acc_kernel(float* __restrict__ acc, const float* __restrict__ x, int64_t n, float scale, float final_div,
                                                             int flags) {
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < n; f += (int64_t)gridDim.x * kBlock) {
        float o = __fadd_rn(acc[f], __fmul_rn(x[f], scale));
        if (flags & SONAR_VORONOI_FINAL_DIV) o = __fdiv_rn(o, final_div);
        acc[f] = o;
    }
}

}  // namespace

}  // namespace sonar

// the checks every octave entry point shares (pass 0 and 1 of the fuzz entry take no output); rank: the rank route's ops, and its ranks
// are held to [0, N) by the entry point itself.  *launch: there are pixels to compute
static int voronoi_checks(const char* who, const float* fp, float* out, const float* aux, int64_t B, int64_t C, int64_t H, int64_t W, int64_t N,
                          int flags, const sonar_voronoi_program* prog, int pass, bool rank, bool* launch) {
    using namespace sonar;
    constexpr int64_t kMax = (int64_t)1 << 31;
    *launch = false;
    SONAR_REQUIRE(fp != nullptr && (out != nullptr || pass == 0 || pass == 1) && prog != nullptr, SONAR_ERR_ARG, "%s: NULL tensor or program", who);
    SONAR_REQUIRE((const void*)out != (const void*)fp, SONAR_ERR_ARG, "%s: out must not be fp", who);
    SONAR_REQUIRE(aux == nullptr || ((const void*)aux != (const void*)out), SONAR_ERR_ARG, "%s: out must not be aux", who);
    SONAR_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0 && N >= 0, SONAR_ERR_ARG, "%s: negative size (%lld, %lld, %lld, %lld, %lld)", who,
                  (long long)B, (long long)C, (long long)H, (long long)W, (long long)N);
    SONAR_REQUIRE(B < kMax && C < kMax && H < kMax && W < kMax && N < kMax, SONAR_ERR_ARG, "%s: a size beyond 2^31", who);
    SONAR_REQUIRE((flags & ~SONAR_VORONOI_FINAL_DIV) == 0, SONAR_ERR_ARG, "%s: flags 0x%x", who, flags);
    SONAR_REQUIRE(prog->n_d >= 1 && prog->n_d <= SONAR_VORONOI_MAX_TERMS && prog->n_r >= 1 && prog->n_r <= SONAR_VORONOI_MAX_TERMS, SONAR_ERR_ARG,
                  "%s: %d distance and %d result terms (1..%d each)", who, prog->n_d, prog->n_r, SONAR_VORONOI_MAX_TERMS);
    bool cellid = false;
    for (int t = 0; t < prog->n_d; ++t) {
        const sonar_voronoi_dterm& d = prog->d[t];
        SONAR_REQUIRE(d.metric >= SONAR_VORONOI_D_EUCLIDEAN && d.metric <= SONAR_VORONOI_D_ANGLE_SIGMOID, SONAR_ERR_ARG,
                      "%s: distance term %d: unknown metric %d", who, t, d.metric);
        SONAR_REQUIRE(d.idx >= 0 && d.idx <= 2, SONAR_ERR_ARG, "%s: distance term %d: component %d", who, t, d.idx);
        SONAR_REQUIRE(d.n_xform >= 0 && d.n_xform <= SONAR_VORONOI_MAX_CHAIN, SONAR_ERR_ARG, "%s: distance term %d: %d transforms", who, t, d.n_xform);
        for (int k = 0; k < d.n_xform; ++k)
            SONAR_REQUIRE(d.xform[k] >= SONAR_VORONOI_X_WEIGHT && d.xform[k] <= SONAR_VORONOI_X_FRACTAL_COS, SONAR_ERR_ARG,
                          "%s: distance term %d: unknown transform %d", who, t, d.xform[k]);
    }
    for (int t = 0; t < prog->n_r; ++t) {
        const sonar_voronoi_rterm& r = prog->r[t];
        SONAR_REQUIRE(r.op >= SONAR_VORONOI_R_F && r.op <= (rank ? SONAR_VORONOI_R_SOFTMIN_SORTED : SONAR_VORONOI_R_CELLID_RAW), SONAR_ERR_ARG,
                      "%s: result term %d: unknown op %d", who, t, r.op);
        SONAR_REQUIRE(rank || (r.idx1 >= 0 && r.idx1 <= 3 && r.idx2 >= 0 && r.idx2 <= 3), SONAR_ERR_ARG,
                      "%s: result term %d: idx (%d, %d) outside 0..3", who, t, r.idx1, r.idx2);
        SONAR_REQUIRE(r.n_fn >= 0 && r.n_fn <= SONAR_VORONOI_MAX_CHAIN && r.n_ridge >= 0 && r.n_ridge <= SONAR_VORONOI_MAX_CHAIN, SONAR_ERR_ARG,
                      "%s: result term %d: chains of %d and %d", who, t, r.n_fn, r.n_ridge);
        for (int k = 0; k < r.n_fn; ++k)
            SONAR_REQUIRE(r.fn[k] == SONAR_VORONOI_X_FRACTAL_SIN || r.fn[k] == SONAR_VORONOI_X_FRACTAL_COS, SONAR_ERR_ARG,
                          "%s: result term %d: unknown function %d", who, t, r.fn[k]);
        cellid = cellid || r.op == SONAR_VORONOI_R_CELLID;
    }
    SONAR_REQUIRE(!cellid || aux != nullptr, SONAR_ERR_ARG, "%s: a cellid term without aux", who);
    if (B == 0 || C == 0 || H == 0 || W == 0) return SONAR_OK;
    SONAR_REQUIRE(B * C < kMax && H * W < kMax && B * C * H * W < kMax, SONAR_ERR_ARG, "%s: 2^31 output values or more", who);
    SONAR_REQUIRE(N >= 2, SONAR_ERR_ARG, "%s: %lld feature points (at least 2)", who, (long long)N);
    SONAR_REQUIRE(N <= SONAR_VORONOI_MAX_POINTS, SONAR_ERR_UNSUPPORTED, "%s: %lld feature points (at most %d)", who, (long long)N,
                  SONAR_VORONOI_MAX_POINTS);
    *launch = true;
    return SONAR_OK;
}

// the checks and the launch the two top-four entry points share; fz NULL (pass -1): no fuzz term
static int voronoi_octave(const char* who, const float* fp, float* out, const float* aux, int64_t B, int64_t C, int64_t H, int64_t W, int64_t N,
                          float scale, float z_norm, float amplitude, float final_div, int flags, const sonar_voronoi_program* prog,
                          const sonar::FuzzArgs* fz, int pass, void* stream) {
    using namespace sonar;
    bool launch = false;
    const int rc = voronoi_checks(who, fp, out, aux, B, C, H, W, N, flags, prog, pass, false, &launch);
    if (rc != SONAR_OK || !launch) return rc;
    const int64_t planes = B * C, tiles = (H * W + kBlock - 1) / kBlock;
    const dim3 grid(grid_for(planes * tiles * kBlock, kBlock)), block(kBlock);
    const bool simple = fz == nullptr && prog->n_d == 1 && prog->n_r == 1 && prog->d[0].n_xform == 0 && prog->r[0].n_fn == 0;
    const FuzzArgs none{};
#define SONAR_VORONOI_LAUNCH(SIMPLE, PASS)                                                                                                  \
    hipLaunchKernelGGL((voronoi_octave_kernel<SIMPLE, PASS>), grid, block, 0, (hipStream_t)stream, fp, out, aux, planes, (int)H, (int)W, (int)N, \
                       scale, z_norm, amplitude, final_div, flags, *prog, fz ? *fz : none)
    if (fz == nullptr) {
        if (simple) SONAR_VORONOI_LAUNCH(true, -1);
        else SONAR_VORONOI_LAUNCH(false, -1);
    } else if (pass == 0) {
        SONAR_VORONOI_LAUNCH(false, 0);
    } else if (pass == 1) {
        SONAR_VORONOI_LAUNCH(false, 1);
    } else {
        SONAR_VORONOI_LAUNCH(false, 2);
    }
#undef SONAR_VORONOI_LAUNCH
    return check_launch(who);
}

extern "C" int sonar_voronoi_octave_f32(const float* fp, float* out, const float* aux, int64_t B, int64_t C, int64_t H, int64_t W, int64_t N,
                                        float scale, float z_norm, float amplitude, float final_div, int flags,
                                        const sonar_voronoi_program* prog, void* stream) {
    return voronoi_octave("sonar_voronoi_octave_f32", fp, out, aux, B, C, H, W, N, scale, z_norm, amplitude, final_div, flags, prog, nullptr, -1,
                          stream);
}

// what the fuzz distance term's arguments must satisfy, for both entry points that take one
static int voronoi_fuzz_checks(const char* who, const float* fp, const float* out, const float* u, const uint32_t* stats,
                               const sonar_voronoi_program* prog, int pass, int fuzz_term, double fuzz, uint64_t stream_id, int64_t elem_offset) {
    using namespace sonar;
    SONAR_REQUIRE(stats != nullptr, SONAR_ERR_ARG, "%s: NULL stats", who);
    SONAR_REQUIRE((const void*)stats != (const void*)out && (const void*)stats != (const void*)fp && (const void*)stats != (const void*)u &&
                      (u == nullptr || (const void*)u != (const void*)out),
                  SONAR_ERR_ARG, "%s: stats and u must be buffers of their own", who);
    SONAR_REQUIRE(pass >= 0 && pass <= 2, SONAR_ERR_ARG, "%s: pass %d", who, pass);
    SONAR_REQUIRE(prog == nullptr || (fuzz_term >= 0 && fuzz_term < prog->n_d), SONAR_ERR_ARG, "%s: fuzz term %d", who, fuzz_term);
    SONAR_REQUIRE(fuzz == fuzz, SONAR_ERR_ARG, "%s: fuzz is NaN", who);
    SONAR_REQUIRE(elem_offset >= 0 && elem_offset < ((int64_t)1 << 48) && stream_id < ((uint64_t)1 << 48), SONAR_ERR_ARG,
                  "%s: elem_offset %lld or the stream id outside [0, 2^48)", who, (long long)elem_offset);
    // (the flat index stays below 2^31 outputs x 4096 points, the stream element below that plus 2^48)
    return SONAR_OK;
}

extern "C" int sonar_voronoi_fuzz_octave_f32(const float* fp, float* out, const float* aux, const float* u, uint32_t* stats, int64_t B, int64_t C,
                                             int64_t H, int64_t W, int64_t N, float scale, float z_norm, float amplitude, float final_div,
                                             int flags, const sonar_voronoi_program* prog, int pass, int fuzz_term, double fuzz, uint64_t seed,
                                             uint64_t stream_id, int64_t elem_offset, void* stream) {
    using namespace sonar;
    const char* who = "sonar_voronoi_fuzz_octave_f32";
    const int rc = voronoi_fuzz_checks(who, fp, out, u, stats, prog, pass, fuzz_term, fuzz, stream_id, elem_offset);
    if (rc != SONAR_OK) return rc;
    const FuzzArgs fz{u, stats, fuzz, fuzz_term, seed, stream_id, elem_offset};
    return voronoi_octave(who, fp, out, aux, B, C, H, W, N, scale, z_norm, amplitude, final_div, flags, prog, &fz, pass, stream);
}

extern "C" int sonar_voronoi_rank_octave_f32(const float* fp, float* out, const float* aux, const float* u, uint32_t* stats, int64_t B, int64_t C,
                                             int64_t H, int64_t W, int64_t N, float scale, float z_norm, float amplitude, float final_div,
                                             int flags, const sonar_voronoi_program* prog, int fuzz_term, double fuzz, uint64_t seed,
                                             uint64_t stream_id, int64_t elem_offset, void* stream) {
    using namespace sonar;
    const char* who = "sonar_voronoi_rank_octave_f32";
    const bool fuzzed = fuzz_term != -1;
    if (fuzzed) {
        const int rc = voronoi_fuzz_checks(who, fp, out, u, stats, prog, 2, fuzz_term, fuzz, stream_id, elem_offset);
        if (rc != SONAR_OK) return rc;
    } else {
        SONAR_REQUIRE(u == nullptr && stats == nullptr, SONAR_ERR_ARG, "%s: uniforms or statistics without a fuzz term", who);
    }
    bool launch = false;
    const int rc = voronoi_checks(who, fp, out, aux, B, C, H, W, N, flags, prog, 2, true, &launch);
    if (rc != SONAR_OK) return rc;
    bool row = false;
    for (int t = 0; t < prog->n_r; ++t) {
        const sonar_voronoi_rterm& r = prog->r[t];
        SONAR_REQUIRE(r.idx1 >= 0 && r.idx2 >= 0, SONAR_ERR_ARG, "%s: result term %d: ranks (%d, %d) below 0", who, t, r.idx1, r.idx2);
        row = row || r.op == SONAR_VORONOI_R_SOFTMIN_SORTED;
    }
    if (!launch) return SONAR_OK;
    for (int t = 0; t < prog->n_r; ++t)
        SONAR_REQUIRE(prog->r[t].idx1 < N && prog->r[t].idx2 < N, SONAR_ERR_ARG, "%s: result term %d: ranks (%d, %d) of %lld points", who, t,
                      prog->r[t].idx1, prog->r[t].idx2, (long long)N);
    SONAR_REQUIRE(!row || N <= SONAR_VORONOI_RANK_ROW_N, SONAR_ERR_UNSUPPORTED, "%s: softmin:use_sorted on %lld feature points (at most %d)", who,
                  (long long)N, SONAR_VORONOI_RANK_ROW_N);
    const int64_t planes = B * C;
    const int per = row ? kRowLanes : kBlock;
    const int64_t tiles = (H * W + per - 1) / per;
    const dim3 grid(grid_for(planes * tiles * per, per)), block(per);
    const size_t lds = (size_t)(3 * kChunk + (row ? kRowLanes * (int)N : 0)) * sizeof(float);
    const FuzzArgs fz{u, stats, fuzz, fuzz_term, seed, stream_id, elem_offset};
#define SONAR_VORONOI_RANK_LAUNCH(ROW, FUZZ)                                                                                                  \
    do {                                                                                                                                      \
        if (ROW) lds_attr(reinterpret_cast<const void*>(voronoi_rank_kernel<ROW, FUZZ>), (int)((3 * kChunk + kRowLanes * kRowN) * sizeof(float))); \
        hipLaunchKernelGGL((voronoi_rank_kernel<ROW, FUZZ>), grid, block, lds, (hipStream_t)stream, fp, out, aux, planes, (int)H, (int)W, (int)N, \
                           scale, z_norm, amplitude, final_div, flags, *prog, fz);                                                            \
    } while (0)
    if (row) {
        if (fuzzed) SONAR_VORONOI_RANK_LAUNCH(true, true);
        else SONAR_VORONOI_RANK_LAUNCH(true, false);
    } else {
        if (fuzzed) SONAR_VORONOI_RANK_LAUNCH(false, true);
        else SONAR_VORONOI_RANK_LAUNCH(false, false);
    }
#undef SONAR_VORONOI_RANK_LAUNCH
    return check_launch(who);
}

extern "C" int sonar_voronoi_gradient_f32(const float* r1, const float* r2, float* acc, int64_t planes, int64_t H, int64_t W, float scale,
                                          void* stream) {
    using namespace sonar;
    const char* who = "sonar_voronoi_gradient_f32";
    constexpr int64_t kMax = (int64_t)1 << 31;
    SONAR_REQUIRE(r1 != nullptr && r2 != nullptr && acc != nullptr, SONAR_ERR_ARG, "%s: NULL tensor", who);
    SONAR_REQUIRE(acc != r1 && acc != r2, SONAR_ERR_ARG, "%s: acc must not be an input", who);
    SONAR_REQUIRE(planes >= 0 && H >= 0 && W >= 0, SONAR_ERR_ARG, "%s: negative size (%lld, %lld, %lld)", who, (long long)planes, (long long)H,
                  (long long)W);
    SONAR_REQUIRE(planes < kMax && H < kMax && W < kMax, SONAR_ERR_ARG, "%s: a size beyond 2^31", who);
    if (planes == 0 || H == 0 || W == 0) return SONAR_OK;
    SONAR_REQUIRE(H * W < kMax && planes * H * W < kMax, SONAR_ERR_ARG, "%s: 2^31 values or more", who);
    const int64_t total = planes * H * W;
    hipLaunchKernelGGL(voronoi_gradient_kernel, dim3(grid_for(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, r1, r2, acc, total, (int)H, (int)W,
                       scale);
    return check_launch(who);
}

extern "C" int sonar_voronoi_fuzz_add_f32(float* x, const float* u, int64_t n, float twice_fuzz, float fuzz, void* stream) {
    using namespace sonar;
    const char* who = "sonar_voronoi_fuzz_add_f32";
    SONAR_REQUIRE(x != nullptr && u != nullptr, SONAR_ERR_ARG, "%s: NULL tensor", who);
    SONAR_REQUIRE((const float*)x != u, SONAR_ERR_ARG, "%s: x must not be u", who);
    SONAR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), SONAR_ERR_ARG, "%s: n = %lld", who, (long long)n);
    if (n == 0) return SONAR_OK;
    hipLaunchKernelGGL(voronoi_fuzz_add_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, x, u, n, twice_fuzz, fuzz);
    return check_launch(who);
}

extern "C" int sonar_voronoi_acc_f32(float* acc, const float* x, int64_t n, float scale, float final_div, int flags, void* stream) {
    using namespace sonar;
    const char* who = "sonar_voronoi_acc_f32";
    SONAR_REQUIRE(acc != nullptr && x != nullptr, SONAR_ERR_ARG, "%s: NULL tensor", who);
    SONAR_REQUIRE((const float*)acc != x, SONAR_ERR_ARG, "%s: acc must not be x", who);
    SONAR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), SONAR_ERR_ARG, "%s: n = %lld", who, (long long)n);
    SONAR_REQUIRE((flags & ~SONAR_VORONOI_FINAL_DIV) == 0, SONAR_ERR_ARG, "%s: flags 0x%x", who, flags);
    if (n == 0) return SONAR_OK;
    hipLaunchKernelGGL(voronoi_acc_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, acc, x, n, scale, final_div, flags);
    return check_launch(who);
}
