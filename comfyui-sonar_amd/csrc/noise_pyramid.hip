// Pyramid (multi-resolution) noise: the resampler, the flat and the plane (LDS-staged) generate kernels with their route and
// look-ahead launch, and the levels that are drawn only to be shrunk.  The plane kernel hosts a chain's previous item (Prefix) and a
// later call's Perlin lattice (noise_stream.h).
#include "noise_stream.h"

namespace sonar {

#ifdef SONAR_NG_TRACE
__device__ unsigned long long g_ng_trace[256 * 16];
#endif

// ------------------------------------------------------------------------------------------------
// Resampling (F.interpolate semantics, ATen UpSampleKernel index/weight rules).
struct alignas(16) Lin {
    int i0, i1;
    float w0, w1;
};
__device__ __forceinline__ Lin lin_coord(int dst, float scale, int in_size) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;   // align_corners=False
    src = src < 0.0f ? 0.0f : src;
    int i0 = (int)floorf(src);
    i0 = i0 < in_size - 1 ? i0 : in_size - 1;
    float l1 = src - (float)i0;
    l1 = fminf(fmaxf(l1, 0.0f), 1.0f);
    Lin r;
    r.i0 = i0;
    r.i1 = i0 + 1 < in_size - 1 ? i0 + 1 : in_size - 1;
    r.w0 = 1.0f - l1;
    r.w1 = l1;
    return r;
}
__device__ __forceinline__ float bilerp(const float* __restrict__ plane, int w, const Lin& ly, const Lin& lx) {
    const float* r0 = plane + (int64_t)ly.i0 * w;
    const float* r1 = plane + (int64_t)ly.i1 * w;
    const float t0 = r0[lx.i0] * lx.w0 + r0[lx.i1] * lx.w1;
    const float t1 = r1[lx.i0] * lx.w0 + r1[lx.i1] * lx.w1;
    return t0 * ly.w0 + t1 * ly.w1;
}
__device__ __forceinline__ int nearest_exact_idx(int dst, float scale, int in_size) {
    const int i = (int)floorf(((float)dst + 0.5f) * scale);
    return i < in_size - 1 ? i : in_size - 1;
}
__device__ __forceinline__ int nearest_idx(int dst, float scale, int in_size) {  // legacy "nearest": floor(dst * scale)
    const int i = (int)floorf((float)dst * scale);
    return i < in_size - 1 ? i : in_size - 1;
}
// align_corners=True bilinear: src = dst * (in - 1) / (out - 1)
__device__ __forceinline__ Lin lin_coord_aligned(int dst, float scale, int in_size) {
    const float src = scale * (float)dst;
    int i0 = (int)src;
    i0 = i0 < in_size - 1 ? i0 : in_size - 1;
    const float l1 = src - (float)i0;
    Lin r;
    r.i0 = i0;
    r.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    r.w0 = 1.0f - l1;
    r.w1 = l1;
    return r;
}
// bicubic (A = -0.75, ATen UpSampleBicubic2d): taps at floor(src) - 1 .. + 2 with clamped indices; weights from t = src - floor(src)
struct Cubic {
    int i[4];
    float c[4];
};
__device__ __forceinline__ Cubic cubic_coord(int dst, float scale, int in_size, bool aligned) {
    const float A = -0.75f;
    const float src = aligned ? scale * (float)dst : scale * ((float)dst + 0.5f) - 0.5f;
    const float fl = floorf(src);
    const int i0 = (int)fl;
    const float t = src - fl, u = 1.0f - t;
    Cubic r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.i[k] = min(max(i0 - 1 + k, 0), in_size - 1);
    const float t1 = t + 1.0f, u1 = u + 1.0f;
    r.c[0] = ((A * t1 - 5.0f * A) * t1 + 8.0f * A) * t1 - 4.0f * A;
    r.c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    r.c[2] = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
    r.c[3] = ((A * u1 - 5.0f * A) * u1 + 8.0f * A) * u1 - 4.0f * A;
    return r;
}
__device__ __forceinline__ float bicubic(const float* __restrict__ plane, int w, const Cubic& cy, const Cubic& cx) {
    float rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* r = plane + (int64_t)cy.i[k] * w;
        rows[k] = r[cx.i[0]] * cx.c[0] + r[cx.i[1]] * cx.c[1] + r[cx.i[2]] * cx.c[2] + r[cx.i[3]] * cx.c[3];
    }
    return rows[0] * cy.c[0] + rows[1] * cy.c[1] + rows[2] * cy.c[2] + rows[3] * cy.c[3];
}
__device__ __forceinline__ float area_sample(const float* __restrict__ plane, int h, int w, int H, int W, int y, int x) {
    // adaptive average pooling window: [floor(i*in/out), ceil((i+1)*in/out)); 32-bit quotients whenever the products fit (a 64-bit
    // division is ~80 instructions, four of them per value were this mode's cost)
    int y0, y1, x0, x1;
    if ((int64_t)(H + 1) * h < (1ll << 31) && (int64_t)(W + 1) * w < (1ll << 31)) {
        y0 = (int)(((unsigned)y * (unsigned)h) / (unsigned)H), y1 = (int)((((unsigned)y + 1u) * (unsigned)h + (unsigned)H - 1u) / (unsigned)H);
        x0 = (int)(((unsigned)x * (unsigned)w) / (unsigned)W), x1 = (int)((((unsigned)x + 1u) * (unsigned)w + (unsigned)W - 1u) / (unsigned)W);
    } else {
        y0 = (int)(((int64_t)y * h) / H), y1 = (int)((((int64_t)y + 1) * h + H - 1) / H);
        x0 = (int)(((int64_t)x * w) / W), x1 = (int)((((int64_t)x + 1) * w + W - 1) / W);
    }
    float acc = 0.0f;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) acc += plane[(int64_t)yy * w + xx];
    return acc / (float)((y1 - y0) * (x1 - x0));
}

template <bool STATS>
__global__ void __launch_bounds__(kBlock) resample_acc_kernel(float* dst, const float* __restrict__ src, int64_t planes,
                                                               int H, int W, int h, int w, float scale, int mode,
                                                               int accumulate, double* partials) {
    kernarg_touch_for(dst, src, planes, H, W, h, w, scale, mode, accumulate, partials);
    __shared__ double red[2 * kBlock / 64];
    double s = 0.0, q = 0.0;
    const int64_t total = planes * H * W;
    const bool aligned = mode == 5 || mode == 6;  // align_corners=True: (in - 1) / (out - 1), 0 for a single output
    const float sy = aligned ? (H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f) : (float)h / (float)H;
    const float sx = aligned ? (W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f) : (float)w / (float)W;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int64_t p = i / ((int64_t)W * H);
        const float* plane = src + p * (int64_t)h * w;
        float v;
        if (mode == 0) {
            v = bilerp(plane, w, lin_coord(y, sy, h), lin_coord(x, sx, w));
        } else if (mode == 1) {
            v = plane[(int64_t)nearest_exact_idx(y, sy, h) * w + nearest_exact_idx(x, sx, w)];
        } else if (mode == 2) {
            v = area_sample(plane, h, w, H, W, y, x);
        } else if (mode == 3) {
            v = plane[(int64_t)nearest_idx(y, sy, h) * w + nearest_idx(x, sx, w)];
        } else if (mode == 6) {
            v = bilerp(plane, w, lin_coord_aligned(y, sy, h), lin_coord_aligned(x, sx, w));
        } else if (H == h && W == w) {
            v = plane[(int64_t)y * w + x];  // same size: ATen copies
        } else {
            v = bicubic(plane, w, cubic_coord(y, sy, h, aligned), cubic_coord(x, sx, w, aligned));
        }
        if (scale != 1.0f) v = v * scale;
        if (accumulate) v = dst[i] + v;
        dst[i] = v;
        if constexpr (STATS) {
            const double d = v;
            s += d; q += d * d;
        }
    }
    if constexpr (STATS) write_partial<kBlock>(s, q, partials, red);
}

// Pyramid, generate mode: out = N(0,1)[stream] * base_scale + sum_l bilerp(level_l) * w_l.  A level with the latent's own
// size (the reference's i = 0 level: ratio r^0 = 1) is one more independent N(0,1) per element times w0; the sum of the two
// independent normals is drawn as ONE normal scaled by sqrt(1 + w0^2) (same distribution, half the generator work).
constexpr int kMaxLevels = 12;
struct PyramidLevels {
    const float* ptr[kMaxLevels];
    int h[kMaxLevels], w[kMaxLevels];
    float weight[kMaxLevels];
    int count;       // small-grid levels
    int supplied;    // ... of them with a grid passed in (ptr != nullptr: replay mode)
    unsigned long long draw_stream[kMaxLevels];  // ptr == nullptr: the level grid is drawn by the plane kernel from this stream id
    int fullres;     // number of leading full-resolution levels folded into the base draw (0 or 1)
    float fullres_weight;
    float base_scale;  // sqrt(1 + fullres_weight^2) when fullres else 1
};

// MODE as in perlin_generate_kernel (0 raw (+stats), 1 statistics only, 2 normalised final).
template <int MODE, bool STATS>
__global__ void __launch_bounds__(kBlock) pyramid_generate_kernel(float* out, int64_t planes, int H, int W,
                                                                  PyramidLevels lv, int mode, uint64_t seed,
                                                                  uint64_t stream_id, int64_t elem_offset,
                                                                  double* partials, NormArgs na) {
    kernarg_touch_for(out, planes, H, W, lv, mode, seed, stream_id, elem_offset, partials, na);
    __shared__ double red[2 * kBlock / 64];
    __shared__ NormDecision sh;
    NormDecision dec{0.f, 1.f, 0, 0};
    if constexpr (MODE == 2) dec = decide_norm<kBlock>(na.partials, kNPart, na.n_total, na.thr_sd, red, &sh);
    const NormFast norm(dec, na.factor);
    double s = 0.0, q = 0.0;
    const int64_t n = planes * (int64_t)H * W;
    // W % 4 == 0 and elem_offset % 4 == 0 (launcher): a 4-group never straddles a row or the shard ends
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
    const int64_t first = elem_offset / kTileElems, last = (elem_offset + n - 1) / kTileElems;
    for (int64_t tile = first + wave; tile <= last; tile += nwaves) {
        TileRng rng = rng_stream(seed, stream_id, (uint64_t)tile, lane);
        const int64_t base = tile * kTileElems + (int64_t)lane * 4 - elem_offset;
        for (int it = 0; it < kTileIters; ++it) {
            float v[4];
            rng.normal4(v);
            if (lv.fullres) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] *= lv.base_scale;
            }
            const int64_t e = base + it * 256;
            if (e < 0 || e >= n) continue;
            const int x4 = (int)(e % W);
            const int y = (int)((e / W) % H);
            const int64_t p = e / ((int64_t)W * H);
            for (int l = 0; l < lv.count; ++l) {
                const int h = lv.h[l], w = lv.w[l];
                const float* plane = lv.ptr[l] + p * (int64_t)h * w;
                const float sy = (float)h / (float)H, sx = (float)w / (float)W;
                const float wt = lv.weight[l];
                if (mode == 0) {
                    const Lin ly = lin_coord(y, sy, h);
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += bilerp(plane, w, ly, lin_coord(x4 + k, sx, w)) * wt;
                } else if (mode == 1) {
                    const float* row = plane + (int64_t)nearest_exact_idx(y, sy, h) * w;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += row[nearest_exact_idx(x4 + k, sx, w)] * wt;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] += area_sample(plane, h, w, H, W, y, x4 + k) * wt;
                }
            }
            if constexpr (MODE == 2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = norm(v[k]);
            }
            if constexpr (MODE == 1) {
                const float ps = (v[0] + v[1]) + (v[2] + v[3]);
                const float pq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], v[3] * v[3])));
                s += (double)ps;
                q += (double)pq;
            } else {
                store_group<true>(out, n, e, v, s, q, STATS);
            }
        }
    }
    if constexpr (STATS || MODE == 1) write_partial<kBlock>(s, q, partials, red);
}

// One workgroup per plane, the plane's level grids staged in LDS (they are re-read ~4 H W / (h w) times each by the
// bilinear gathers); the four waves stride over the plane's RNG tiles.  Same values as the flat kernel above (to rounding).
// Requires W % 4 == 0 and elem_offset % (H * W) == 0 (whole planes; a plane may straddle RNG tiles).
// XROWS (bilinear, when it fits): every level grid is first stretched along x to the full width W in LDS (h_l rows of W
// floats), so an output needs, per level, two conflict-free 16-byte reads and two FMAs per value instead of four gathers, a
// coordinate-table read and eleven arithmetic instructions; the level weight is folded into the y weights.
constexpr size_t kPyramidLdsBudget = 64 * 1024;
// The grids and the stretched rows of a plane take up to 64 KB of LDS, so two workgroups fit a CU: with 256 threads that is two
// waves per SIMD (one at batch 64, where there is a plane per CU) and the tile loop runs at the latency of its dependent chains.
// kPyrParts 256-thread parts share one plane's LDS instead.
constexpr int kPyrParts = 2;
// items a thread stretches along x per round (XROWS).  Re-swept once the column-fixed path had made an item cheap (same box, batch 512 / 64,
// normalised call): 8 items 92.1 / 22.3 us, 4 items (the setting while an item was a table read and two dependent gathers) 89.7 / 21.9, 3 items
// 88.6 / 22.0, 2 items 88.5 / 21.7, **1 item 87.3 / 21.6**
constexpr int kPyrStretch = 1;
constexpr int kPyrGroup = 1, kPyrGroupPre = 1;  // burst steps whose level reads are in flight together (XROWS)
constexpr int kPyrBlock = kPyrParts * kBlock;
static_assert((kPyrParts & (kPyrParts - 1)) == 0 && kTileIters % kPyrParts == 0, "parts split a tile's burst evenly");

// fold (nullable y): the values are folded into a chain's running sum, out == fold.y (sonar_pyramid_generate_acc_f32); PRE != 0: the
// chain's previous item rides along (Prefix above) -- its generator shares this kernel's tile keying, so its state simply walks the
// same (tile, iteration) sequence.
// A Perlin lattice computed in `blocks` extra leading workgroups of a plane-kernel launch: the lattice of a LATER call's hosted Perlin item
// (sonar_pyramid_generate_acc_ahead_f32) -- independent of everything else in the launch.  blocks == 0: none.
// N words of a stream passed over as straight-line code: a counted loop around one multiply-add spent 96 cycles per word on its own
// bookkeeping (vector-exec loop, trace build of round 5: 3.1 k cycles for the 32 words of half a burst)
template <int N>
__device__ __forceinline__ void skip_words(TileRng& r) {
#pragma unroll
    for (int k = 0; k < N; ++k) r.next();
}

struct LatticeJob {
    float* out;
    int blocks, iters, blend_mode;
    int64_t C;
    uint64_t seed, stream_id;
};
static constexpr LatticeJob kNoLattice{nullptr, 0, 0, 0, 0, 0, 0};

// AHEAD (round 6, sonar_pyramid_noise_ahead_f32): a normalised call inside a prepared plan as ONE launch.  Workgroups [0, ah.main_blocks)
// run THIS call's planes and store them normalised -- the statistics were left by the previous call's launch -- with scale_noise_kernel's own
// operation sequence (ExactNorm: the same bits as the in-place pass); the workgroups behind them run the NEXT call's planes (its level
// table `ah.lv`, its stream ids) without storing anything and leave that call's (sum, sumsq) partials, workgroup by workgroup what its own
// generating launch would leave.  At the launch-bound sizes the two kinds sit side by side on the chip (one plane workgroup per CU before).
struct PyrAhead {
    NormArgs na;
    int npart;                      // partial pairs of THIS call's statistics (the workgroups of the launch that left them)
    PyramidLevels lv;               // the next call's level table, stream id and grid size
    unsigned long long stream_id;
    int grid_floats;
    int main_blocks;
    double* partials;               // the next call's statistics
};
// the decision as scale_noise_kernel's 256-thread blocks take it (same strides, same reduction order: same bits), inside a larger block
template <int SUB, int BLOCK>
__device__ __forceinline__ NormDecision decide_norm_as(const double* __restrict__ partials, int64_t npart, int64_t n_total, float thr_sd, double* red,
                                                       NormDecision* sh) {
    static_assert(BLOCK >= SUB && SUB % 64 == 0, "the first SUB threads of the block");
    constexpr int NW = SUB / 64;
    double s = 0.0, q = 0.0;
    if ((int)threadIdx.x < SUB)
        for (int64_t i = threadIdx.x; i < npart; i += SUB) {
            s += partials[2 * i];
            q += partials[2 * i + 1];
        }
    s = wave_sum(s);
    q = wave_sum(q);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0 && wid < NW) {
        red[wid] = s;
        red[NW + wid] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ss = 0.0, qq = 0.0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            ss += red[i];
            qq += red[NW + i];
        }
        *sh = decision_from_totals(ss, qq, n_total, thr_sd);
    }
    __syncthreads();
    return *sh;
}
// scale_noise_kernel's value sequence -- subtract, IEEE quotient, multiply -- with the quotient by the correctly rounded reciprocal and one
// residual step (sampler_steps.hip, PendingNorm:the same bits as `v / std` for every v in the normal range)
struct ExactNorm {
    float mean, stdv, inv_std, factor;
    bool sub, div, mul;
    __device__ __forceinline__ ExactNorm(const NormDecision& d, float f)
        : mean(d.mean), stdv(d.stdv), inv_std(1.0f / d.stdv), factor(f), sub(d.do_sub != 0), div(d.do_div != 0), mul(f != 1.0f) {}
    __device__ __forceinline__ float operator()(float v) const {
        if (sub) v = v - mean;
        if (div) {
            const float q = v * inv_std;
            v = __builtin_fmaf(__builtin_fmaf(-stdv, q, v), inv_std, q);
        }
        if (mul) v = v * factor;
        return v;
    }
};

// ROLE: 0 an ordinary launch; the look-ahead launch's workgroups: 1 this call's planes (normalised stores, no statistics), 2 the next call's
// planes (statistics into ah.partials, no stores).  The body is instantiated per role and handed ITS level table by reference -- the kernel
// arguments stay in scalar registers (selecting between the two tables at run time put a copy in scratch memory: 2 x slower).
template <bool STATS, bool XROWS, int PRE, bool NT, int ROLE>
__device__ __forceinline__ void pyramid_plane_body(float* out, int64_t planes, int H, int W, const PyramidLevels& lv, int mode, uint64_t seed,
                                                   uint64_t stream_id, int64_t elem_offset, double* partials, int grid_floats, const Accum& fold,
                                                   const Prefix& pre, const PyrAhead& ah, const int bid, const int nblocks) {
    static_assert(ROLE == 0 || (XROWS && !STATS && PRE == 0), "the look-ahead form is the stretched-rows kernel of a single generator");
    extern __shared__ __align__(16) float pyr_lds[];
    __shared__ double red[2 * kPyrBlock / 64];
    __shared__ NormDecision sh_dec;
    // the levels' parameters where a thread can index them by a run-time level (kernel arguments live in scalar registers: per-level
    // loops over them are sixteen short dependent loops; flattened over (level, item) a thread has four independent items in flight)
    __shared__ int lvl_h[kMaxLevels], lvl_w[kMaxLevels], lvl_off[kMaxLevels + 1], lvl_item0[kMaxLevels + 1], lvl_row0[kMaxLevels];
    __shared__ float lvl_weight[kMaxLevels];
    __shared__ unsigned long long lvl_stream[kMaxLevels];
    SONAR_NG_STAMP(0);
    double s = 0.0, q = 0.0;
    NormDecision dec{0.f, 1.f, 0, 0};
    if constexpr (ROLE == 1) dec = decide_norm_as<kBlock, kPyrBlock>(ah.na.partials, ah.npart, ah.na.n_total, ah.na.thr_sd, red, &sh_dec);
    const ExactNorm enorm(dec, ROLE == 1 ? ah.na.factor : 1.0f);
    const int HW = H * W;
    const uint32_t lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int part = wave / (kBlock / 64);  // 256-thread parts of the workgroup (wave-uniform: the step-ahead below is straight-line code)
    const int dy = 256 / W, dx = 256 - dy * W;  // one burst step advances 256 elements
    // bilinear source coordinates depend on (level, x) and (level, y) only: tabulated once per workgroup
    Lin* const xtab = reinterpret_cast<Lin*>(pyr_lds + grid_floats);  // [level][W]
    Lin* const ytab = xtab + lv.count * W;                            // [level][H]
    float* const xrows = reinterpret_cast<float*>(ytab + lv.count * H);  // XROWS: [level][h_l][W]
    if (mode == 2) {
        // area: the adaptive-average window [floor(i in / out), ceil((i + 1) in / out)) of every (level, x) and (level, y), tabulated once
        // per workgroup (i0 = start, i1 = end): the tile loop otherwise divides four times per value and level
        for (int l = 0; l < lv.count; ++l) {
            for (int i = threadIdx.x; i < W + H; i += kPyrBlock) {
                const bool isx = i < W;
                const int64_t d = isx ? i : i - W, in = isx ? lv.w[l] : lv.h[l], on = isx ? W : H;
                Lin a;
                a.i0 = (int)((d * in) / on);
                a.i1 = (int)(((d + 1) * in + on - 1) / on);
                a.w0 = (float)(a.i1 - a.i0);
                a.w1 = 0.0f;
                (isx ? xtab[l * W + d] : ytab[l * H + d]) = a;
            }
        }
    }
    // The parts other than the first reach their share of a tile's burst by stepping their generators over the iterations before it: a
    // dependent chain (~160 cycles per word at two waves per SIMD, 5 k cycles for half a burst -- those waves left the tile loop 2.2 us
    // after part 0's).  For the workgroup's first plane they do it HERE, while part 0 builds the coordinate tables alone.
    constexpr int kIters = kTileIters / kPyrParts;
    const int64_t t_ahead = part != 0 ? (elem_offset + (int64_t)bid * HW) / kTileElems + wave % (kBlock / 64) : -1;
    TileRng rng_ahead, prng_ahead;
    if (threadIdx.x == 0) {
        int off = 0, item = 0, row = 0;
#pragma unroll
        for (int l = 0; l < kMaxLevels; ++l) {
            if (l < lv.count) {
                const int n = lv.h[l] * lv.w[l];
                lvl_row0[l] = row;  // XROWS: the level's first stretched row
                row += lv.h[l];
                lvl_h[l] = lv.h[l];
                lvl_w[l] = lv.w[l];
                lvl_weight[l] = lv.weight[l];
                lvl_stream[l] = lv.draw_stream[l];
                lvl_off[l] = off;
                lvl_item0[l] = item;
                off += n;
                item += lv.ptr[l] ? 0 : min(kBlock, (n + 3) / 4);  // drawn levels: one item per active generator slot
            }
        }
        lvl_off[lv.count] = off;
        lvl_item0[lv.count] = item;
    }
    __syncthreads();
    SONAR_NG_STAMP(13);               // (trace builds: the level parameters are in LDS)
    SONAR_NG_STAMP_T(kBlock, 14);
    if (part != 0 && bid < planes) {
        rng_ahead = rng_stream(seed, stream_id, (uint64_t)t_ahead, lane);
        if constexpr (PRE != 0) prng_ahead = rng_stream(pre.seed, pre.stream_id, (uint64_t)t_ahead, lane);
        for (int k = 0; k < part; ++k) {
            skip_words<kIters * 4>(rng_ahead);
            if constexpr (PRE != 0) skip_words<kIters * 4>(prng_ahead);
        }
    }
    SONAR_NG_STAMP_T(kBlock, 15);     // (trace builds: the second part's generators are stepped ahead)
    if (mode == 0 && part == 0) {
        const int per = W + H;
        for (int j = threadIdx.x; j < lv.count * per; j += kBlock) {
            const int l = j / per, r = j - l * per, h = lvl_h[l], w = lvl_w[l];
            if (r < W) {
                xtab[l * W + r] = lin_coord(r, (float)w / (float)W, w);
            } else {
                const int i = r - W;
                Lin ly = lin_coord(i, (float)h / (float)H, h);
                const int pitch = XROWS ? W : w;
                ly.i0 *= pitch;  // row offsets
                ly.i1 *= pitch;
                if constexpr (XROWS) {
                    ly.i0 += lvl_row0[l] * W;  // ... from the first level's first stretched row
                    ly.i1 += lvl_row0[l] * W;
                    const float wt = lvl_weight[l];
                    ly.w0 *= wt;
                    ly.w1 *= wt;
                }
                ytab[l * H + i] = ly;
            }
        }
    }
    SONAR_NG_STAMP(1);
    for (int64_t p = bid; p < planes; p += nblocks) {
        __syncthreads();
        SONAR_NG_STAMP(2);
        if (lv.supplied) {  // (generate mode has none: the walk below costs a wait for three scalar loads per level to find that out)
            int off = 0;
            for (int l = 0; l < lv.count; ++l) {  // supplied levels (replay mode): copied
                const int n = lv.h[l] * lv.w[l];
                if (lv.ptr[l]) {
                    const float* src = lv.ptr[l] + p * (int64_t)n;
                    for (int i = threadIdx.x; i < n; i += kPyrBlock) pyr_lds[off + i] = src[i];
                }
                off += n;
            }
        }
        // drawn levels: stream (level stream id, global plane, slot), slot t of 256 owns elements 4t.., 4(t + 256)..; the (level, slot)
        // items of all levels are dealt to the workgroup's threads in one go (per level, the small levels left most threads idle
        // behind a generator seeding each)
        for (int item = threadIdx.x; item < lvl_item0[lv.count]; item += kPyrBlock) {
            int l = 0;
            while (item >= lvl_item0[l + 1]) ++l;
            const int gslot = item - lvl_item0[l], off = lvl_off[l], n = lvl_off[l + 1] - off;
            TileRng rng = rng_stream(seed, lvl_stream[l], (uint64_t)(elem_offset / HW + p), gslot);
            for (int i = gslot * 4; i < n; i += kBlock * 4) {
                float z[4];
                rng.normal4(z);
                float* const g = pyr_lds + off + i;
                if (i + 3 < n) {  // (four plain stores: the guarded loop below is a vector loop with a select chain per value, ~80 instructions)
                    g[0] = z[0]; g[1] = z[1]; g[2] = z[2]; g[3] = z[3];
                } else {
                    for (int k = 0; k < 4 && i + k < n; ++k) g[k] = z[k];
                }
            }
        }
        SONAR_NG_STAMP(3);
        __syncthreads();
        SONAR_NG_STAMP(4);
        if constexpr (XROWS) {
            int go = 0, ro = 0;
            for (int l = 0; l < lv.count; ++l) {
                const int h = lv.h[l], w = lv.w[l];
                const float* g = pyr_lds + go;
                const Lin* xt = xtab + l * W;
                int yy = (int)threadIdx.x / W, xx = (int)threadIdx.x - yy * W;
                const int sy = kPyrBlock / W, sx = kPyrBlock - sy * W;
                // kPyrStretch items per thread and round: their table reads and gathers are in flight together (one at a time, a level of
                // 45 rows was 13 rounds of three dependent LDS latencies: 4.4-4.9 k cycles per plane, as long as half the tile loop)
                if (sx == 0) {
                    // the workgroup's threads cover whole rows (W divides 512: every power-of-two width): a thread keeps its column, so
                    // its table entry is read once per level and an item is two gathers at a fixed stride, a multiply-add and a store
                    if (yy < h) {
                        const Lin lx = xt[xx];
                        const float* c0 = g + lx.i0;
                        const float* c1 = g + lx.i1;
                        for (int r = yy; r < h; r += kPyrStretch * sy) {
                            float a[kPyrStretch], b[kPyrStretch];
#pragma unroll
                            for (int u = 0; u < kPyrStretch; ++u) {
                                const int ru = r + u * sy < h ? r + u * sy : r;
                                a[u] = c0[ru * w];
                                b[u] = c1[ru * w];
                            }
#pragma unroll
                            for (int u = 0; u < kPyrStretch; ++u)
                                if (r + u * sy < h) xrows[ro + (r + u * sy) * W + xx] = __builtin_fmaf(b[u], lx.w1, a[u] * lx.w0);
                        }
                    }
                    go += h * w;
                    ro += h * W;
                    continue;
                }
                for (int i = threadIdx.x; i < h * W; i += kPyrStretch * kPyrBlock) {
                    float a[kPyrStretch], b[kPyrStretch], wa[kPyrStretch], wb[kPyrStretch];
#pragma unroll
                    for (int u = 0; u < kPyrStretch; ++u) {
                        const bool on = i + u * kPyrBlock < h * W;
                        const Lin lx = xt[on ? xx : 0];
                        const float* row = g + (on ? yy : 0) * w;
                        a[u] = row[lx.i0];
                        b[u] = row[lx.i1];
                        wa[u] = lx.w0;
                        wb[u] = lx.w1;
                        yy += sy;
                        xx += sx;
                        if (xx >= W) {
                            xx -= W;
                            yy += 1;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kPyrStretch; ++u)
                        if (i + u * kPyrBlock < h * W) xrows[ro + i + u * kPyrBlock] = __builtin_fmaf(b[u], wb[u], a[u] * wa[u]);
                }
                go += h * w;
                ro += h * W;
            }
            SONAR_NG_STAMP(5);
            __syncthreads();
        }
        SONAR_NG_STAMP(6);
        float* const oplane = out + p * (int64_t)HW;
        const Accum pfold{fold.y, pre.ya, pre.f};
        const Divider pdiv(PRE == 2 ? pre.div_fac : 1.0f);
        // Perlin prefix: the plane's lattice vectors (the lattice repeats per latent of pre.chw = channels * H * W elements)
        const float* const tplane = PRE == 2 ? pre.terms + (int)(p % (pre.chw / HW)) * HW : nullptr;
        // RNG tiles overlapping this plane (a plane need not start or end on a tile boundary: the neighbours' workgroups draw
        // the shared tile too and each keeps its own part)
        const int64_t g0 = elem_offset + p * (int64_t)HW;
        const int64_t tile_first = g0 / kTileElems, tile_last = (g0 + HW - 1) / kTileElems;
        // a tile's burst is split between the parts: part k runs iterations [k, k + 1) * kTileIters / kPyrParts after stepping its
        // generators over the iterations before them (8 plain instructions per word instead of a Box-Muller pair)
        for (int64_t t = tile_first + wave % (kBlock / 64); t <= tile_last; t += kBlock / 64) {
            TileRng rng, prng;
            if (t == t_ahead && p == bid) {  // wave-uniform: stepped ahead before the tables
                rng = rng_ahead;
                if constexpr (PRE != 0) prng = prng_ahead;
            } else {
                rng = rng_stream(seed, stream_id, (uint64_t)t, lane);
                if constexpr (PRE != 0) prng = rng_stream(pre.seed, pre.stream_id, (uint64_t)t, lane);
                for (int k = 0; k < part; ++k) {
                    skip_words<kIters * 4>(rng);
                    if constexpr (PRE != 0) skip_words<kIters * 4>(prng);
                }
            }
            SONAR_NG_STAMP(7);
            // element index inside the plane; < 0 or >= HW: not ours
            int e = (int)(t * kTileElems - g0) + (int)lane * 4 + part * kIters * 256;
            int y = e >= 0 ? e / W : -((-e + W - 1) / W);        // floor
            int x4 = e - y * W;
            if constexpr (XROWS) {
                // kPyrGroup burst steps at a time: a level's table entries, then its row pairs, are requested for the whole group before
                // the first is used.  Step by step a level was two dependent LDS latencies (table entry -> row addresses -> rows) and a
                // scalar load of its height: ~675 cycles per step with three levels at one or two workgroups per CU (trace build of round
                // 5), the arithmetic of a step being ~120 instructions.  Same draws, same operation order per value: the same bits.
                constexpr int G = PRE != 0 ? kPyrGroupPre : kPyrGroup;
                static_assert(kIters % G == 0, "groups tile a part's share of the burst");
                const float base_mul = lv.fullres ? lv.base_scale : 1.0f;  // (x 1 is exact: no select per value)
                // WHOLE: the tile lies inside the plane (always, when planes are whole tiles): no per-lane ownership test around the stores
                auto burst = [&](auto whole_c, const auto& dv) {  // dv: the hosted Perlin item's word-to-value converter (with_divider)
                    constexpr bool WHOLE = decltype(whole_c)::value;
                    // A hosted Perlin item's lattice vectors.  Launch-bound sizes (NT, one workgroup per CU): all of the part's share of
                    // the burst requested before the first step, the loop unrolled so that the steps index them statically -- a step that
                    // asks for its own waits for it with one other wave on its SIMD to cover: 7 k of the chain's 15.5 k cycles per tile
                    // (trace build of round 5), chain at batch 64 26.1 -> 25.2 us.  At batch 512 (four waves per SIMD cover the load) the
                    // same form is 3 % SLOWER (120 registers, eight copies of the step), and so is a request one step ahead in the rolled
                    // loop (+5 %): there a step loads its own.
                    constexpr bool LAT_AHEAD = PRE == 2 && NT;
                    auto lattice = [&](int ei) {
                        return PRE == 2 && (WHOLE || (ei >= 0 && ei < HW)) ? *reinterpret_cast<const float4*>(tplane + ei) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    };
                    constexpr int NTV = LAT_AHEAD ? kIters : 1;
                    float4 tva[NTV];
                    if constexpr (LAT_AHEAD) {
#pragma unroll
                        for (int i = 0; i < kIters; ++i) tva[i] = lattice(e + 256 * i);
                    }
#pragma unroll NTV
                    for (int it0 = 0; it0 < kIters; it0 += G) {
                        float4 tvs[G];
#pragma unroll
                        for (int j = 0; j < G; ++j) tvs[j] = LAT_AHEAD ? tva[LAT_AHEAD ? it0 + j : 0] : lattice(e + 256 * j);
                        float v[G][4], px[G][4];
                        int ee[G], yy[G], xx[G];
#pragma unroll
                        for (int j = 0; j < G; ++j) {
                            rng.normal4(v[j]);
                            const bool ours = WHOLE || (e >= 0 && e < HW);
                            if constexpr (PRE != 0) {  // the prefix's generator walks every iteration of the tile, ours or not
                                const float4 tv = tvs[j];
                                prefix_draw<PRE>(prng, dv, tv, px[j]);
                            }
                            ee[j] = e;
                            yy[j] = ours ? y : 0;  // (not ours: any entry of the tables, the values are dropped)
                            xx[j] = ours ? x4 : 0;
                            e += 256;
                            y += dy;
                            x4 += dx;
                            if (x4 >= W) {
                                x4 -= W;
                                y += 1;
                            }
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[j][k] *= base_mul;
                        }
                        // the four values of a step as ONE 16-byte register value from the draw to the store: the level sums are packed
                        // multiply-adds on its halves, the store takes it as it is (as four scalars the compiler moved them between
                        // register pairs around the level loop and again before the store: 8-11 moves per step)
                        sonar_v4f vv[G];
#pragma unroll
                        for (int j = 0; j < G; ++j) vv[j] = sonar_v4f{v[j][0], v[j][1], v[j][2], v[j][3]};
                        const int nl = lv.count;
                        for (int l = 0; l < nl; ++l) {
                            Lin ly[G];
#pragma unroll
                            for (int j = 0; j < G; ++j) ly[j] = ytab[l * H + yy[j]];
                            sonar_v4f a[G], b[G];
#pragma unroll
                            for (int j = 0; j < G; ++j) {
                                a[j] = *reinterpret_cast<const sonar_v4f*>(xrows + ly[j].i0 + xx[j]);
                                b[j] = *reinterpret_cast<const sonar_v4f*>(xrows + ly[j].i1 + xx[j]);
                            }
#pragma unroll
                            for (int j = 0; j < G; ++j) {
                                const sonar_v4f w0 = {ly[j].w0, ly[j].w0, ly[j].w0, ly[j].w0}, w1 = {ly[j].w1, ly[j].w1, ly[j].w1, ly[j].w1};
                                vv[j] = __builtin_elementwise_fma(a[j], w0, __builtin_elementwise_fma(b[j], w1, vv[j]));
                            }
                        }
#pragma unroll
                        for (int j = 0; j < G; ++j) {
                            const int ej = ee[j];
                            if (!WHOLE && (ej < 0 || ej >= HW)) continue;
                            if constexpr (PRE != 0) {
                                float w[4] = {vv[j].x, vv[j].y, vv[j].z, vv[j].w};
                                prefix_fold(pre, pfold, fold, p * (int64_t)HW + ej, px[j], w);
                                vv[j] = sonar_v4f{w[0], w[1], w[2], w[3]};
                            } else if (fold.y) {
                                const float4 yv = *reinterpret_cast<const float4*>(fold.y + p * (int64_t)HW + ej);
                                vv[j] = sonar_v4f{fold(yv.x, vv[j].x), fold(yv.y, vv[j].y), fold(yv.z, vv[j].z), fold(yv.w, vv[j].w)};
                            }
                            if constexpr (ROLE == 1) vv[j] = sonar_v4f{enorm(vv[j].x), enorm(vv[j].y), enorm(vv[j].z), enorm(vv[j].w)};
                            if constexpr (ROLE != 2) {
                                if constexpr (NT) __builtin_nontemporal_store(vv[j], reinterpret_cast<sonar_v4f*>(oplane + ej));
                                else *reinterpret_cast<sonar_v4f*>(oplane + ej) = vv[j];
                            }
                            if constexpr (STATS || ROLE == 2) {
                                float s01 = vv[j].x + vv[j].y;
                                asm volatile("" : "+v"(s01));  // (two scalar adds: paired into one packed add they cost three moves)
                                const float ps = s01 + (vv[j].z + vv[j].w);
                                const float pq = __builtin_fmaf(vv[j].x, vv[j].x, __builtin_fmaf(vv[j].y, vv[j].y, __builtin_fmaf(vv[j].z, vv[j].z, vv[j].w * vv[j].w)));
                                s += (double)ps;
                                q += (double)pq;
                            }
                        }
                    }
                };
                const bool whole = t * kTileElems >= g0 && (t + 1) * kTileElems <= g0 + HW;
                auto run = [&](const auto& dv) {
                    if (whole) burst(std::true_type{}, dv);
                    else burst(std::false_type{}, dv);
                };
                if constexpr (PRE == 2) with_divider(pdiv, run);
                else run(pdiv);
                continue;
            }
#pragma unroll 1
            for (int it = 0; it < kIters; ++it, e += 256, y += dy, x4 += dx, y += x4 >= W, x4 -= x4 >= W ? W : 0) {
                float v[4];
                rng.normal4(v);
                float px[4];
                if constexpr (PRE != 0) {  // the prefix's generator walks every iteration of the tile, ours or not
                    const bool ours = e >= 0 && e < HW;
                    const float4 tv = PRE == 2 && ours ? *reinterpret_cast<const float4*>(tplane + e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    prefix_draw<PRE>(prng, pdiv, tv, px);
                }
                if (e < 0 || e >= HW) continue;
                if (lv.fullres) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] *= lv.base_scale;
                }
                int lo = 0;
                for (int l = 0; l < lv.count; ++l) {
                    const int h = lv.h[l], w = lv.w[l];
                    const float* plane = pyr_lds + lo;
                    lo += h * w;
                    const float wt = lv.weight[l];
                    if (mode == 0) {
                        const Lin ly = ytab[l * H + y];
                        const float* r0 = plane + ly.i0;
                        const float* r1 = plane + ly.i1;
                        const Lin* xt = xtab + l * W + x4;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const Lin lx = xt[k];
                            const float t0 = r0[lx.i0] * lx.w0 + r0[lx.i1] * lx.w1;
                            const float t1 = r1[lx.i0] * lx.w0 + r1[lx.i1] * lx.w1;
                            v[k] += (t0 * ly.w0 + t1 * ly.w1) * wt;
                        }
                    } else if (mode == 1) {
                        const float sy = (float)h / (float)H, sx = (float)w / (float)W;
                        const float* row = plane + nearest_exact_idx(y, sy, h) * w;
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] += row[nearest_exact_idx(x4 + k, sx, w)] * wt;
                    } else {
                        const Lin ly = ytab[l * H + y];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const Lin lx = xtab[l * W + x4 + k];
                            float acc = 0.0f;  // same order and rounding as area_sample
                            for (int yy = ly.i0; yy < ly.i1; ++yy)
                                for (int xx = lx.i0; xx < lx.i1; ++xx) acc += plane[yy * w + xx];
                            v[k] += acc / (ly.w0 * lx.w0) * wt;
                        }
                    }
                }
                if constexpr (PRE != 0) {
                    prefix_fold(pre, pfold, fold, p * (int64_t)HW + e, px, v);
                } else if (fold.y) {
                    const float4 yv = *reinterpret_cast<const float4*>(fold.y + p * (int64_t)HW + e);
                    v[0] = fold(yv.x, v[0]); v[1] = fold(yv.y, v[1]); v[2] = fold(yv.z, v[2]); v[3] = fold(yv.w, v[3]);
                }
                store4<NT>(oplane + e, v[0], v[1], v[2], v[3]);
                if constexpr (STATS) {
                    const float ps = (v[0] + v[1]) + (v[2] + v[3]);
                    const float pq = __builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], v[3] * v[3])));
                    s += (double)ps;
                    q += (double)pq;
                }
            }
        }
    }
    SONAR_NG_STAMP(8);
#ifdef SONAR_NG_TRACE  // when each of the waves 1..6 left the tile loop (wave 0 is slot 8)
#ifdef SONAR_NG_TRACE_PART1  // (the second part's waves 4..6 instead)
    if (lane == 0 && wave >= 4 && wave <= 6 && blockIdx.x < 256) g_ng_trace[blockIdx.x * 16 + 6 + wave] = __builtin_readcyclecounter();
#else
    if (lane == 0 && wave >= 1 && wave <= 3 && blockIdx.x < 256) g_ng_trace[blockIdx.x * 16 + 9 + wave] = __builtin_readcyclecounter();
#endif
#endif
    if constexpr (STATS) write_partial_at<kPyrBlock>(s, q, partials, red, bid, nblocks);
    if constexpr (ROLE == 2) write_partial_at<kPyrBlock>(s, q, ah.partials, red, bid, nblocks);
    SONAR_NG_STAMP(9);
}

template <bool STATS, bool XROWS, int PRE = 0, bool NT = false /* common.h store4: launch-bound sizes */, bool AHEAD = false>
__global__ void __launch_bounds__(kPyrBlock) pyramid_plane_kernel(float* out, int64_t planes, int H, int W, PyramidLevels lv, int mode,
                                                               uint64_t seed, uint64_t stream_id, int64_t elem_offset,
                                                               double* partials, int grid_floats, Accum fold, Prefix pre, LatticeJob lat,
                                                               PyrAhead ah) {
    kernarg_touch_for(out, planes, H, W, lv, mode, seed, stream_id, elem_offset, partials, grid_floats, fold, pre, lat, ah);
    if ((int)blockIdx.x < lat.blocks) {
        perlin_lattice_cells<kPyrBlock>(lat.out, lat.iters, lat.C, H, W, lat.blend_mode, lat.seed, lat.stream_id, blockIdx.x, lat.blocks);
        return;
    }
    const int bid = (int)blockIdx.x - lat.blocks;  // this workgroup among those that own planes
    if constexpr (!AHEAD) {
        pyramid_plane_body<STATS, XROWS, PRE, NT, 0>(out, planes, H, W, lv, mode, seed, stream_id, elem_offset, partials, grid_floats, fold, pre, ah, bid,
                                                     (int)gridDim.x - lat.blocks);
    } else if (bid < ah.main_blocks) {  // (workgroup-uniform)
        pyramid_plane_body<false, true, 0, NT, 1>(out, planes, H, W, lv, mode, seed, stream_id, elem_offset, nullptr, grid_floats, fold, pre, ah, bid,
                                                  ah.main_blocks);
    } else {
        pyramid_plane_body<false, true, 0, NT, 2>(out, planes, H, W, ah.lv, mode, seed, ah.stream_id, elem_offset, nullptr, ah.grid_floats, fold, pre, ah,
                                                  bid - ah.main_blocks, (int)gridDim.x - lat.blocks - ah.main_blocks);
    }
}

// Which kernel a level table gets, for the launch and for the host's query of it (sonar_pyramid_route) alike: 0 the flat kernel
// (pyramid_generate_kernel), 1 the plane kernel, 2 the plane kernel with stretched rows -- and the LDS sizes the decision rests on.
struct PyramidRoute {
    int route;
    size_t grid_floats, lds, lds_x;
};
static PyramidRoute pyramid_route(const PyramidLevels& lv, int64_t H, int64_t W, int mode, int64_t elem_offset) {
    size_t grid_floats = 0, rows = 0;
    for (int l = 0; l < lv.count; ++l) {
        grid_floats += (size_t)lv.h[l] * lv.w[l];
        rows += (size_t)lv.h[l];
    }
    grid_floats = (grid_floats + 3) & ~(size_t)3;  // the coordinate tables that follow are 16-byte entries
    const size_t lds = grid_floats * sizeof(float) + (mode == 0 || mode == 2 ? (size_t)lv.count * (H + W) * sizeof(Lin) : 0);
    const size_t lds_x = lds + rows * W * sizeof(float);
    int route = 1;
    if (W % 4 != 0 || elem_offset % (H * W) != 0 || lds > kPyramidLdsBudget) route = 0;
    else if (mode == 0 && lds_x <= kPyramidLdsBudget) route = 2;
    return PyramidRoute{route, grid_floats, lds, lds_x};
}

// true if the plane kernel was launched; *slots (optional): the number of partial pairs its workgroups own (the rest are zeroed)
static bool launch_pyramid_plane(float* out, int64_t planes, int64_t H, int64_t W, const PyramidLevels& lv, int mode, uint64_t seed,
                                 uint64_t stream_id, int64_t elem_offset, double* partials, hipStream_t st, Accum fold = kNoAccum,
                                 int pre_kind = 0, Prefix pre = Prefix{1.0f, 1.0f, 1.0f, 0, 0, nullptr, 1, 0}, LatticeJob lat = kNoLattice,
                                 int* slots = nullptr) {
    const PyramidRoute r = pyramid_route(lv, H, W, mode, elem_offset);
    if (r.route == 0) return false;
    const size_t grid_floats = r.grid_floats, lds = r.lds, lds_x = r.lds_x;
    const bool xrows = r.route == 2;
    const int g = (int)std::min<int64_t>(planes, kNPart);
    if (slots) *slots = g;
    const bool nt = nt_stores_host(planes * H * W);
#define SONAR_PPN(ST, XR, P, N) \
    hipLaunchKernelGGL((pyramid_plane_kernel<ST, XR, P, N>), dim3(g + lat.blocks), dim3(kPyrBlock), XR ? lds_x : lds, st, out, planes, (int)H, (int)W, lv, mode, \
                       seed, stream_id, elem_offset, partials, (int)grid_floats, fold, pre, lat, PyrAhead{})
#define SONAR_PP(ST, XR, P) \
    do { \
        if (nt) SONAR_PPN(ST, XR, P, true); else SONAR_PPN(ST, XR, P, false); \
    } while (0)
#define SONAR_PPK(ST, XR) \
    do { \
        if (pre_kind == SONAR_PREFIX_NORMAL) SONAR_PP(ST, XR, 1); \
        else if (pre_kind == SONAR_PREFIX_PERLIN) SONAR_PP(ST, XR, 2); \
        else SONAR_PP(ST, XR, 0); \
    } while (0)
    if (partials) {
        if (xrows) SONAR_PPK(true, true); else SONAR_PPK(true, false);
    } else {
        if (xrows) SONAR_PPK(false, true); else SONAR_PPK(false, false);
    }
#undef SONAR_PPK
#undef SONAR_PP
#undef SONAR_PPN
    return true;
}

// LDS of the stretched-rows form for one level table; 0: the form does not take it
static size_t pyramid_xrows_lds(const PyramidLevels& lv, int64_t H, int64_t W, int* grid_floats) {
    size_t gf = 0, rows = 0;
    for (int l = 0; l < lv.count; ++l) {
        gf += (size_t)lv.h[l] * lv.w[l];
        rows += (size_t)lv.h[l];
    }
    gf = (gf + 3) & ~(size_t)3;
    *grid_floats = (int)gf;
    const size_t lds = gf * sizeof(float) + (size_t)lv.count * (H + W) * sizeof(Lin) + rows * W * sizeof(float);
    return lds <= kPyramidLdsBudget ? lds : 0;
}
// The look-ahead launch: `now` planes of this call (null: none -- the statistics of `next` alone, for a call that found none left), `next`
// the call whose statistics go to partials_next.  false: a level table is beyond the stretched-rows form (nothing launched).
static bool launch_pyramid_ahead(float* out, int64_t planes, int64_t H, int64_t W, const PyramidLevels* now, uint64_t stream_now,
                                 const PyramidLevels& next, uint64_t stream_next, uint64_t seed, int64_t elem_offset, NormArgs na, int npart,
                                 double* partials_next, hipStream_t st) {
    int gf_now = 0, gf_next = 0;
    const size_t lds_now = now ? pyramid_xrows_lds(*now, H, W, &gf_now) : 1, lds_next = pyramid_xrows_lds(next, H, W, &gf_next);
    if (W % 4 != 0 || elem_offset % (H * W) != 0 || !lds_now || !lds_next) return false;
    const int g = (int)std::min<int64_t>(planes, kNPart);  // launch_pyramid_plane's grid: the partials' grouping
    PyrAhead ah{};
    ah.na = na;
    ah.npart = npart;
    ah.lv = next;
    ah.stream_id = stream_next;
    ah.grid_floats = gf_next;
    ah.main_blocks = now ? g : 0;
    ah.partials = partials_next;
    const PyramidLevels& first = now ? *now : next;
    const size_t lds = std::max(now ? lds_now : 0, lds_next);
    const Prefix nopre{1.0f, 1.0f, 1.0f, 0, 0, nullptr, 1, 0};
    if (nt_stores_host(planes * H * W))
        hipLaunchKernelGGL((pyramid_plane_kernel<false, true, 0, true, true>), dim3(ah.main_blocks + g), dim3(kPyrBlock), lds, st, out, planes, (int)H, (int)W, first,
                           0, seed, stream_now, elem_offset, (double*)nullptr, gf_now, kNoAccum, nopre, kNoLattice, ah);
    else
        hipLaunchKernelGGL((pyramid_plane_kernel<false, true, 0, false, true>), dim3(ah.main_blocks + g), dim3(kPyrBlock), lds, st, out, planes, (int)H, (int)W, first,
                           0, seed, stream_now, elem_offset, (double*)nullptr, gf_now, kNoAccum, nopre, kNoLattice, ah);
    return true;
}

// ------------------------------------------------------------------------------------------------
// Levels that are drawn only to be shrunk.  PyramidOld (py/noise_generation.py:567-606): noise = sum_i discount^i * interpolate(normal(std =
// 0.5^i) at (2^(i+1) H) x (2^(i+1) W), size = (H, W)); HighresPyramid (:517-564): levels of up to 15 x the latent's sides.  The reference (and the replay path here) materialises every level -- the last of five is 32 x 32 times the latent:
// 1 GiB for four SDXL latents -- to keep, with the default nearest-exact mode, ONE value of each 2^(i+1) x 2^(i+1) block.  On-device
// draws need no such tensor: the level value at (plane, ys, xs) is a counter-based normal keyed by its global element index
// (Philox4x32-10 of group e / 4, Box-Muller, slot e % 4), so the kernel draws exactly the taps the shrinking interpolation reads --
// nearest-exact / nearest 1, bilinear 2 x 2, bicubic 4 x 4 per level and output (the ratio is an exact power of two: the source
// coordinate sits half way between two samples), any ratio through the resampler's own index rules.  sonar_level_normal_f32 writes a
// whole level from the same keys: the definition the sampled kernel is tested against.  Area mode averages whole blocks of independent normals: the
// block mean IS a normal of std 0.5^i / 2^(i+1), drawn directly (same joint distribution as drawing the level and pooling it).
__device__ __forceinline__ float level_normal(uint64_t seed, uint64_t stream, int64_t e) {
    float z[4];
    philox_normal4(seed, stream, (uint64_t)(e >> 2), z);
    const int slot = (int)(e & 3);
    return slot == 0 ? z[0] : slot == 1 ? z[1] : slot == 2 ? z[2] : z[3];
}

// MODE: RESAMPLE ids 0 bilinear, 1 nearest-exact, 2 area (whole-block windows only), 3 nearest, 4 bicubic -- the resampler's own index and
// weight rules (lin_coord / nearest_*_idx / cubic_coord above) with the plane read replaced by the keyed draw.
constexpr int kMaxSampledLevels = 16;
struct SampledLevels {
    int count;
    int h[kMaxSampledLevels], w[kMaxSampledLevels];
    float weight[kMaxSampledLevels], sd[kMaxSampledLevels];
};

template <int MODE>
__global__ void __launch_bounds__(kBlock) levels_sampled_kernel(float* out, int64_t planes, int H, int W, SampledLevels lv, uint64_t seed,
                                                                 uint64_t stream0, int64_t plane_offset, int accumulate) {
    kernarg_touch_for(out, planes, H, W, lv, seed, stream0, plane_offset, accumulate);
    const int64_t total = planes * H * W;
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kBlock) {
        const int64_t p = idx / ((int64_t)H * W);
        const int rem = (int)(idx - p * H * W), y = rem / W, x = rem - y * W;
        float acc = accumulate ? out[idx] : 0.0f;
        for (int l = 0; l < lv.count; ++l) {
            const int h = lv.h[l], w = lv.w[l];
            const float sd = lv.sd[l];
            const int64_t base = (plane_offset + p) * (int64_t)h * w;
            const uint64_t stream = stream0 + (uint64_t)l;
            auto at = [&](int yy, int xx) { return level_normal(seed, stream, base + (int64_t)yy * w + xx) * sd; };
            const float sy = (float)h / (float)H, sx = (float)w / (float)W;
            float v;
            if constexpr (MODE == 2) {
                // area over whole r x r blocks of independent N(0, sd^2) values: the block mean is exactly one N(0, (sd / r)^2) value,
                // independent from block to block -- drawn as such, keyed by the OUTPUT element (no level value is defined for this mode)
                v = level_normal(seed, stream, (plane_offset + p) * (int64_t)H * W + rem) * (sd / sqrtf((float)(h / H) * (float)(w / W)));
            } else if constexpr (MODE == 1) {
                v = at(nearest_exact_idx(y, sy, h), nearest_exact_idx(x, sx, w));
            } else if constexpr (MODE == 3) {
                v = at(nearest_idx(y, sy, h), nearest_idx(x, sx, w));
            } else if constexpr (MODE == 0) {
                const Lin ly = lin_coord(y, sy, h), lx = lin_coord(x, sx, w);
                const float t0 = at(ly.i0, lx.i0) * lx.w0 + at(ly.i0, lx.i1) * lx.w1;
                const float t1 = at(ly.i1, lx.i0) * lx.w0 + at(ly.i1, lx.i1) * lx.w1;
                v = t0 * ly.w0 + t1 * ly.w1;
            } else {
                const Cubic cy = cubic_coord(y, sy, h, false), cx = cubic_coord(x, sx, w, false);
                float rows[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    rows[k] = at(cy.i[k], cx.i[0]) * cx.c[0] + at(cy.i[k], cx.i[1]) * cx.c[1] + at(cy.i[k], cx.i[2]) * cx.c[2] + at(cy.i[k], cx.i[3]) * cx.c[3];
                v = rows[0] * cy.c[0] + rows[1] * cy.c[1] + rows[2] * cy.c[2] + rows[3] * cy.c[3];
            }
            v = v * lv.weight[l];  // the resampler's order: scale, then add to the running sum
            acc = acc + v;
        }
        out[idx] = acc;
    }
}

__global__ void __launch_bounds__(kBlock) level_normal_kernel(float* level, int64_t n, float sd, uint64_t seed, uint64_t stream,
                                                               int64_t elem_offset) {
    kernarg_touch_for(level, n, sd, seed, stream, elem_offset);
    // a thread per Philox group of four consecutive elements (the ends of the range may cut a group)
    const int64_t g0 = elem_offset >> 2, g1 = (elem_offset + n + 3) >> 2;
    for (int64_t g = g0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; g < g1; g += (int64_t)gridDim.x * kBlock) {
        float z[4];
        philox_normal4(seed, stream, (uint64_t)g, z);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = 4 * g + k - elem_offset;
            if (i >= 0 && i < n) level[i] = z[k] * sd;
        }
    }
}

static int fill_levels(PyramidLevels& lv, int64_t H, int64_t W, int64_t nlevels, const float* const* level_ptrs,
                       const int64_t* level_h, const int64_t* level_w, const float* level_weight, uint64_t stream_id, bool* drawn,
                       const char* what) {
    *drawn = false;
    lv = PyramidLevels{};
    lv.fullres_weight = 1.0f;
    lv.base_scale = 1.0f;
    SONAR_REQUIRE(nlevels == 0 || (level_ptrs && level_h && level_w && level_weight), SONAR_ERR_ARG, "%s: level arrays missing", what);
    for (int64_t l = 0; l < nlevels; ++l) {
        if (level_ptrs[l] == nullptr && level_h[l] == H && level_w[l] == W) {
            // a NULL pointer at the latent's own size: the level is folded into the base draw
            SONAR_REQUIRE(lv.fullres == 0, SONAR_ERR_ARG, "%s: only one in-kernel full-resolution level", what);
            lv.fullres = 1;
            lv.fullres_weight = level_weight[l];
            lv.base_scale = sqrtf(1.0f + level_weight[l] * level_weight[l]);
            continue;
        }
        SONAR_REQUIRE(lv.count < kMaxLevels, SONAR_ERR_UNSUPPORTED, "%s: too many levels", what);
        lv.ptr[lv.count] = level_ptrs[l];
        lv.draw_stream[lv.count] = stream_id + 2 + (uint64_t)l;  // used when ptr is NULL: the plane kernel draws the grid
        if (!level_ptrs[l]) *drawn = true;
        else ++lv.supplied;
        lv.h[lv.count] = (int)level_h[l];
        lv.w[lv.count] = (int)level_w[l];
        lv.weight[lv.count] = level_weight[l];
        ++lv.count;
    }
    return SONAR_OK;
}

}  // namespace sonar

using namespace sonar;

// ================================================================================================
extern "C" int sonar_resample_acc_f32(float* dst, const float* src, int64_t planes, int64_t H, int64_t W, int64_t h,
                                      int64_t w, float scale, int mode, int accumulate, double* partials, void* stream) {
    SONAR_REQUIRE(dst && src && planes >= 0 && H > 0 && W > 0 && h > 0 && w > 0 && mode >= 0 && mode <= 6, SONAR_ERR_ARG,
                  "sonar_resample_acc_f32: bad argument");
    SONAR_REQUIRE(H < (1 << 24) && W < (1 << 24) && h < (1 << 24) && w < (1 << 24), SONAR_ERR_UNSUPPORTED,
                  "sonar_resample_acc_f32: plane too large");
    if (planes == 0) return SONAR_OK;
    const int g = (int)std::min<int64_t>(kNPart, grid_for(planes * H * W, kBlock * 2));
    if (partials)
        hipLaunchKernelGGL((resample_acc_kernel<true>), dim3(g), dim3(kBlock), 0, (hipStream_t)stream, dst, src, planes,
                           (int)H, (int)W, (int)h, (int)w, scale, mode, accumulate, partials);
    else
        hipLaunchKernelGGL((resample_acc_kernel<false>), dim3(g), dim3(kBlock), 0, (hipStream_t)stream, dst, src, planes,
                           (int)H, (int)W, (int)h, (int)w, scale, mode, accumulate, partials);
    return check_launch("sonar_resample_acc_f32");
}

static int pyramid_common(const char* what, float* out, int64_t planes, int64_t H, int64_t W, int mode, int64_t elem_offset) {
    SONAR_REQUIRE(out && planes >= 0 && H > 0 && W > 0 && mode >= 0 && mode <= 2 && elem_offset >= 0, SONAR_ERR_ARG,
                  "%s: bad argument", what);
    SONAR_REQUIRE(W % 4 == 0 && aligned16(out) && elem_offset % 4 == 0, SONAR_ERR_UNSUPPORTED,
                  "%s: needs W %% 4 == 0 and 16-byte aligned output", what);
    return SONAR_OK;
}

extern "C" int sonar_pyramid_route(int64_t H, int64_t W, int64_t nlevels, const int64_t* level_h, const int64_t* level_w, int mode,
                                   int64_t elem_offset) {
    SONAR_REQUIRE(H > 0 && W > 0 && nlevels >= 0 && (nlevels == 0 || (level_h && level_w)) && mode >= 0 && mode <= 2 && elem_offset >= 0,
                  SONAR_ERR_ARG, "sonar_pyramid_route: bad argument");
    PyramidLevels lv{};
    bool folded = false;
    for (int64_t l = 0; l < nlevels; ++l) {
        SONAR_REQUIRE(level_h[l] > 0 && level_w[l] > 0, SONAR_ERR_ARG, "sonar_pyramid_route: bad argument");
        if (!folded && level_h[l] == H && level_w[l] == W) {  // as fill_levels takes a NULL level of the latent's own size: no grid
            folded = true;
            continue;
        }
        SONAR_REQUIRE(lv.count < kMaxLevels, SONAR_ERR_UNSUPPORTED, "sonar_pyramid_route: too many levels");
        lv.h[lv.count] = (int)level_h[l];
        lv.w[lv.count] = (int)level_w[l];
        ++lv.count;
    }
    return pyramid_route(lv, H, W, mode, elem_offset).route;
}

extern "C" int sonar_pyramid_generate_f32(float* out, int64_t planes, int64_t H, int64_t W, int64_t nlevels,
                                          const float* const* level_ptrs, const int64_t* level_h, const int64_t* level_w,
                                          const float* level_weight, int mode, uint64_t seed, uint64_t stream_id,
                                          int64_t elem_offset, double* partials, void* stream) {
    int rc = pyramid_common("sonar_pyramid_generate_f32", out, planes, H, W, mode, elem_offset);
    if (rc != SONAR_OK) return rc;
    PyramidLevels lv;
    bool drawn = false;
    rc = fill_levels(lv, H, W, nlevels, level_ptrs, level_h, level_w, level_weight, stream_id, &drawn, "sonar_pyramid_generate_f32");
    if (rc != SONAR_OK) return rc;
    if (planes == 0) return SONAR_OK;
    if (launch_pyramid_plane(out, planes, H, W, lv, mode, seed, stream_id, elem_offset, partials, (hipStream_t)stream))
        return check_launch("sonar_pyramid_generate_f32");
    SONAR_REQUIRE(!drawn, SONAR_ERR_UNSUPPORTED, "sonar_pyramid_generate_f32: in-kernel level grids need the plane kernel (H*W %% 4096 == 0, "
                  "whole planes, grids within the LDS budget): pass the grids explicitly");
    const int g = tile_grid(planes * H * W, elem_offset);
    if (partials)
        hipLaunchKernelGGL((pyramid_generate_kernel<0, true>), dim3(g), dim3(kBlock), 0, (hipStream_t)stream, out, planes,
                           (int)H, (int)W, lv, mode, seed, stream_id, elem_offset, partials, NormArgs{});
    else
        hipLaunchKernelGGL((pyramid_generate_kernel<0, false>), dim3(g), dim3(kBlock), 0, (hipStream_t)stream, out, planes,
                           (int)H, (int)W, lv, mode, seed, stream_id, elem_offset, partials, NormArgs{});
    return check_launch("sonar_pyramid_generate_f32");
}

// The same values folded into a chain's running sum (y <- y * y_mul + pyramid * x_mul, sonar_accumulate), optionally with the chain's
// previous item riding along (sonar_fold_prefix).  Plane kernel only: SONAR_ERR_UNSUPPORTED when it cannot run this shape.
static int pyramid_generate_acc(const char* what, const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t planes, int64_t H, int64_t W,
                                int64_t nlevels, const float* const* level_ptrs, const int64_t* level_h, const int64_t* level_w,
                                const float* level_weight, int mode, uint64_t seed, uint64_t stream_id, int64_t elem_offset, LatticeJob lat,
                                void* stream) {
    SONAR_REQUIRE(acc && acc->y, SONAR_ERR_ARG, "%s: bad argument", what);
    int rc = pyramid_common(what, acc->y, planes, H, W, mode, elem_offset);
    if (rc != SONAR_OK) return rc;
    PyramidLevels lv;
    bool drawn = false;
    rc = fill_levels(lv, H, W, nlevels, level_ptrs, level_h, level_w, level_weight, stream_id, &drawn, what);
    if (rc != SONAR_OK) return rc;
    Prefix px{1.0f, 1.0f, 1.0f, 0, 0, nullptr, 1, 0};
    if (pre) {
        rc = make_prefix(pre, px, what);
        if (rc != SONAR_OK) return rc;
        SONAR_REQUIRE(pre->kind != SONAR_PREFIX_PERLIN || pre->chw % (H * W) == 0, SONAR_ERR_UNSUPPORTED,
                      "%s: the Perlin prefix's latent is not a whole number of planes", what);
    }
    if (planes == 0) return SONAR_OK;
    SONAR_REQUIRE(launch_pyramid_plane(acc->y, planes, H, W, lv, mode, seed, stream_id, elem_offset, acc->partials, (hipStream_t)stream,
                                       Accum{acc->y, acc->y_mul, acc->x_mul}, pre ? pre->kind : 0, px, lat),
                  SONAR_ERR_UNSUPPORTED, "%s: the plane kernel cannot run this shape (whole planes, grids within the LDS budget)", what);
    return check_launch(what);
}

extern "C" int sonar_pyramid_generate_acc_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t planes, int64_t H, int64_t W,
                                              int64_t nlevels, const float* const* level_ptrs, const int64_t* level_h,
                                              const int64_t* level_w, const float* level_weight, int mode, uint64_t seed,
                                              uint64_t stream_id, int64_t elem_offset, void* stream) {
    return pyramid_generate_acc("sonar_pyramid_generate_acc_f32", acc, pre, planes, H, W, nlevels, level_ptrs, level_h, level_w, level_weight, mode,
                                seed, stream_id, elem_offset, kNoLattice, stream);
}

extern "C" int sonar_pyramid_generate_acc_ahead_f32(const sonar_accumulate* acc, const sonar_fold_prefix* pre, int64_t planes, int64_t H, int64_t W,
                                                    int64_t nlevels, const float* const* level_ptrs, const int64_t* level_h,
                                                    const int64_t* level_w, const float* level_weight, int mode, uint64_t seed,
                                                    uint64_t stream_id, int64_t elem_offset, float* lattice_out, int64_t lattice_iters,
                                                    int64_t lattice_channels, int blend_mode, uint64_t lattice_stream_id, void* stream) {
    const char* what = "sonar_pyramid_generate_acc_ahead_f32";
    SONAR_REQUIRE(pre && pre->kind == SONAR_PREFIX_PERLIN && lattice_out && lattice_out != pre->terms && lattice_iters >= 0 &&
                      lattice_iters < (1 << 20) && lattice_channels > 0 && blend_mode >= 0 && blend_mode <= 2 && H > 0 && W > 0 &&
                      lattice_channels * H * W == pre->chw,
                  SONAR_ERR_ARG, "%s: a hosted Perlin item and a lattice buffer for the later call's [C, H, W] table are required", what);
    LatticeJob lat{lattice_out, grid_for(pre->chw, kPyrBlock), (int)lattice_iters, blend_mode, lattice_channels, seed, lattice_stream_id};
    return pyramid_generate_acc(what, acc, pre, planes, H, W, nlevels, level_ptrs, level_h, level_w, level_weight, mode, seed, stream_id, elem_offset,
                                lat, stream);
}

extern "C" int sonar_levels_sampled_f32(float* out, int64_t planes, int64_t H, int64_t W, int nlevels, const int64_t* level_h,
                                       const int64_t* level_w, const float* level_weight, const float* level_sd, int mode, uint64_t seed,
                                       uint64_t stream_id, int64_t plane_offset, int accumulate, void* stream) {
    SONAR_REQUIRE(out && planes >= 0 && H > 0 && W > 0 && nlevels >= 0 && nlevels <= kMaxSampledLevels && plane_offset >= 0 &&
                      (nlevels == 0 || (level_h && level_w && level_weight && level_sd)),
                  SONAR_ERR_ARG, "sonar_levels_sampled_f32: bad argument (at most %d levels)", kMaxSampledLevels);
    SONAR_REQUIRE(mode >= 0 && mode <= 4, SONAR_ERR_UNSUPPORTED, "sonar_levels_sampled_f32: mode %d", mode);
    SampledLevels lv;
    lv.count = nlevels;
    for (int l = 0; l < nlevels; ++l) {
        SONAR_REQUIRE(level_h[l] > 0 && level_w[l] > 0 && level_h[l] < (1ll << 30) && level_w[l] < (1ll << 30) &&
                          (double)(plane_offset + planes) * (double)level_h[l] * (double)level_w[l] < 9.0e18,
                      SONAR_ERR_UNSUPPORTED, "sonar_levels_sampled_f32: level %d is too large for its element keys", l);
        // area: only whole blocks average independent values (any other ratio's windows overlap: draw the level and pool it)
        SONAR_REQUIRE(mode != 2 || (level_h[l] % H == 0 && level_w[l] % W == 0), SONAR_ERR_UNSUPPORTED,
                      "sonar_levels_sampled_f32: area mode needs levels of whole multiples of the output size");
        lv.h[l] = (int)level_h[l];
        lv.w[l] = (int)level_w[l];
        lv.weight[l] = level_weight[l];
        lv.sd[l] = level_sd[l];
    }
    if (planes == 0) return SONAR_OK;
    const int g = grid_for(planes * H * W, kBlock);
    hipStream_t st = (hipStream_t)stream;
#define SONAR_LS(M) hipLaunchKernelGGL(levels_sampled_kernel<M>, dim3(g), dim3(kBlock), 0, st, out, planes, (int)H, (int)W, lv, seed, stream_id, plane_offset, accumulate)
    if (mode == 0) SONAR_LS(0); else if (mode == 1) SONAR_LS(1); else if (mode == 2) SONAR_LS(2); else if (mode == 3) SONAR_LS(3); else SONAR_LS(4);
#undef SONAR_LS
    return check_launch("sonar_levels_sampled_f32");
}

extern "C" int sonar_level_normal_f32(float* level, int64_t planes, int64_t h, int64_t w, float sd, uint64_t seed, uint64_t stream_id,
                                      int64_t plane_offset, void* stream) {
    SONAR_REQUIRE(level && planes >= 0 && h > 0 && w > 0 && plane_offset >= 0, SONAR_ERR_ARG, "sonar_level_normal_f32: bad argument");
    const int64_t n = planes * h * w;
    if (n == 0) return SONAR_OK;
    hipLaunchKernelGGL(level_normal_kernel, dim3(grid_for(n / 4 + 2, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, level, n, sd, seed, stream_id,
                       plane_offset * h * w);
    return check_launch("sonar_level_normal_f32");
}

extern "C" int sonar_pyramid_noise_f32(float* out, int64_t planes, int64_t H, int64_t W, int64_t nlevels,
                                       const float* const* level_ptrs, const int64_t* level_h, const int64_t* level_w,
                                       const float* level_weight, int mode, uint64_t seed, uint64_t stream_id,
                                       int64_t elem_offset, float factor, float threshold_std_devs, double* partials,
                                       void* stream) {
    int rc = pyramid_common("sonar_pyramid_noise_f32", out, planes, H, W, mode, elem_offset);
    if (rc != SONAR_OK) return rc;
    SONAR_REQUIRE(partials, SONAR_ERR_ARG, "sonar_pyramid_noise_f32: partials workspace required");
    PyramidLevels lv;
    bool drawn = false;
    rc = fill_levels(lv, H, W, nlevels, level_ptrs, level_h, level_w, level_weight, stream_id, &drawn, "sonar_pyramid_noise_f32");
    if (rc != SONAR_OK) return rc;
    if (planes == 0) return SONAR_OK;
    // The level gathers make a re-draw cost more than a sweep: generate once (with statistics), then normalise in place
    int slots = kNPart;
    if (launch_pyramid_plane(out, planes, H, W, lv, mode, seed, stream_id, elem_offset, partials, (hipStream_t)stream, kNoAccum, 0,
                             Prefix{1.0f, 1.0f, 1.0f, 0, 0, nullptr, 1, 0}, kNoLattice, &slots)) {
        rc = check_launch("sonar_pyramid_noise_f32");
        if (rc != SONAR_OK) return rc;
        // the normalising pass reduces only the pairs the plane kernel's workgroups own (the others are zeros: the same sums, bit for bit,
        // from a quarter of the reads at batch 64, where every one of its 2048 workgroups reduced 16 KB of partials for 8 KB of values)
        return sonar_scale_noise_f32(out, planes * H * W, factor, 1, threshold_std_devs, partials, slots, planes * H * W, stream);
    }
    SONAR_REQUIRE(!drawn, SONAR_ERR_UNSUPPORTED, "sonar_pyramid_noise_f32: in-kernel level grids need the plane kernel: pass the grids explicitly");
    const int g = tile_grid(planes * H * W, elem_offset);
    const NormArgs na{partials, planes * H * W, factor, threshold_std_devs};
    hipLaunchKernelGGL((pyramid_generate_kernel<1, false>), dim3(g), dim3(kBlock), 0, (hipStream_t)stream, out, planes, (int)H,
                       (int)W, lv, mode, seed, stream_id, elem_offset, partials, NormArgs{});
    hipLaunchKernelGGL((pyramid_generate_kernel<2, false>), dim3(g), dim3(kBlock), 0, (hipStream_t)stream, out, planes, (int)H,
                       (int)W, lv, mode, seed, stream_id, elem_offset, nullptr, na);
    return check_launch("sonar_pyramid_noise_f32");
}

extern "C" int sonar_pyramid_noise_ahead_f32(float* out, int64_t planes, int64_t H, int64_t W, int64_t nlevels, const int64_t* level_h,
                                             const int64_t* level_w, const float* level_weight, int mode, uint64_t seed, uint64_t stream_id,
                                             int64_t elem_offset, float factor, float threshold_std_devs, double* partials, int have_stats,
                                             uint64_t next_stream_id, int64_t next_nlevels, const int64_t* next_level_h,
                                             const int64_t* next_level_w, const float* next_level_weight, double* partials_next, void* stream) {
    const char* what = "sonar_pyramid_noise_ahead_f32";
    int rc = pyramid_common(what, out, planes, H, W, mode, elem_offset);
    if (rc != SONAR_OK) return rc;
    SONAR_REQUIRE(partials && partials_next && partials != partials_next, SONAR_ERR_ARG, "%s: two statistics workspaces required", what);
    SONAR_REQUIRE(mode == 0 && nlevels <= kMaxLevels && next_nlevels <= kMaxLevels, SONAR_ERR_UNSUPPORTED,
                  "%s: bilinear levels drawn in the kernel only (sonar_pyramid_noise_f32 takes the rest)", what);
    const float* none[kMaxLevels] = {};
    PyramidLevels now, next;
    bool drawn = false;
    rc = fill_levels(now, H, W, nlevels, none, level_h, level_w, level_weight, stream_id, &drawn, what);
    if (rc != SONAR_OK) return rc;
    rc = fill_levels(next, H, W, next_nlevels, none, next_level_h, next_level_w, next_level_weight, next_stream_id, &drawn, what);
    if (rc != SONAR_OK) return rc;
    if (planes == 0) return SONAR_OK;
    int gf = 0;
    SONAR_REQUIRE(W % 4 == 0 && pyramid_xrows_lds(now, H, W, &gf) && pyramid_xrows_lds(next, H, W, &gf), SONAR_ERR_UNSUPPORTED,
                  "%s: a level table is beyond the plane kernel's stretched-rows form (nothing was launched)", what);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = planes * H * W;
    const int slots = (int)std::min<int64_t>(planes, kNPart);
    if (!have_stats) {
        // nobody left this call's statistics: its planes once without stores (the same partials the ordinary generating launch leaves)
        SONAR_REQUIRE(launch_pyramid_ahead(out, planes, H, W, nullptr, stream_id, now, stream_id, seed, elem_offset, NormArgs{}, 0, partials, st),
                      SONAR_ERR_UNSUPPORTED, "%s: shape not taken", what);
    }
    SONAR_REQUIRE(launch_pyramid_ahead(out, planes, H, W, &now, stream_id, next, next_stream_id, seed, elem_offset,
                                       NormArgs{partials, n, factor, threshold_std_devs}, slots, partials_next, st),
                  SONAR_ERR_UNSUPPORTED, "%s: shape not taken", what);
    return check_launch(what);
}

#ifdef SONAR_NG_TRACE
extern "C" int sonar_debug_ng_trace(unsigned long long* host_out) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sonar::g_ng_trace), sizeof(sonar::g_ng_trace));
}
#endif
