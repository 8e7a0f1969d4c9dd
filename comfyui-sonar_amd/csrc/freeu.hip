// FreeU Extreme (py/nodes/freeu_extreme.py:187-230): the hidden-mean scale map and the fused filter / scale / blend of a channel slice,
// in place on the UNet's feature map in its own dtype.
//   hidden mean   mean[b][p] over ALL channels (lanes walk p: coalesced across H * W; the channels of a position are split over the
//                 workgroup's waves and summed in fp32 through LDS), then one workgroup per sample takes (min, max) of its map.  The apply
//                 kernel normalises on the fly: s = 1 + (scale - 1) * ((m - min) / (max - min)), each step rounded as the reference's.
//   apply         PLAIN / FILTERED: one sweep, V elements per lane.  FUSED: one workgroup per plane of the slice -- load in the tensor's
//                 dtype, forward rows (W/2 complex values) + r2c split + forward columns, x filter, inverse columns, c2r rows: the
//                 general-size plane kernel's passes (power_any_core.h, power_irfft2_any_kernel SRC 2) with run-time factor pairs -- then
//                 scale, blend with the original value, one rounding, store in place.
// The original value is READ AGAIN in the epilogue rather than kept: the plane buffer H x (W/2 + 1) complex is all the LDS a 128 x 128 plane
// leaves for two workgroups per CU (66.5 of 80 KB), a second copy would halve the occupancy or shut the larger planes out, and the lines were
// loaded by this same workgroup a plane-time earlier (32 KB of fp16 per plane against 4 MB of L2 per XCD), so the second read is PRESUMED
// to hit the L2 -- no counter run has confirmed it.  In place is safe: a plane belongs
// to one workgroup, every load of the transform precedes the barrier in front of the epilogue, and an epilogue item reads exactly the
// elements it then writes.
#include <math.h>

#include <algorithm>

#include "dtype_io.h"
#include "power_any_core.h"
#include "range_reduce.h"

namespace sonar {
namespace freeu {

// dtype_io.h's conversions, keyed by the run-time dtype code of a 16-bit type
__device__ __forceinline__ float widen16(uint32_t bits, int dtype) {
    return dtype == SONAR_DTYPE_F16 ? widen(F16{(uint16_t)bits}) : widen(BF16{(uint16_t)bits});
}
// narrow<BF16>'s rule restated: through the shared function the NaN case compiles to a select where this compiles to a branch, and the
// four-element sweep measured 1.3 % slower with the select (profiles/dtype_io_time.txt)
__device__ __forceinline__ uint32_t narrow16(float v, int dtype) {  // nearest even; bf16 NaN -> the quiet NaN torch writes
    if (dtype == SONAR_DTYPE_F16) return narrow<F16>(v).bits;
    const uint32_t u = __float_as_uint(v);
    if (v != v) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// V consecutive elements of `dtype` from element index i of p; VEC: one access (the caller has checked the alignment)
template <int V, bool VEC>
__device__ __forceinline__ void load_elems(const void* p, int64_t i, int dtype, float (&v)[V]) {
    if (dtype == SONAR_DTYPE_F32) {
        const float* f = reinterpret_cast<const float*>(p) + i;
        if constexpr (VEC && V == 4) {
            const float4 t = *reinterpret_cast<const float4*>(f);
            v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        } else if constexpr (VEC && V == 2) {
            const float2 t = *reinterpret_cast<const float2*>(f);
            v[0] = t.x, v[1] = t.y;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = f[k];
        }
    } else {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p) + i;
        if constexpr (VEC && V == 4) {
            const uint2 t = *reinterpret_cast<const uint2*>(h);
            v[0] = widen16(t.x & 0xFFFFu, dtype), v[1] = widen16(t.x >> 16, dtype);
            v[2] = widen16(t.y & 0xFFFFu, dtype), v[3] = widen16(t.y >> 16, dtype);
        } else if constexpr (VEC && V == 2) {
            const uint32_t t = *reinterpret_cast<const uint32_t*>(h);
            v[0] = widen16(t & 0xFFFFu, dtype), v[1] = widen16(t >> 16, dtype);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = widen16(h[k], dtype);
        }
    }
}
template <int V, bool VEC>
__device__ __forceinline__ void store_elems(void* p, int64_t i, int dtype, const float (&v)[V]) {
    if (dtype == SONAR_DTYPE_F32) {
        float* f = reinterpret_cast<float*>(p) + i;
        if constexpr (VEC && V == 4) {
            *reinterpret_cast<float4*>(f) = make_float4(v[0], v[1], v[2], v[3]);
        } else if constexpr (VEC && V == 2) {
            *reinterpret_cast<float2*>(f) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) f[k] = v[k];
        }
    } else {
        uint16_t* h = reinterpret_cast<uint16_t*>(p) + i;
        if constexpr (VEC && V == 4) {
            uint2 t;
            t.x = narrow16(v[0], dtype) | (narrow16(v[1], dtype) << 16);
            t.y = narrow16(v[2], dtype) | (narrow16(v[3], dtype) << 16);
            *reinterpret_cast<uint2*>(h) = t;
        } else if constexpr (VEC && V == 2) {
            *reinterpret_cast<uint32_t*>(h) = narrow16(v[0], dtype) | (narrow16(v[1], dtype) << 16);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) h[k] = (uint16_t)narrow16(v[k], dtype);
        }
    }
}
template <int V, bool VEC>
__device__ __forceinline__ void load_f32(const float* p, int64_t i, float (&v)[V]) {
    load_elems<V, VEC>(p, i, SONAR_DTYPE_F32, v);
}

// what follows the filter: the scale (map or scalar), the blend with the original, for one sample
struct Finish {
    const float* mean;      // [B][HW] raw channel means, or null: the scalar
    const float* extremes;  // [B][2]
    float scale, scale_m1;  // (float)scale and (float)(scale - 1.0)
    int blend_mode;         // SONAR_CFG_BLEND_NONE: the scaled value itself
    float blend;
};
struct SampleScale {
    float lo, span;
};
__device__ __forceinline__ SampleScale sample_scale(const Finish& fin, int64_t b) {
    if (!fin.mean) return SampleScale{0.0f, 1.0f};
    const float lo = fin.extremes[2 * b], hi = fin.extremes[2 * b + 1];
    return SampleScale{lo, hi - lo};
}
// one element: f = filtered value, orig = the tensor's own, m = the channel mean at its position
__device__ __forceinline__ float finish_value(const Finish& fin, const SampleScale& ss, float f, float orig, float m) {
    const float s = fin.mean ? 1.0f + fin.scale_m1 * ((m - ss.lo) / ss.span) : fin.scale;
    const float v = f * s;
    return fin.blend_mode < 0 ? v : blend<float>(fin.blend_mode, orig, v, fin.blend);
}

// ---- hidden mean --------------------------------------------------------------------------------------------------------------------------
// block = 64 positions x kMeanSlices channel slices: lane l of every wave owns position p0 + l, wave w the channels cb + w, cb + w +
// kMeanSlices, ... of the workgroup's channel group [cb, ce).  One group: the mean itself is written.  G > 1 groups (few positions, many
// channels: [2, 1280, 32, 32] is 32 position chunks for 256 CUs): every group leaves its partial SUM in ws[g][b][p], and the extremes launch
// adds the G partials in order, divides and writes the mean before it reduces it.
constexpr int kMeanSlices = 8, kMeanThreads = 64 * kMeanSlices, kMeanMaxGroups = 16;
__global__ void __launch_bounds__(kMeanThreads) hidden_mean_kernel(const void* __restrict__ x, int dtype, int64_t C, int64_t HW, int64_t sb,
                                                                   int64_t sc, float* __restrict__ mean, int64_t chunks, float* __restrict__ ws,
                                                                   int groups, int64_t per_group, int64_t B) {
    kernarg_touch_for(x, dtype, C, HW, sb, sc, mean, chunks, ws, groups, per_group, B);
    __shared__ float part[kMeanSlices][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = blockIdx.x / chunks, p = (blockIdx.x - b * chunks) * 64 + lane;
    const int64_t cb = (int64_t)blockIdx.y * per_group, ce = cb + per_group < C ? cb + per_group : C;
    float acc = 0.0f;
    if (p < HW) {
        const int64_t base = b * sb + p;
        int64_t c = cb + w;
        // four independent loads in flight per lane
        for (; c + 3 * kMeanSlices < ce; c += 4 * kMeanSlices) {
            float v0[1], v1[1], v2[1], v3[1];
            load_elems<1, false>(x, base + c * sc, dtype, v0);
            load_elems<1, false>(x, base + (c + kMeanSlices) * sc, dtype, v1);
            load_elems<1, false>(x, base + (c + 2 * kMeanSlices) * sc, dtype, v2);
            load_elems<1, false>(x, base + (c + 3 * kMeanSlices) * sc, dtype, v3);
            acc += (v0[0] + v1[0]) + (v2[0] + v3[0]);
        }
        for (; c < ce; c += kMeanSlices) {
            float v0[1];
            load_elems<1, false>(x, base + c * sc, dtype, v0);
            acc += v0[0];
        }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && p < HW) {
        float s = part[0][lane];
#pragma unroll
        for (int k = 1; k < kMeanSlices; ++k) s += part[k][lane];
        if (groups > 1) ws[((int64_t)blockIdx.y * B + b) * HW + p] = s;
        else mean[b * HW + p] = s / (float)C;
    }
}

// (min, max) of one sample's map; a NaN anywhere makes both NaN (torch.min / torch.max propagate it).  groups > 1: the map is first made
// from the channel groups' partial sums (ws[g][b][p], g ascending) and written.
constexpr int kExtThreads = 1024;
__global__ void __launch_bounds__(kExtThreads) hidden_extremes_kernel(float* __restrict__ mean, int64_t HW, float* __restrict__ extremes,
                                                                      const float* __restrict__ ws, int groups, int64_t C) {
    kernarg_touch_for(mean, HW, extremes, ws, groups, C);
    __shared__ float red[3 * kExtThreads / 64];
    float* m = mean + (int64_t)blockIdx.x * HW;
    const int64_t B = gridDim.x;
    float lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    for (int64_t i = threadIdx.x; i < HW; i += kExtThreads) {
        float v;
        if (groups > 1) {
            v = ws[(int64_t)blockIdx.x * HW + i];
            for (int g = 1; g < groups; ++g) v += ws[((int64_t)g * B + blockIdx.x) * HW + i];
            v = v / (float)C;
            m[i] = v;
        } else {
            v = m[i];
        }
        nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax_nan<kExtThreads>(lo, hi, nan, red);  // a NaN poisons both
    if (threadIdx.x == 0) {
        extremes[2 * blockIdx.x] = nan_poisons(nan, lo);
        extremes[2 * blockIdx.x + 1] = nan_poisons(nan, hi);
    }
}

// ---- apply without a transform: PLAIN (f = x) and FILTERED (f from the fp32 temporary) -------------------------------------------------------
// item = V consecutive elements of one plane (HW % V == 0); lanes walk a plane's items, then the planes
template <int V, bool VEC>
__global__ void __launch_bounds__(kBlock) freeu_sweep_kernel(void* x, int dtype, int64_t HW, int64_t sb, int64_t sc, int64_t c0, int64_t cn,
                                                             int64_t planes, const float* __restrict__ filtered, Finish fin) {
    kernarg_touch_for(x, dtype, HW, sb, sc, c0, cn, planes, filtered, fin);
    const int64_t per_plane = HW / V, total = planes * per_plane;
    for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < total; it += (int64_t)gridDim.x * kBlock) {
        const int64_t plane = it / per_plane, p = (it - plane * per_plane) * V;
        const int64_t b = plane / cn, c = c0 + (plane - b * cn);
        const int64_t at = b * sb + c * sc + p;
        const SampleScale ss = sample_scale(fin, b);
        float orig[V], f[V], m[V], r[V];
        load_elems<V, VEC>(x, at, dtype, orig);
        if (filtered) load_f32<V, VEC>(filtered, plane * HW + p, f);
        if (fin.mean) load_f32<V, VEC>(fin.mean, b * HW + p, m);
#pragma unroll
        for (int k = 0; k < V; ++k) r[k] = finish_value(fin, ss, filtered ? f[k] : orig[k], orig[k], fin.mean ? m[k] : 0.0f);
        store_elems<V, VEC>(x, at, dtype, r);
    }
}

// ---- fused apply: one workgroup per plane, both transforms in LDS ----------------------------------------------------------------------------
// the run-time codelets are the plane kernel's (kSetSmall, 2 .. 12): with the 16-point codelet in the switch (kSetLines) this kernel spilled
// 6 vector and 300 scalar registers at its 128-register budget; a line of 128 or more then runs its second factor as direct sums
constexpr int kFreeuSet = kSetSmall;
// `V` elements (V / 2 complex values of a row) per item of the load and of the epilogue
template <int NT, int V, bool VEC>
__device__ __forceinline__ void plane_load(c32* A, const void* x, int64_t at, int dtype, int H, int M, int S, int tid) {
    constexpr int CV = V / 2;
    const int Mi = M / CV, W = 2 * M;  // items per row
    const int dr = NT / Mi, dm = NT - dr * Mi;
    int r = tid / Mi, mi = tid - r * Mi;
    for (int j = tid; j < H * Mi; j += NT) {
        float v[V];
        load_elems<V, VEC>(x, at + (int64_t)r * W + V * mi, dtype, v);
        c32* dst = A + r * S + CV * mi;
#pragma unroll
        for (int k = 0; k < CV; ++k) dst[k] = make_float2(v[2 * k], v[2 * k + 1]);
        r += dr;
        mi += dm;
        if (mi >= Mi) {
            mi -= Mi;
            ++r;
        }
    }
}
template <int NT, int V, bool VEC>
__device__ __forceinline__ void plane_finish(const c32* A, void* x, int64_t at, int dtype, int H, int M, int S, float inv_n, const Finish& fin,
                                             const SampleScale& ss, int64_t mean_at, int tid) {
    constexpr int CV = V / 2;
    const int Mi = M / CV, W = 2 * M;
    const int dr = NT / Mi, dm = NT - dr * Mi;
    int r = tid / Mi, mi = tid - r * Mi;
    for (int j = tid; j < H * Mi; j += NT) {
        const int64_t p = (int64_t)r * W + V * mi;
        float orig[V], m[V], o[V];
        load_elems<V, VEC>(x, at + p, dtype, orig);
        if (fin.mean) load_f32<V, VEC>(fin.mean, mean_at + p, m);
        const c32* src = A + r * S + CV * mi;
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const c32 g = src[k];
            o[2 * k] = finish_value(fin, ss, g.x * inv_n, orig[2 * k], fin.mean ? m[2 * k] : 0.0f);
            o[2 * k + 1] = finish_value(fin, ss, g.y * inv_n, orig[2 * k + 1], fin.mean ? m[2 * k + 1] : 0.0f);
        }
        store_elems<V, VEC>(x, at + p, dtype, o);
        r += dr;
        mi += dm;
        if (mi >= Mi) {
            mi -= Mi;
            ++r;
        }
    }
}

// access: 4 = four elements per item, one access each (M even, everything aligned to four elements), 2 = pairs, 0 = pairs, element by element
template <int NT>
__global__ void __launch_bounds__(NT, 4) freeu_fused_kernel(void* x, int dtype, int64_t sb, int64_t sc, int64_t c0, int64_t cn, int64_t planes,
                                                            AnyPlan pl, const float* __restrict__ filter, Finish fin, int access) {
    kernarg_touch_for(x, dtype, sb, sc, c0, cn, planes, pl, filter, fin, access);
    extern __shared__ __align__(16) unsigned char freeu_lds[];
    const int H = pl.H, M = pl.M, W = 2 * M, S = M + 1, NC = H * S;
    c32* const A = reinterpret_cast<c32*>(freeu_lds);
    c32* const twH = A + NC;   // e^{2 pi i j / H}
    c32* const twW = twH + H;  // e^{2 pi i j / W}
    const int tid = threadIdx.x;
    for (int j = tid; j < H + W; j += NT) {
        const int n = j < H ? H : W, i = j < H ? j : j - H;
        double sn, cs;
        sincospi(2.0 * (double)i / (double)n, &sn, &cs);
        twH[j] = make_float2((float)cs, (float)sn);
    }
    const float inv_n = 1.0f / ((float)H * (float)W);  // both transforms unscaled: ortho x ortho
    const int64_t HW = (int64_t)H * W;
    for (int64_t plane = blockIdx.x; plane < planes; plane += gridDim.x) {
        const int64_t b = plane / cn, c = c0 + (plane - b * cn);
        const int64_t at = b * sb + c * sc;
        __syncthreads();  // the previous plane's epilogue has read the buffer (and the twiddle tables are visible)
        if (access == 4) plane_load<NT, 4, true>(A, x, at, dtype, H, M, S, tid);
        else if (access == 2) plane_load<NT, 2, true>(A, x, at, dtype, H, M, S, tid);
        else plane_load<NT, 2, false>(A, x, at, dtype, H, M, S, tid);
        __syncthreads();
        // ---- forward r2c: rows as W/2 complex values, the split into the half-spectrum, forward columns, x filter (power_irfft2_any_kernel)
        line_dft<NT, true, 0, 0, kFreeuSet>(A, twW, W, 2, pl.mn1, pl.mn2, H, 1, S, tid);
        const int FQ = M / 2 + 1, fdr = NT / FQ, fdk = NT - fdr * FQ;
        int fr = tid / FQ, fk = tid - fr * FQ;
        for (int j = tid; j < H * FQ; j += NT) {
            const int r = fr, k = fk;
            fr += fdr;
            fk += fdk;
            if (fk >= FQ) {
                fk -= FQ;
                ++fr;
            }
            c32* row = A + r * S;
            if (k == 0) {
                const c32 q0 = row[0];
                row[0] = make_float2(q0.x + q0.y, 0.0f);
                row[M] = make_float2(q0.x - q0.y, 0.0f);
            } else {
                const int kk = M - k;
                const c32 a = row[k], bb = row[kk];
                const c32 e = make_float2(0.5f * (a.x + bb.x), 0.5f * (a.y - bb.y));
                const c32 o = make_float2(0.5f * (a.y + bb.y), -0.5f * (a.x - bb.x));
                const c32 w = twW[k];  // conj -> e^{-2 pi i k / W}
                const c32 t = make_float2(o.x * w.x + o.y * w.y, o.y * w.x - o.x * w.y);
                row[k] = make_float2(e.x + t.x, e.y + t.y);
                if (kk != k) row[kk] = make_float2(e.x - t.x, -(e.y - t.y));
            }
        }
        __syncthreads();
        line_dft<NT, true, 0, 0, kFreeuSet>(A, twH, H, 1, pl.hn1, pl.hn2, S, S, 1, tid);
        for (int j = tid; j < NC; j += NT) {
            const float f = filter[j];
            c32 v = A[j];
            v.x *= f;
            v.y *= f;
            A[j] = v;
        }
        __syncthreads();
        // ---- inverse: columns, then the rows' c2r pre-twiddle + length-M inverse; value m of a row is (x[2m], x[2m+1])
        line_dft<NT, false, 0, 0, kFreeuSet>(A, twH, H, 1, pl.hn1, pl.hn2, S, S, 1, tid);
        c2r_rows<NT, 0, 0, kFreeuSet>(A, twW, W, pl.mn1, pl.mn2, H, M, S, pl.c2r_fuse, tid);
        // ---- the whole plane is transformed: scale, blend with the original (read again), one rounding, in place
        const SampleScale ss = sample_scale(fin, b);
        if (access == 4) plane_finish<NT, 4, true>(A, x, at, dtype, H, M, S, inv_n, fin, ss, b * HW, tid);
        else if (access == 2) plane_finish<NT, 2, true>(A, x, at, dtype, H, M, S, inv_n, fin, ss, b * HW, tid);
        else plane_finish<NT, 2, false>(A, x, at, dtype, H, M, S, inv_n, fin, ss, b * HW, tid);
    }
}

// the widest item (4, 2, or 0 = element by element) every plane start of the window allows
static inline int access_width(const void* x, int dtype, int64_t sb, int64_t sc, int64_t row_elems) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(x);
    const int eb = elem_bytes(dtype);
    for (int v = 4; v >= 2; v -= 2)
        if (a % (uintptr_t)(v * eb) == 0 && sb % v == 0 && sc % v == 0 && row_elems % v == 0) return v;
    return 0;
}

}  // namespace freeu
}  // namespace sonar

using namespace sonar;
using namespace sonar::freeu;

extern "C" int64_t sonar_freeu_hidden_mean_groups(int64_t B, int64_t C, int64_t HW) {
    if (B <= 0 || C <= 0 || HW <= 0) return 1;
    // enough workgroups for two per CU, at least 32 channels (four per wave) in a group
    const int64_t blocks = B * ((HW + 63) / 64);
    const int64_t want = (512 + blocks - 1) / blocks, most = C / (4 * kMeanSlices);
    return std::max<int64_t>(1, std::min<int64_t>(std::min(want, most), kMeanMaxGroups));
}

extern "C" int sonar_freeu_hidden_mean(int dtype, const void* x, int64_t B, int64_t C, int64_t HW, int64_t stride_b, int64_t stride_c, float* mean,
                                       float* extremes, float* ws, int64_t ws_elems, void* stream) {
    SONAR_REQUIRE_DTYPE(dtype, "sonar_freeu_hidden_mean");
    SONAR_REQUIRE(B >= 0 && C > 0 && HW > 0 && stride_c >= HW && stride_b >= HW && ws_elems >= 0, SONAR_ERR_ARG,
                  "sonar_freeu_hidden_mean: bad shape or a stride smaller than the plane");
    SONAR_REQUIRE(HW <= ((int64_t)1 << 40) && B * ((HW + 63) / 64) < ((int64_t)1 << 31), SONAR_ERR_UNSUPPORTED,
                  "sonar_freeu_hidden_mean: more than 2^31 workgroups");
    if (B == 0) return SONAR_OK;
    SONAR_REQUIRE(x && mean && extremes, SONAR_ERR_ARG, "sonar_freeu_hidden_mean: null pointer");
    SONAR_REQUIRE(reinterpret_cast<uintptr_t>(x) % elem_bytes(dtype) == 0 && reinterpret_cast<uintptr_t>(mean) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(extremes) % 4 == 0 && reinterpret_cast<uintptr_t>(ws) % 4 == 0,
                  SONAR_ERR_ARG, "sonar_freeu_hidden_mean: misaligned buffer");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t chunks = (HW + 63) / 64;
    // the channel groups the workspace has room for (none: one group, the mean written directly)
    const int64_t room = ws ? ws_elems / (B * HW) : 0;
    int groups = (int)std::min<int64_t>(sonar_freeu_hidden_mean_groups(B, C, HW), room);
    if (groups < 2) groups = 1;
    const int64_t per_group = (C + groups - 1) / groups;
    groups = (int)((C + per_group - 1) / per_group);  // no empty group
    hipLaunchKernelGGL(hidden_mean_kernel, dim3((unsigned)(B * chunks), (unsigned)groups), dim3(kMeanThreads), 0, st, x, dtype, C, HW, stride_b,
                       stride_c, mean, chunks, ws, groups, per_group, B);
    hipLaunchKernelGGL(hidden_extremes_kernel, dim3((unsigned)B), dim3(kExtThreads), 0, st, mean, HW, extremes, (const float*)ws, groups, C);
    return check_launch("sonar_freeu_hidden_mean");
}

extern "C" int sonar_freeu_apply(int dtype, void* x, int64_t B, int64_t C, int64_t H, int64_t W, int64_t stride_b, int64_t stride_c, int64_t c0,
                                 int64_t cn, int mode, const float* filter, const float* filtered, const float* mean, const float* extremes,
                                 double scale, int blend_mode, float blend, void* stream) {
    SONAR_REQUIRE_DTYPE(dtype, "sonar_freeu_apply");
    SONAR_REQUIRE(mode >= SONAR_FREEU_PLAIN && mode <= SONAR_FREEU_FILTERED, SONAR_ERR_ARG, "sonar_freeu_apply: unknown mode %d", mode);
    SONAR_REQUIRE(blend_mode >= SONAR_CFG_BLEND_NONE && blend_mode <= SONAR_BLEND_SUBTRACT_B, SONAR_ERR_ARG,
                  "sonar_freeu_apply: unknown blend mode %d", blend_mode);
    SONAR_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && H <= (1 << 20) && W <= (1 << 20), SONAR_ERR_ARG, "sonar_freeu_apply: bad shape");
    const int64_t HW = H * W;
    SONAR_REQUIRE(stride_c >= HW && stride_b >= HW, SONAR_ERR_ARG, "sonar_freeu_apply: a stride smaller than the plane");
    SONAR_REQUIRE(c0 >= 0 && cn >= 0 && c0 + cn <= C, SONAR_ERR_ARG,
                  "sonar_freeu_apply: channel window [%lld, %lld) outside the %lld channels", (long long)c0, (long long)(c0 + cn), (long long)C);
    if (B == 0 || cn == 0) return SONAR_OK;
    SONAR_REQUIRE(x && (mode != SONAR_FREEU_FUSED || filter) && (mode != SONAR_FREEU_FILTERED || filtered) && (mean == nullptr || extremes),
                  SONAR_ERR_ARG, "sonar_freeu_apply: null pointer (the filter of FUSED, the temporary of FILTERED, extremes with a mean)");
    SONAR_REQUIRE(reinterpret_cast<uintptr_t>(x) % elem_bytes(dtype) == 0 && reinterpret_cast<uintptr_t>(filter) % 4 == 0 &&
                      reinterpret_cast<uintptr_t>(filtered) % 16 == 0 && reinterpret_cast<uintptr_t>(mean) % 16 == 0 &&
                      reinterpret_cast<uintptr_t>(extremes) % 4 == 0,
                  SONAR_ERR_ARG, "sonar_freeu_apply: misaligned buffer");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t planes = B * cn;
    const Finish fin{mean, extremes, (float)scale, (float)(scale - 1.0), blend_mode, blend};
    if (mode != SONAR_FREEU_FUSED) {
        const float* f = mode == SONAR_FREEU_FILTERED ? filtered : nullptr;
        const int v = access_width(x, dtype, stride_b, stride_c, HW);  // items stay inside a plane: HW % V == 0
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((planes * HW / std::max(v, 1) + kBlock - 1) / kBlock, kMaxGrid));
        if (v == 4) hipLaunchKernelGGL((freeu_sweep_kernel<4, true>), dim3(grid), dim3(kBlock), 0, st, x, dtype, HW, stride_b, stride_c, c0, cn, planes, f, fin);
        else if (v == 2) hipLaunchKernelGGL((freeu_sweep_kernel<2, true>), dim3(grid), dim3(kBlock), 0, st, x, dtype, HW, stride_b, stride_c, c0, cn, planes, f, fin);
        else hipLaunchKernelGGL((freeu_sweep_kernel<1, false>), dim3(grid), dim3(kBlock), 0, st, x, dtype, HW, stride_b, stride_c, c0, cn, planes, f, fin);
        return check_launch("sonar_freeu_apply");
    }
    const int kind = sonar_power_plane_kind(H, W);
    SONAR_REQUIRE((kind == 1 || kind == 2) && any_plane_ok(H, W), SONAR_ERR_UNSUPPORTED,
                  "sonar_freeu_apply: %lld x %lld is no LDS-resident plane (sonar_power_plane_kind 1 or 2): filter it first, then SONAR_FREEU_FILTERED",
                  (long long)H, (long long)W);
    AnyPlan pl;
    AnyShape sh;
    any_plan_fill(pl, sh, H, W, 0, 0, 0, 0, kFreeuSet);
    int access = access_width(x, dtype, stride_b, stride_c, W);
    if (access == 4 && (pl.M & 1)) access = 2;  // an item is whole complex values of ONE row
    const int grid = (int)std::min<int64_t>(planes, (int64_t)256 * sh.per_cu);
    if (sh.nt == kAnySlots) {
        auto kern = freeu_fused_kernel<kAnySlots>;
        lds_attr(reinterpret_cast<const void*>(kern), (int)kAnyLdsLimit);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kAnySlots), sh.lds, st, x, dtype, stride_b, stride_c, c0, cn, planes, pl, filter, fin, access);
    } else {
        auto kern = freeu_fused_kernel<kAnyThreads>;
        lds_attr(reinterpret_cast<const void*>(kern), (int)kAnyLdsLimit);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kAnyThreads), sh.lds, st, x, dtype, stride_b, stride_c, c0, cn, planes, pl, filter, fin, access);
    }
    return check_launch("sonar_freeu_apply");
}
