// Bislerp resampling (ComfyUI's comfy.utils.bislerp, which the reference reaches through common_upscale(..., "bislerp") and does not
// vendor: parity unpinned, the definition is restated in DESIGN.md and pinned by tests/bislerp_refs.py).  The C-vector of every pixel is
// resampled by spherical interpolation, first along the width, then along the height:
//     T[n, :, y, X] = slerp(S[n, :, y, c1w[X]], S[n, :, y, c2w[X]], rw[X])
//     O[n, :, Y, X] = slerp(T[n, :, c1h[Y], X], T[n, :, c2h[Y], X], rh[Y])
// One launch, no [N, C, h, W] intermediate: a thread owns an output pixel, evaluates the two width-pass slerps it needs (rows c1h[Y] and
// c2h[Y]) and then the height-pass slerp.  The axis tables come from the host (torch's own bilinear coordinates, hip_lib.bislerp_axis).
#include <algorithm>

#include "common.h"

namespace sonar {

// slerp(b1, b2, r) as coefficients: every branch of the definition is (p * (b1 / d1) + q * (b2 / d2)) * l
//     dot >  1 - 1e-5:  b1                       p = 1, q = 0, d = 1, l = 1   (exact: x / 1, x * 1, x + 0 * y)
//     dot < -1 + 1e-5:  b1 * (1 - r) + b2 * r    p = 1 - r, q = r, d = 1, l = 1
//     otherwise:        d = the norms (a zero norm gives the unit vector 0), p = sin((1 - r) om) / sin(om), q = sin(r om) / sin(om),
//                       l = n1 * (1 - r) + n2 * r
// The jump at the two thresholds is the definition's and is kept.
struct Slerp {
    float p, q, d1, d2, l;
    __device__ __forceinline__ float operator()(float b1, float b2) const { return (p * unit(b1, d1) + q * unit(b2, d2)) * l; }
    static __device__ __forceinline__ float unit(float b, float n) { return n == 0.0f ? 0.0f : b / n; }
};
__device__ __forceinline__ Slerp slerp_coef(float n1, float n2, float dot, float r) {
    const float hi = (float)(1.0 - 1e-5), lo = (float)(1e-5 - 1.0);  // the thresholds as an fp32 comparison sees them
    const float r1 = 1.0f - r;
    if (dot > hi) return Slerp{1.0f, 0.0f, 1.0f, 1.0f, 1.0f};
    if (dot < lo) return Slerp{r1, r, 1.0f, 1.0f, 1.0f};
    const float om = acosf(dot), so = sinf(om);
    return Slerp{sinf(r1 * om) / so, sinf(r * om) / so, n1, n2, n1 * r1 + n2 * r};
}

template <int CR, typename F>
__device__ __forceinline__ void for_channels(int C, F&& f) {
    if constexpr (CR > 0) {
#pragma unroll
        for (int c = 0; c < CR; ++c)
            if (c < C) f(c);
    } else {
        for (int c = 0; c < C; ++c) f(c);
    }
}

// CR > 0: C <= CR, the pixel's four source vectors and its two width-pass results stay in registers (every source value is read once);
// CR == 0: any C, the vectors are re-read from the (small, cached) source grid in each pass over the channels and the width-pass results
// recomputed -- nothing is sized by a channel count.
template <int CR, bool STATS>
__global__ void __launch_bounds__(kBlock) bislerp_acc_kernel(float* dst, const float* __restrict__ src, int64_t N, int C, int H, int W, int h, int w,
                                                             float scale, int accumulate, const int* __restrict__ c1w,
                                                             const int* __restrict__ c2w, const float* __restrict__ rw,
                                                             const int* __restrict__ c1h, const int* __restrict__ c2h,
                                                             const float* __restrict__ rh, double* partials) {
    kernarg_touch_for(dst, src, N, C, H, W, h, w, scale, accumulate, c1w, c2w, rw, c1h, c2h, rh, partials);
    __shared__ double red[2 * kBlock / 64];
    constexpr int NR = CR > 0 ? CR : 1;
    double s = 0.0, q = 0.0;
    const int64_t total = N * H * W, hw = (int64_t)h * w, HW = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int X = (int)(i % W);
        const int Y = (int)((i / W) % H);
        const int64_t n = i / HW;
        // (clamped: a table built for another size cannot make the kernel read outside the grid)
        const int xa = min(max(c1w[X], 0), w - 1), xb = min(max(c2w[X], 0), w - 1);
        const int ya = min(max(c1h[Y], 0), h - 1), yb = min(max(c2h[Y], 0), h - 1);
        const float fw = rw[X], fh = rh[Y];
        const float* const base = src + n * C * hw;
        const float* const ptr[4] = {base + (int64_t)ya * w + xa, base + (int64_t)ya * w + xb, base + (int64_t)yb * w + xa,
                                     base + (int64_t)yb * w + xb};
        float reg[4][NR], t[2][NR];
        if constexpr (CR > 0) {
            for_channels<CR>(C, [&](int c) {
#pragma unroll
                for (int k = 0; k < 4; ++k) reg[k][c] = ptr[k][c * hw];
            });
        }
        auto S = [&](int k, int c) { return CR > 0 ? reg[k][CR > 0 ? c : 0] : ptr[k][c * hw]; };
        // width pass, rows ya (vectors 0, 1) and yb (vectors 2, 3)
        float sq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for_channels<CR>(C, [&](int c) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = S(k, c);
                sq[k] += v * v;
            }
        });
        float nr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) nr[k] = sqrtf(sq[k]);
        float da = 0.0f, db = 0.0f;
        for_channels<CR>(C, [&](int c) {
            da += Slerp::unit(S(0, c), nr[0]) * Slerp::unit(S(1, c), nr[1]);
            db += Slerp::unit(S(2, c), nr[2]) * Slerp::unit(S(3, c), nr[3]);
        });
        const Slerp sa = slerp_coef(nr[0], nr[1], da, fw), sb = slerp_coef(nr[2], nr[3], db, fw);
        // height pass on the two results
        float ta2 = 0.0f, tb2 = 0.0f;
        for_channels<CR>(C, [&](int c) {
            const float a = sa(S(0, c), S(1, c)), b = sb(S(2, c), S(3, c));
            if constexpr (CR > 0) {
                t[0][c] = a;
                t[1][c] = b;
            }
            ta2 += a * a;
            tb2 += b * b;
        });
        auto TA = [&](int c) { return CR > 0 ? t[0][CR > 0 ? c : 0] : sa(S(0, c), S(1, c)); };
        auto TB = [&](int c) { return CR > 0 ? t[1][CR > 0 ? c : 0] : sb(S(2, c), S(3, c)); };
        const float na = sqrtf(ta2), nb = sqrtf(tb2);
        float dt = 0.0f;
        for_channels<CR>(C, [&](int c) { dt += Slerp::unit(TA(c), na) * Slerp::unit(TB(c), nb); });
        const Slerp so = slerp_coef(na, nb, dt, fh);
        float* const o = dst + n * C * HW + (int64_t)Y * W + X;
        for_channels<CR>(C, [&](int c) {
            float v = so(TA(c), TB(c));
            if (scale != 1.0f) v = v * scale;
            if (accumulate) v = o[c * HW] + v;
            o[c * HW] = v;
            if constexpr (STATS) {
                const double d = v;
                s += d;
                q += d * d;
            }
        });
    }
    if constexpr (STATS) write_partial<kBlock>(s, q, partials, red);
}

template <int CR>
static void bislerp_launch(int g, hipStream_t st, float* dst, const float* src, int64_t N, int C, int H, int W, int h, int w, float scale,
                           int accumulate, const int* c1w, const int* c2w, const float* rw, const int* c1h, const int* c2h, const float* rh,
                           double* partials) {
    if (partials)
        hipLaunchKernelGGL((bislerp_acc_kernel<CR, true>), dim3(g), dim3(kBlock), 0, st, dst, src, N, C, H, W, h, w, scale, accumulate, c1w, c2w, rw,
                           c1h, c2h, rh, partials);
    else
        hipLaunchKernelGGL((bislerp_acc_kernel<CR, false>), dim3(g), dim3(kBlock), 0, st, dst, src, N, C, H, W, h, w, scale, accumulate, c1w, c2w, rw,
                           c1h, c2h, rh, partials);
}

}  // namespace sonar

using namespace sonar;

extern "C" int sonar_bislerp_acc_f32(float* dst, const float* src, int64_t N, int64_t C, int64_t H, int64_t W, int64_t h, int64_t w, float scale,
                                     int accumulate, const int32_t* c1w, const int32_t* c2w, const float* rw, const int32_t* c1h,
                                     const int32_t* c2h, const float* rh, double* partials, void* stream) {
    SONAR_REQUIRE(dst && src && N >= 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0 && c1w && c2w && rw && c1h && c2h && rh, SONAR_ERR_ARG,
                  "sonar_bislerp_acc_f32: bad argument");
    SONAR_REQUIRE(H < (1 << 24) && W < (1 << 24) && h < (1 << 24) && w < (1 << 24) && C < (1 << 24), SONAR_ERR_UNSUPPORTED,
                  "sonar_bislerp_acc_f32: plane or channel count too large");
    if (N == 0) return SONAR_OK;
    const int g = (int)std::min<int64_t>(kNPart, grid_for(N * H * W, kBlock));
    hipStream_t st = (hipStream_t)stream;
    if (C <= 4)
        bislerp_launch<4>(g, st, dst, src, N, (int)C, (int)H, (int)W, (int)h, (int)w, scale, accumulate, c1w, c2w, rw, c1h, c2h, rh, partials);
    else if (C <= 16)
        bislerp_launch<16>(g, st, dst, src, N, (int)C, (int)H, (int)W, (int)h, (int)w, scale, accumulate, c1w, c2w, rw, c1h, c2h, rh, partials);
    else
        bislerp_launch<0>(g, st, dst, src, N, (int)C, (int)H, (int)W, (int)h, (int)w, scale, accumulate, c1w, c2w, rw, c1h, c2h, rh, partials);
    return check_launch("sonar_bislerp_acc_f32");
}
