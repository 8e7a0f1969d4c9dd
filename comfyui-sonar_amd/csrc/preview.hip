// Filter previews of SonarPowerNoise / SonarPowerFilterNoise (py/nodes/powernoise.py:268-294, 410-468): the picture the node shows while a
// filter is tuned.  Two or three panels side by side, one launch per image:
//   filter panel  tanh(filter_gain * F) * 256, F = rfft2_to_fft2(filter): the half-spectrum [H][Wh] fft-shifted along the rows on the right,
//                 its mirror image (both axes flipped, one more row of roll for an even H) on the left.  The mirrored half drops column 0
//                 always and the last column only when Wh is odd: L = Wh - 2 (Wh odd) or Wh - 1 (Wh even) columns, FW = L + Wh in all --
//                 W = 6 gives 7 columns, W = 9 gives 8.  The reference's widths, kept.
//   kernel panel  (tanh(kernel_gain * k) + 1) * 128, k = irfft2(filter) rolled by (H/2, W/2)
//   noise panel   (tanh(n * (1/3)) + 1) * 128
// Every roll, flip and concatenation is addressing: a lane owns four consecutive values of the output (flat over planes, rows and columns),
// finds each one's panel and source element, and stores them as one 16-byte (fp32) or one 4-byte (uint8: clamp(0, 255), truncated) access;
// the last, partial group of the buffer is stored value by value.  No LDS, nothing shared between lanes.  Every product and sum is rounded
// on its own (-ffp-contract=off), in the reference's order.
#include <math.h>

#include "common.h"

namespace sonar {

struct PreviewArgs {
    const float* filt;   // [planes][H][Wh]
    const float* kern;   // [planes][H][W]; null: no kernel panel
    const float* noise;  // [planes][H][W]; null: no noise panel
    void* out;           // [planes][H][TW], float or uint8_t
    int64_t total;       // planes * H * TW
    int H, W, Wh;
    int L, FW, KW, TW;   // mirrored columns, filter panel, kernel panel (W or 0) and image widths
    int gain;            // 0: the panels' source values as they are (rfft2_to_fft2 and the rolled kernel: data movement only)
    float filter_gain, kernel_gain;
};

__device__ __forceinline__ float preview_value(const PreviewArgs& a, int64_t plane, int r, int c) {
    const int half = a.H >> 1;
    if (c < a.FW) {
        int sr, sc;
        if (c < a.L) {  // mirrored half: row H - 1 - (r - 1 mod H) for an even H, H - 1 - r for an odd one, of the shifted rows
            const int back = (a.H & 1) ? r : (r == 0 ? a.H - 1 : r - 1);
            sr = a.H - 1 - back - half;
            sc = a.L - c;  // 1 .. L
        } else {
            sr = r - half;
            sc = c - a.L;  // 0 .. Wh - 1
        }
        if (sr < 0) sr += a.H;
        const float f = a.filt[(plane * a.H + sr) * a.Wh + sc];
        return a.gain ? __fmul_rn(tanhf(__fmul_rn(f, a.filter_gain)), 256.0f) : f;
    }
    c -= a.FW;
    if (c < a.KW) {
        int sr = r - half, sc = c - (a.W >> 1);
        if (sr < 0) sr += a.H;
        if (sc < 0) sc += a.W;
        const float k = a.kern[(plane * a.H + sr) * a.W + sc];
        return a.gain ? __fmul_rn(__fadd_rn(tanhf(__fmul_rn(k, a.kernel_gain)), 1.0f), 128.0f) : k;
    }
    c -= a.KW;
    const float n = a.noise[(plane * a.H + r) * a.W + c];
    return a.gain ? __fmul_rn(__fadd_rn(tanhf(__fmul_rn(n, (float)(1.0 / 3.0))), 1.0f), 128.0f) : n;
}

__device__ __forceinline__ uint32_t grey_level(float v) { return (uint32_t)fminf(fmaxf(v, 0.0f), 255.0f); }  // clamp(0, 255).to(uint8)

// OUT: float or uint8_t.  VEC: the buffer starts on a 16-byte (float) / 4-byte (uint8_t) boundary, whole groups go out as one store.
template <typename OUT, bool VEC>
__global__ void __launch_bounds__(kBlock) preview_panels_kernel(PreviewArgs a) {
    kernarg_touch_for(a);
    OUT* __restrict__ out = static_cast<OUT*>(a.out);
    const int64_t groups = (a.total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (int64_t)gridDim.x * kBlock) {
        const int64_t first = g << 2;
        const int64_t line = first / a.TW;  // plane * H + row
        int64_t plane = line / a.H;
        int r = (int)(line - plane * a.H), c = (int)(first - line * a.TW);
        const int count = (int)(a.total - first < 4 ? a.total - first : 4);  // tail guarded: first + j < total
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < count) {
                v[j] = preview_value(a, plane, r, c);
                if (++c == a.TW) {
                    c = 0;
                    if (++r == a.H) {
                        r = 0;
                        ++plane;
                    }
                }
            }
        }
        if constexpr (sizeof(OUT) == 4) {
            if (VEC && count == 4) {
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + first) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < count) out[first + j] = (OUT)v[j];
            }
        } else {
            if (VEC && count == 4) {
                const uint32_t packed = grey_level(v[0]) | (grey_level(v[1]) << 8) | (grey_level(v[2]) << 16) | (grey_level(v[3]) << 24);
                *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(out) + first) = packed;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < count) out[first + j] = (OUT)grey_level(v[j]);
            }
        }
    }
}

static int preview_launch(const char* what, bool u8, const float* filter, const float* kernel, const float* noise, int64_t planes, int64_t H, int64_t W,
                          int64_t noise_h, int64_t noise_w, float filter_gain, float kernel_gain, int gain, void* out, void* stream) {
    // the noise plane's size travels with its pointer: both or neither, and the image's own size
    const bool noise_ok = noise ? (noise_h == H && noise_w == W) : (noise_h == 0 && noise_w == 0);
    // only the data-movement form (gain == 0) may leave the kernel plane out: rfft2_to_fft2 alone
    const bool kernel_ok = kernel != nullptr || (gain == 0 && noise == nullptr);
    if (!(filter && out && kernel_ok && noise_ok && planes >= 1 && H >= 2 && W >= 2 && H <= (1 << 20) && W <= (1 << 20))) {
        set_error("%s: bad argument", what);
        return SONAR_ERR_ARG;
    }
    PreviewArgs a;
    a.filt = filter; a.kern = kernel; a.noise = noise; a.out = out;
    a.H = (int)H; a.W = (int)W; a.Wh = (int)(W / 2 + 1);
    a.L = (a.Wh & 1) ? a.Wh - 2 : a.Wh - 1;
    a.FW = a.L + a.Wh;
    a.KW = kernel ? a.W : 0;
    a.TW = a.FW + a.KW + (noise ? a.W : 0);
    a.total = planes * H * (int64_t)a.TW;
    a.gain = gain != 0; a.filter_gain = filter_gain; a.kernel_gain = kernel_gain;
    const dim3 grid(grid_for((a.total + 3) / 4, kBlock)), block(kBlock);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & (u8 ? 3u : 15u)) == 0;
    if (u8) {
        if (vec) hipLaunchKernelGGL((preview_panels_kernel<uint8_t, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((preview_panels_kernel<uint8_t, false>), grid, block, 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((preview_panels_kernel<float, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((preview_panels_kernel<float, false>), grid, block, 0, st, a);
    }
    return check_launch(what);
}

}  // namespace sonar

using namespace sonar;

extern "C" int sonar_preview_panels_f32(const float* filter, const float* kernel, const float* noise, int64_t planes, int64_t H, int64_t W,
                                        int64_t noise_h, int64_t noise_w, float filter_gain, float kernel_gain, int gain, float* out,
                                        void* stream) {
    return preview_launch("sonar_preview_panels_f32", false, filter, kernel, noise, planes, H, W, noise_h, noise_w, filter_gain, kernel_gain, gain,
                          out, stream);
}

extern "C" int sonar_preview_compose_u8(const float* filter, const float* kernel, const float* noise, int64_t planes, int64_t H, int64_t W,
                                        int64_t noise_h, int64_t noise_w, float filter_gain, float kernel_gain, uint8_t* out, void* stream) {
    return preview_launch("sonar_preview_compose_u8", true, filter, kernel, noise, planes, H, W, noise_h, noise_w, filter_gain, kernel_gain, 1, out,
                          stream);
}
