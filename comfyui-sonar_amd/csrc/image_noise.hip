// SonarNoiseImage (py/nodes/misc.py:158-357): the image side of the node.  The noise arrives as the sampler made it, NCHW fp32; the image
// is a ComfyUI IMAGE, NHWC.  One launch of the compose kernel does, per value and in the reference's order: normalize_to_scale of the noise
// between its per-sample extremes -> * multiplier -> blend into the target channels -> clip (clamp mode) or per-sample min / max partials of
// the unclipped image (rescale mode; a second launch then rescales the NHWC image in place).  Greyscale mode folds the channel mean BEFORE
// the min / max the rescale needs, so a first small kernel writes the mean plane (1/C of the noise) and the compose kernel reads that one
// plane for every channel.  Everything is HBM-bound: one lane owns one pixel, the C noise planes are read as C coalesced dword streams, the
// pixel is read and written as one 16-byte access for C = 4 and as C consecutive dwords otherwise (a wave's accesses cover one contiguous
// run of 64 * C * 4 bytes).  Every product and sum is rounded on its own (-ffp-contract=off, and the explicit _rn forms where the sequence
// is normalize_to_scale's): the result has the reference's bits on top of the same noise.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "range_reduce.h"

namespace sonar {

// blocks per sample of the compose launch == min / max partial slots per sample that the rescale launch reduces
static inline int image_parts(int64_t plane) { return (int)std::max<int64_t>(1, std::min<int64_t>((plane + kBlock - 1) / kBlock, SONAR_IMAGE_NPART)); }

struct ComposeArgs {
    const float* noise;            // [batch][greyscale ? 1 : channels][plane]
    const float *noise_lo, *noise_hi;  // [batch] extremes of the noise (of the mean plane in greyscale mode); null: no normalize_to_scale
    const float* image;            // [batch][plane][channels]; null: zeros (pure noise)
    float* out;                    // [batch][plane][channels]
    float *part_min, *part_max;    // rescale mode: [batch][SONAR_IMAGE_NPART]
    int64_t plane;
    uint64_t mask;                 // bit c: channel c is a blend target
    int channels, greyscale, blend_mode;
    float tmin, tmax, span, eps, multiplier, strength;
};

// normalize_to_scale's value sequence (minmax_rescale_by, common.h), then `result *= noise_multiplier`
__device__ __forceinline__ float prepare_noise(float n, bool normalize, float lo, float denom, const ComposeArgs& a) {
    if (normalize) n = minmax_rescale_by(n, lo, denom, a.tmin, a.tmax, a.span);
    return __fmul_rn(n, a.multiplier);
}

__device__ __forceinline__ float blend_image(int mode, float img, float n, float t) {
    return mode == SONAR_IMAGE_BLEND_ADD ? __fadd_rn(img, n) : blend<float>(mode, img, n, t);
}

__device__ __forceinline__ float clip01(float v) { return v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f); }  // clip_ keeps NaN

// block-wide (min, max) of the values the block wrote -> its partial slot; a NaN never wins
__device__ __forceinline__ void write_minmax_part(float lo, float hi, float* part_min, float* part_max, int64_t slot) {
    __shared__ float red[2 * kBlock / 64];
    block_minmax<kBlock>(lo, hi, red);
    if (threadIdx.x == 0) {
        part_min[slot] = lo;
        part_max[slot] = hi;
    }
}

// CT: channel count known at compile time (3, 4: one lane owns one pixel, its channels in registers), 0: any count, a plain strided loop.
// grid = (image_parts(plane), batch); a block strides over the pixels of ONE sample, so its min / max belong to that sample.
template <int CT, bool CLAMP>
__global__ void __launch_bounds__(kBlock) image_compose_kernel(ComposeArgs a) {
    kernarg_touch_for(a);
    const int64_t b = blockIdx.y;
    const int C = CT ? CT : a.channels;
    const int64_t nstride = a.greyscale ? 0 : a.plane;  // greyscale: every channel reads the one mean plane
    const float* __restrict__ nz = a.noise + b * (a.greyscale ? 1 : C) * a.plane;
    const float* __restrict__ img = a.image ? a.image + b * a.plane * C : nullptr;
    float* __restrict__ out = a.out + b * a.plane * C;
    const bool normalize = a.noise_lo != nullptr;
    float lo = 0.0f, denom = 1.0f;
    if (normalize) {
        lo = a.noise_lo[b];
        denom = minmax_rescale_denom(lo, a.noise_hi[b], a.eps);
    }
    float vlo = INFINITY, vhi = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < a.plane; p += stride) {  // tail guarded: p < plane
        if constexpr (CT != 0) {
            float n[CT], px[CT];
            if (a.greyscale) {
                const float g = prepare_noise(nz[p], normalize, lo, denom, a);
#pragma unroll
                for (int c = 0; c < CT; ++c) n[c] = g;
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c) n[c] = prepare_noise(nz[c * nstride + p], normalize, lo, denom, a);
            }
            if (img == nullptr) {
#pragma unroll
                for (int c = 0; c < CT; ++c) px[c] = 0.0f;
            } else if constexpr (CT == 4) {
                const float4 t = reinterpret_cast<const float4*>(img)[p];
                px[0] = t.x; px[1] = t.y; px[2] = t.z; px[3] = t.w;
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c) px[c] = img[p * CT + c];
            }
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                float v = (a.mask >> c) & 1u ? blend_image(a.blend_mode, px[c], n[c], a.strength) : px[c];
                if constexpr (CLAMP) {
                    v = clip01(v);
                } else {
                    vlo = fminf(vlo, v);
                    vhi = fmaxf(vhi, v);
                }
                px[c] = v;
            }
            if constexpr (CT == 4) {
                reinterpret_cast<float4*>(out)[p] = make_float4(px[0], px[1], px[2], px[3]);
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c) out[p * CT + c] = px[c];
            }
        } else {
            for (int c = 0; c < C; ++c) {
                const float n = prepare_noise(nz[c * nstride + p], normalize, lo, denom, a);
                const float s = img ? img[p * C + c] : 0.0f;
                float v = (a.mask >> c) & 1u ? blend_image(a.blend_mode, s, n, a.strength) : s;
                if constexpr (CLAMP) {
                    v = clip01(v);
                } else {
                    vlo = fminf(vlo, v);
                    vhi = fmaxf(vhi, v);
                }
                out[p * C + c] = v;
            }
        }
    }
    if constexpr (!CLAMP) write_minmax_part(vlo, vhi, a.part_min, a.part_max, b * SONAR_IMAGE_NPART + blockIdx.x);
}

// result.mean(dim=1): torch's sum over a strided dimension adds the channels in order, the mean is a true division by C
__global__ void __launch_bounds__(kBlock) image_channel_mean_kernel(const float* __restrict__ noise, int64_t batch, int channels, int64_t plane,
                                                                     float* __restrict__ out) {
    kernarg_touch_for(noise, batch, channels, plane, out);
    const int64_t total = batch * plane;
    const float div = (float)channels;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = i / plane, p = i - b * plane;
        const float* src = noise + b * channels * plane + p;
        float s = src[0];
        for (int c = 1; c < channels; ++c) s = __fadd_rn(s, src[c * plane]);
        out[i] = s / div;
    }
}

// normalize_to_scale(image, 0, 1) over each sample of the NHWC image, in place: the sample's extremes from the compose launch's partial
// slots (every block reduces the <= SONAR_IMAGE_NPART pairs of its sample: 8 KB out of the L2), then minmax_rescale_kernel's sequence
__global__ void __launch_bounds__(kBlock) image_rescale_kernel(float* __restrict__ image, int64_t per_sample, const float* __restrict__ part_min,
                                                                const float* __restrict__ part_max, int parts, float eps) {
    kernarg_touch_for(image, per_sample, part_min, part_max, parts, eps);
    __shared__ float red[2 * kBlock / 64];
    const int64_t b = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < parts; i += kBlock) {
        lo = fminf(lo, part_min[b * SONAR_IMAGE_NPART + i]);
        hi = fmaxf(hi, part_max[b * SONAR_IMAGE_NPART + i]);
    }
    block_minmax<kBlock>(lo, hi, red);  // a NaN never wins
    const float denom = minmax_rescale_denom(lo, hi, eps);
    // targets 0 and 1: the `* 1.0f + 0.0f` steps of the sequence are kept (a -0 becomes +0 as in the reference)
    auto rescale = [&](float x) { return minmax_rescale_by(x, lo, denom, 0.0f, 1.0f, 1.0f); };
    float* row = image + b * per_sample;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    if ((reinterpret_cast<uintptr_t>(row) & 15u) == 0 && (per_sample & 3) == 0) {
        float4* row4 = reinterpret_cast<float4*>(row);
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < (per_sample >> 2); i += stride) {
            float4 v = row4[i];
            v.x = rescale(v.x); v.y = rescale(v.y); v.z = rescale(v.z); v.w = rescale(v.w);
            row4[i] = v;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < per_sample; i += stride) row[i] = rescale(row[i]);
    }
}

}  // namespace sonar

using namespace sonar;

extern "C" int sonar_image_channel_mean_f32(const float* noise, int64_t batch, int64_t channels, int64_t plane, float* out, void* stream) {
    SONAR_REQUIRE(noise && out && batch >= 0 && channels > 0 && channels <= SONAR_IMAGE_MAX_CHANNELS && plane >= 0, SONAR_ERR_ARG,
                  "sonar_image_channel_mean_f32: bad argument");
    if (batch * plane == 0) return SONAR_OK;
    hipLaunchKernelGGL(image_channel_mean_kernel, dim3(grid_for(batch * plane, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, noise, batch,
                       (int)channels, plane, out);
    return check_launch("sonar_image_channel_mean_f32");
}

extern "C" int sonar_image_noise_compose_f32(const float* noise, const float* noise_lo, const float* noise_hi, double noise_min, double noise_max,
                                             float eps, float multiplier, int greyscale, int blend_mode, float blend_strength,
                                             uint64_t channel_mask, const float* image, float* out, int64_t batch, int64_t channels,
                                             int64_t plane, int clamp, float* part_min, float* part_max, void* stream) {
    SONAR_REQUIRE(noise && out && batch >= 0 && batch <= 65535 && channels > 0 && channels <= SONAR_IMAGE_MAX_CHANNELS && plane >= 0 &&
                      blend_mode >= 0 && blend_mode <= SONAR_IMAGE_BLEND_ADD && (noise_lo == nullptr) == (noise_hi == nullptr) &&
                      (clamp || (part_min && part_max)),
                  SONAR_ERR_ARG, "sonar_image_noise_compose_f32: bad argument");
    if (batch * plane == 0) return SONAR_OK;
    ComposeArgs a;
    a.noise = noise; a.noise_lo = noise_lo; a.noise_hi = noise_hi; a.image = image; a.out = out;
    a.part_min = part_min; a.part_max = part_max;
    a.plane = plane; a.mask = channel_mask;
    a.channels = (int)channels; a.greyscale = greyscale != 0; a.blend_mode = blend_mode;
    // the targets are Python floats in the reference: their difference is formed in double and rounded to fp32 once
    a.tmin = (float)noise_min; a.tmax = (float)noise_max; a.span = (float)(noise_max - noise_min);
    a.eps = eps; a.multiplier = multiplier; a.strength = blend_strength;
    const dim3 grid(image_parts(plane), (unsigned)batch), block(kBlock);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec4 = channels == 4 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (reinterpret_cast<uintptr_t>(image) & 15u) == 0;
#define SONAR_COMPOSE(CT) \
    do { \
        if (clamp) hipLaunchKernelGGL((image_compose_kernel<CT, true>), grid, block, 0, st, a); \
        else hipLaunchKernelGGL((image_compose_kernel<CT, false>), grid, block, 0, st, a); \
    } while (0)
    if (vec4) SONAR_COMPOSE(4);
    else if (channels == 3) SONAR_COMPOSE(3);
    else SONAR_COMPOSE(0);
#undef SONAR_COMPOSE
    return check_launch("sonar_image_noise_compose_f32");
}

extern "C" int sonar_image_rescale_f32(float* image, int64_t batch, int64_t channels, int64_t plane, const float* part_min, const float* part_max,
                                       float eps, void* stream) {
    SONAR_REQUIRE(image && part_min && part_max && batch >= 0 && batch <= 65535 && channels > 0 && plane >= 0, SONAR_ERR_ARG,
                  "sonar_image_rescale_f32: bad argument");
    if (batch * plane == 0) return SONAR_OK;
    const int64_t per_sample = channels * plane;
    const dim3 grid(std::min(grid_for(per_sample / 4 + 1, kBlock), SONAR_IMAGE_NPART), (unsigned)batch);
    hipLaunchKernelGGL(image_rescale_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, image, per_sample, part_min, part_max, image_parts(plane),
                       eps);
    return check_launch("sonar_image_rescale_f32");
}
