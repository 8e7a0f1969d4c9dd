// One layer of the dual-tree scattering network the reference reaches through pytorch_wavelets' ScatLayer (py/noise_generation.py:2035-2193):
// the level-1 DTCWT (csrc/dtcwt.hip runs it as six axis_taps launches and a q2c), the smoothed magnitude sqrt(re^2 + im^2 + b^2) - b of the
// six oriented bands, the 2x2 mean of the low-pass, all seven concatenated band-major: out[b][band * C + c].  Fused: one launch reads the
// input once plus a halo and writes only the channels of the window (k0, nk) the caller keeps -- the noise item keeps C of the 7 C.
//
// One workgroup per (output tile, band group, input plane).  The groups are {ll}, {15, 165}, {45, 135}, {75, 105} degrees: the two bands of
// a pair are the two complex combinations of the same quads of ONE doubly filtered plane, and each group needs ONE row-filtered plane
// (low-pass rows for ll and lh, high-pass rows for hh and hl), so a workgroup
//   1. stages its input tile plus the halo of its two filters in LDS (consecutive lanes on consecutive addresses; the symmetric extension
//      and the repeated last row / column of an odd plane live in the index function, scat_fold),
//   2. runs the row filter from LDS into LDS (a lane per column: conflict-free 4-byte reads),
//   3. runs the column filter per output quad in registers: a lane reads the two columns of its quad as one 8-byte LDS read per row -- 32
//      lanes cover one 256-byte bank row, the other half-wave is another row pair and another lane group, so no conflicts --
//   4. combines the quad (mean, or the two complex pairs and their magnitudes) and stores: a half-wave writes 128 consecutive bytes.
// A workgroup whose bands lie outside the window returns before it loads anything.  Filter lengths are template parameters (the three
// banks of py/dtcwt.py's biort_filters); the taps themselves are arguments, taken from that function's tables by the caller.
//
// The magnitude is evaluated as s / (sqrt(s + b^2) + b) with s = re^2 + im^2: the same value as sqrt(s + b^2) - b without the
// cancellation, whose rounding error is of the size of b, not of the band (it matters for |x| << b).
#include <hip/hip_runtime.h>

#include "common.h"

namespace sonar {

constexpr int kScatTileH = SONAR_SCAT_TILE_H, kScatTileW = SONAR_SCAT_TILE_W;  // output values per tile: 2 x as many input rows / columns
constexpr int kScatInH = 2 * kScatTileH, kScatInW = 2 * kScatTileW;
static_assert(kScatInW == 64 && (kScatTileH * kScatTileW) % kBlock == 0, "a row of the row-filtered tile is one 256-byte bank row");

struct ScatTaps {
    float h0[9];  // low-pass h0o, the first L0 used
    float h1[7];  // high-pass h1o, the first L1 used
};

struct ScatArgs {
    const float* x;
    float* out;
    int64_t planes;  // B * C
    int C, H, W;     // the plane as it lies
    int He, We;      // extended to even
    int tiles_x, tiles_y;
    int groups[4], ngroups;  // the band groups the window touches
    int64_t k0, nk;
    float bias;
    ScatTaps taps;
};

// Position i of the even-length (ne) signal extended with half-sample symmetry, any integer i (the full modular fold: a halo may be longer
// than the plane), then onto the stored samples: an odd plane's last sample stands for the one appended to make it even.
__device__ __forceinline__ int scat_fold(int i, int ne, int n) {
    if ((unsigned)i >= (unsigned)ne) {
        const int p = 2 * ne;
        int t = i % p;
        if (t < 0) t += p;
        i = t >= ne ? p - 1 - t : t;
    }
    return i < n ? i : n - 1;
}

__device__ __forceinline__ float scat_mag(float re, float im, float b) {
    const float s = fmaf(re, re, im * im);
    const float den = sqrtf(fmaf(b, b, s)) + b;
    return den == 0.0f ? 0.0f : s / den;
}

// LR / LC: lengths of the row and column filter; PAIR: the group is a pair of oriented bands (otherwise the pooled low-pass)
template <int LR, int LC, bool PAIR, int LMAX>
__device__ __forceinline__ void scat_tile(const ScatArgs& a, const float* __restrict__ hr, const float* __restrict__ hc, const float* __restrict__ src,
                                          float* dst1, float* dst2, int ty, int tx, float* stage, float* rowed) {
    constexpr int MR = LR / 2, MC = LC / 2;
    constexpr int SW = kScatInW + 2 * MR, SH = kScatInH + 2 * MC;
    static_assert(SW <= kScatInW + LMAX - 1 && SH <= kScatInH + LMAX - 1, "the LDS arrays hold the longest filter's halo");
    const int gy0 = ty * kScatInH - MC, gx0 = tx * kScatInW - MR;
    for (int e = threadIdx.x; e < SH * SW; e += kBlock) {
        const int r = e / SW, c = e - r * SW;
        const int y = scat_fold(gy0 + r, a.He, a.H), x = scat_fold(gx0 + c, a.We, a.W);
        stage[e] = src[(int64_t)y * a.W + x];
    }
    __syncthreads();
    // rows: rowed[r][c] = sum_k hr[k] * ext[r][c + MR - k]; stage column = extended column - gx0
    for (int e = threadIdx.x; e < SH * kScatInW; e += kBlock) {
        const int r = e / kScatInW, c = e - r * kScatInW;
        const float* s = stage + r * SW + c;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < LR; ++k) acc = fmaf(hr[k], s[2 * MR - k], acc);
        rowed[e] = acc;
    }
    __syncthreads();
    const int Ho = a.He / 2, Wo = a.We / 2;
#pragma unroll
    for (int j = 0; j < kScatTileH * kScatTileW / kBlock; ++j) {
        const int q = threadIdx.x + j * kBlock;
        const int oy = q / kScatTileW, ox = q - oy * kScatTileW;
        // the LC + 1 rows under the quad's two output rows, both columns in one 8-byte read
        float2 v[LC + 1];
#pragma unroll
        for (int t = 0; t <= LC; ++t) v[t] = *reinterpret_cast<const float2*>(rowed + (2 * oy + t) * kScatInW + 2 * ox);
        float qa = 0.0f, qb = 0.0f, qc = 0.0f, qd = 0.0f;  // a b / c d
#pragma unroll
        for (int k = 0; k < LC; ++k) {
            qa = fmaf(hc[k], v[2 * MC - k].x, qa);
            qb = fmaf(hc[k], v[2 * MC - k].y, qb);
            qc = fmaf(hc[k], v[2 * MC - k + 1].x, qc);
            qd = fmaf(hc[k], v[2 * MC - k + 1].y, qd);
        }
        const int gy = ty * kScatTileH + oy, gx = tx * kScatTileW + ox;
        if (gy >= Ho || gx >= Wo) continue;
        const int64_t at = (int64_t)gy * Wo + gx;
        if constexpr (PAIR) {
            const float s = 0.70710678118654752440f;
            if (dst1) dst1[at] = scat_mag((qa - qd) * s, (qb + qc) * s, a.bias);
            if (dst2) dst2[at] = scat_mag((qa + qd) * s, (qb - qc) * s, a.bias);
        } else {
            dst1[at] = ((qa + qb) + (qc + qd)) * 0.25f;
        }
    }
}

template <int L0, int L1>
__global__ void __launch_bounds__(kBlock) scat_layer_kernel(const ScatArgs a) {
    kernarg_touch_for(a);
    constexpr int LMAX = L0 > L1 ? L0 : L1;
    __shared__ float stage[(kScatInH + LMAX - 1) * (kScatInW + LMAX - 1)];
    __shared__ __attribute__((aligned(16))) float rowed[(kScatInH + LMAX - 1) * kScatInW];
    // blockIdx.x = ((plane * ngroups + gi) * tiles_y + ty) * tiles_x + tx
    int64_t r = blockIdx.x;
    const int tx = (int)(r % a.tiles_x);
    r /= a.tiles_x;
    const int ty = (int)(r % a.tiles_y);
    r /= a.tiles_y;
    const int g = a.groups[(int)(r % a.ngroups)];
    const int64_t plane = r / a.ngroups;
    const int64_t b = plane / a.C, c = plane - b * a.C;
    // band-major channels of this plane's group: band g and, for a pair, its sibling 7 - g
    const int64_t k1 = (int64_t)g * a.C + c, k2 = (int64_t)(7 - g) * a.C + c;
    const bool want1 = k1 >= a.k0 && k1 < a.k0 + a.nk, want2 = g != 0 && k2 >= a.k0 && k2 < a.k0 + a.nk;
    if (!want1 && !want2) return;  // the whole workgroup: nothing loaded, filtered or stored
    const int64_t out_plane = (int64_t)(a.He / 2) * (a.We / 2);
    float* dst1 = want1 ? a.out + (b * a.nk + (k1 - a.k0)) * out_plane : nullptr;
    float* dst2 = want2 ? a.out + (b * a.nk + (k2 - a.k0)) * out_plane : nullptr;
    const float* src = a.x + plane * (int64_t)a.H * a.W;
    const float *h0 = a.taps.h0, *h1 = a.taps.h1;
    switch (g) {  // uniform over the workgroup
        case 0: scat_tile<L0, L0, false, LMAX>(a, h0, h0, src, dst1, dst2, ty, tx, stage, rowed); break;  // ll: low rows, low columns
        case 1: scat_tile<L0, L1, true, LMAX>(a, h0, h1, src, dst1, dst2, ty, tx, stage, rowed); break;   // lh: 15 / 165 degrees
        case 2: scat_tile<L1, L1, true, LMAX>(a, h1, h1, src, dst1, dst2, ty, tx, stage, rowed); break;   // hh: 45 / 135
        default: scat_tile<L1, L0, true, LMAX>(a, h1, h0, src, dst1, dst2, ty, tx, stage, rowed); break;  // hl: 75 / 105
    }
}

}  // namespace sonar

using namespace sonar;

extern "C" int sonar_scat_layer_f32(const float* x, float* out, int64_t B, int64_t C, int64_t H, int64_t W, const float* h0, int n0,
                                    const float* h1, int n1, float magbias, int64_t k0, int64_t nk, void* stream) {
    const char* what = "sonar_scat_layer_f32";
    SONAR_REQUIRE(x && out && h0 && h1 && x != out && ((uintptr_t)x % 4) == 0 && ((uintptr_t)out % 4) == 0, SONAR_ERR_ARG,
                  "%s: x, out, h0 and h1 must be distinct non-NULL float pointers", what);
    SONAR_REQUIRE(B >= 0 && C >= 1 && H >= 1 && W >= 1, SONAR_ERR_ARG, "%s: bad shape [%lld, %lld, %lld, %lld]", what, (long long)B, (long long)C,
                  (long long)H, (long long)W);
    SONAR_REQUIRE(H <= SONAR_SCAT_MAX_SIDE && W <= SONAR_SCAT_MAX_SIDE && C <= (1 << 24), SONAR_ERR_UNSUPPORTED,
                  "%s: a plane side beyond %d or more than 2^24 channels", what, SONAR_SCAT_MAX_SIDE);
    SONAR_REQUIRE(magbias >= 0.0f && magbias <= 3.0e38f, SONAR_ERR_ARG, "%s: magbias %g must be finite and not negative", what, (double)magbias);
    SONAR_REQUIRE(k0 >= 0 && nk >= 1 && k0 <= 7 * C - nk, SONAR_ERR_ARG, "%s: channel window [%lld, %lld + %lld) outside the %lld output channels",
                  what, (long long)k0, (long long)k0, (long long)nk, (long long)(7 * C));
    const bool known = (n0 == 5 && n1 == 7) || (n0 == 5 && n1 == 3) || (n0 == 9 && n1 == 7);
    SONAR_REQUIRE(known, SONAR_ERR_UNSUPPORTED, "%s: filter lengths %d / %d; built: 5 / 7, 5 / 3, 9 / 7", what, n0, n1);
    ScatArgs a{};
    for (int k = 0; k < n0; ++k) a.taps.h0[k] = h0[k];
    for (int k = 0; k < n1; ++k) a.taps.h1[k] = h1[k];
    for (int k = 0; k < n0; ++k) SONAR_REQUIRE(fabsf(a.taps.h0[k]) <= 3.0e38f, SONAR_ERR_ARG, "%s: h0[%d] is not finite", what, k);
    for (int k = 0; k < n1; ++k) SONAR_REQUIRE(fabsf(a.taps.h1[k]) <= 3.0e38f, SONAR_ERR_ARG, "%s: h1[%d] is not finite", what, k);
    if (B == 0) return SONAR_OK;
    a.x = x;
    a.out = out;
    a.planes = B * C;
    a.C = (int)C;
    a.H = (int)H;
    a.W = (int)W;
    a.He = (int)(H + (H & 1));
    a.We = (int)(W + (W & 1));
    a.tiles_y = (a.He / 2 + kScatTileH - 1) / kScatTileH;
    a.tiles_x = (a.We / 2 + kScatTileW - 1) / kScatTileW;
    a.k0 = k0;
    a.nk = nk;
    a.bias = magbias;
    // bands the window touches -> their groups (band 0: ll; bands g and 7 - g: group g)
    const int band_lo = (int)(k0 / C), band_hi = (int)((k0 + nk - 1) / C);
    for (int g = 0; g < 4; ++g) {
        const bool hit = (g >= band_lo && g <= band_hi) || (g != 0 && 7 - g >= band_lo && 7 - g <= band_hi);
        if (hit) a.groups[a.ngroups++] = g;
    }
    const int64_t blocks = a.planes * a.ngroups * a.tiles_y * a.tiles_x;
    SONAR_REQUIRE(blocks < ((int64_t)1 << 31), SONAR_ERR_UNSUPPORTED, "%s: %lld workgroups in one launch", what, (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    if (n0 == 5 && n1 == 7) hipLaunchKernelGGL((scat_layer_kernel<5, 7>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    else if (n0 == 5 && n1 == 3) hipLaunchKernelGGL((scat_layer_kernel<5, 3>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((scat_layer_kernel<9, 7>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    return check_launch(what);
}
