// CollatzNoiseGenerator (py/noise_generation.py:2330-2615): one iteration of the generator as two kernels over the view
// [outer][len][inner] of the latent (not flattened: len = shape[dim], inner = the sizes behind it; flattened: len = the sizes from dim on,
// inner = 1).  cl = min(len, chain_length) values are kept per chain, cl + chain_offset computed, n_chunks = ceil(len / cl) chains lie along
// `len`, and the kept values fill the padded layout [outer][len_p = n_chunks * cl][inner].
//   collatz_chain_kernel  one thread per chain, chain c = (o * n_chunks + k) * inner + i.  The start value, the zero replacement, the
//                         seed_mode parity fix and the recurrence of lines 2434-2501 with result, muls and adds in registers; what the
//                         reference keeps (result / noise, muls or adds / noise) of the links past chain_offset goes straight to the padded
//                         layout.  With inner > 1 neighbouring threads are neighbouring i, so every link is stored as whole lines.  With
//                         inner == 1 a thread owns cl consecutive outputs and a workgroup a contiguous run of 256 cl: the links pass
//                         through an LDS tile 16 links wide and leave it in memory order.
//   collatz_mix_kernel    acc += (out1 * second) * scale over the unpadded [outer][len][inner], the padding cropped by indexing; second is
//                         1, the chain's seed (repeat_interleave by indexing) or the mix noise.
// Every step is one correctly rounded fp32 operation in the reference's order (the library is built with -ffp-contract=off), so the chain
// stage is the reference's bit for bit.
#include "common.h"

namespace sonar {

namespace {

constexpr int kTileLinks = 16;                  // links per thread staged in LDS before a flush (inner == 1)
constexpr int kTileStride = kTileLinks + 1;     // odd: a thread's row starts in its own bank

struct ChainParams {
    float span, rmin;              // noise = seed * span + rmin
    float emul, eadd, omul, oadd;  // fp32 images of the four scalars
    int mul_any, emul_one, omul_one, add_any, eadd_zero, oadd_zero;  // the reference's shortcuts, decided on the scalars as given
    int integer_math, break_loops, keep_sign, seed_mode, output;
};

// torch.remainder(x, 2): fmod, then the divisor's sign
__device__ __forceinline__ float rem2(float x) {
    float r = fmodf(x, 2.0f);
    if (r != 0.0f && r < 0.0f) r = __fadd_rn(r, 2.0f);
    return r;
}

// utils.trunc_decimals(x, 2)
__device__ __forceinline__ float trunc2(float x) {
    const float xi = truncf(x);
    const float xf = __fsub_rn(x, xi);
    return __fadd_rn(xi, __fmul_rn(truncf(__fmul_rn(xf, 100.0f)), 0.01f));
}

__device__ __forceinline__ float sign_of(float x) { return (float)((0.0f < x) - (x < 0.0f)); }

struct Chain {
    float noise, result, muls, adds;

    __device__ __forceinline__ void start(float seed, float seed_ext, float numel, const ChainParams& p) {
        float v = __fadd_rn(__fmul_rn(seed, p.span), p.rmin);
        if (v == 0.0f) v = __fdiv_rn(__fadd_rn(__fmul_rn(seed_ext, p.span), p.rmin), numel);  // noise.max() / noise.numel()
        if (p.seed_mode != SONAR_COLLATZ_SEED_DEFAULT) {
            const bool even = rem2(v) < 1.0f;
            if (even == (p.seed_mode == SONAR_COLLATZ_SEED_FORCE_ODD)) v = __fadd_rn(v, 1.0f);
        }
        noise = result = v;
        muls = 1.0f;
        adds = 0.0f;
    }

    __device__ __forceinline__ void step(const ChainParams& p) {
        const float prev = result;
        bool reset = false;
        if (p.break_loops) {
            const float pt = trunc2(prev);
            reset = (pt >= 1.0f && pt < 1.001f) || fabsf(pt) < 0.001f;
        }
        const bool even = rem2(prev) < 1.0f;
        float m = muls;
        if (p.mul_any) m = even ? (p.emul_one ? m : __fmul_rn(m, p.emul)) : (p.omul_one ? m : __fmul_rn(m, p.omul));
        if (reset) m = 1.0f;
        float a = __fmul_rn(adds, m);
        if (p.add_any) {
            const float sgn = p.keep_sign ? sign_of(prev) : 1.0f;
            a = even ? (p.eadd_zero ? a : __fadd_rn(a, __fmul_rn(p.eadd, sgn))) : (p.oadd_zero ? a : __fadd_rn(a, __fmul_rn(p.oadd, sgn)));
        }
        if (reset) a = 0.0f;
        float r = __fadd_rn(__fmul_rn(noise, m), a);
        if (p.integer_math) r = truncf(r);
        muls = m;
        adds = a;
        result = reset ? noise : r;
    }

    __device__ __forceinline__ float kept(const ChainParams& p) const {
        return p.output == SONAR_COLLATZ_OUT_MULTS ? muls : __fdiv_rn(p.output == SONAR_COLLATZ_OUT_ADDS ? adds : result, noise);
    }
};

// LAST: inner == 1 and cl > 1, the outputs of a workgroup's chains are one contiguous run
template <bool LAST>
__global__ void __launch_bounds__(kBlock) collatz_chain_kernel(const float* __restrict__ seeds, const float* __restrict__ seed_ext,
                                                               float* __restrict__ out, int64_t chains, int64_t n_chunks, int64_t inner,
                                                               int64_t cl, int64_t offset, ChainParams p) {
    __shared__ float tile[LAST ? kBlock * kTileStride : 1];
    const float ext = *seed_ext;
    const float numel = (float)chains;
    const int64_t links = cl + offset;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < chains; base += (int64_t)gridDim.x * kBlock) {
        const int64_t c = base + threadIdx.x;
        const bool live = c < chains;
        Chain ch;
        int64_t at = 0;  // the chain's first output: (o * len_p + k * cl) * inner + i
        if (live) {
            ch.start(seeds[c], ext, numel, p);
            const int64_t ok = c / inner, i = c - ok * inner;
            at = ok * cl * inner + i;  // o * len_p + k * cl = (o * n_chunks + k) * cl
        }
        for (int64_t t = 0; t < links; ++t) {  // (uniform: every thread of the workgroup reaches the barriers below)
            if (live && t > 0) ch.step(p);
            if (t < offset) continue;
            const int64_t j = t - offset;
            if constexpr (LAST) {
                const int col = (int)(j % kTileLinks);
                if (live) tile[threadIdx.x * kTileStride + col] = ch.kept(p);
                if (col == kTileLinks - 1 || j == cl - 1) {
                    __syncthreads();
                    const int w = col + 1;
                    const int64_t j0 = j - col;
                    const int64_t left = chains - base;
                    const int nrows = left < kBlock ? (int)left : kBlock;
                    for (int e = threadIdx.x; e < nrows * w; e += kBlock) {
                        const int row = e / w, cc = e - row * w;
                        out[(base + row) * cl + j0 + cc] = tile[row * kTileStride + cc];
                    }
                    __syncthreads();
                }
            } else {
                if (live) out[at + j * inner] = ch.kept(p);
            }
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) collatz_mix_kernel(float* __restrict__ acc, const float* __restrict__ out1,
                                                             const float* __restrict__ second, int64_t total, int64_t len, int64_t inner,
                                                             int64_t cl, int64_t n_chunks, float scale) {
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < total; f += (int64_t)gridDim.x * kBlock) {
        const int64_t oj = inner == 1 ? f : f / inner, i = inner == 1 ? 0 : f - oj * inner;
        const int64_t o = oj / len, j = oj - o * len;
        float v = out1[(o * n_chunks * cl + j) * inner + i];
        if constexpr (MODE == SONAR_COLLATZ_SECOND_SEEDS) v = __fmul_rn(second[(o * n_chunks + j / cl) * inner + i], v);
        if constexpr (MODE == SONAR_COLLATZ_SECOND_MIX) v = __fmul_rn(second[f], v);
        acc[f] = __fadd_rn(acc[f], __fmul_rn(v, scale));
    }
}

struct View {
    int64_t outer, len, inner, cl, n_chunks, chains;
    bool empty;
};

// the checks both entry points share; fills `v`
int view(const char* who, int64_t outer, int64_t len, int64_t inner, int64_t chain_length, View& v) {
    constexpr int64_t kMax = (int64_t)1 << 31;
    SONAR_REQUIRE(outer >= 0 && len >= 0 && inner >= 0, SONAR_ERR_ARG, "%s: negative size (%lld, %lld, %lld)", who, (long long)outer,
                  (long long)len, (long long)inner);
    SONAR_REQUIRE(outer <= kMax && len <= kMax && inner <= kMax, SONAR_ERR_ARG, "%s: a size beyond 2^31", who);
    SONAR_REQUIRE(chain_length >= 1 && chain_length <= kMax, SONAR_ERR_ARG, "%s: chain_length %lld", who, (long long)chain_length);
    v.outer = outer, v.len = len, v.inner = inner;
    v.empty = outer == 0 || len == 0 || inner == 0;
    if (v.empty) return SONAR_OK;
    v.cl = len < chain_length ? len : chain_length;
    v.n_chunks = (len + v.cl - 1) / v.cl;
    SONAR_REQUIRE(outer * inner <= kMax && outer * inner * v.n_chunks <= kMax, SONAR_ERR_ARG, "%s: more than 2^31 chains", who);
    v.chains = outer * inner * v.n_chunks;
    SONAR_REQUIRE(v.chains * v.cl <= ((int64_t)1 << 40), SONAR_ERR_ARG, "%s: more than 2^40 values", who);
    return SONAR_OK;
}

}  // namespace

}  // namespace sonar

extern "C" int sonar_collatz_chain_f32(const float* seeds, const float* seed_ext, float* out, int64_t outer, int64_t len, int64_t inner,
                                       int64_t chain_length, int64_t chain_offset, double span, double rmin, double emul, double eadd,
                                       double omul, double oadd, int flags, int seed_mode, int output, void* stream) {
    using namespace sonar;
    const char* who = "sonar_collatz_chain_f32";
    SONAR_REQUIRE(seeds != nullptr && seed_ext != nullptr && out != nullptr, SONAR_ERR_ARG, "%s: NULL tensor", who);
    SONAR_REQUIRE(out != seeds && out != seed_ext, SONAR_ERR_ARG, "%s: out must not be seeds", who);
    View v;
    if (const int rc = view(who, outer, len, inner, chain_length, v)) return rc;
    SONAR_REQUIRE(chain_offset >= 0 && chain_offset <= ((int64_t)1 << 31), SONAR_ERR_ARG, "%s: chain_offset %lld", who, (long long)chain_offset);
    SONAR_REQUIRE(seed_mode >= SONAR_COLLATZ_SEED_DEFAULT && seed_mode <= SONAR_COLLATZ_SEED_FORCE_EVEN, SONAR_ERR_ARG, "%s: seed_mode %d", who,
                  seed_mode);
    SONAR_REQUIRE(output >= SONAR_COLLATZ_OUT_RATIOS && output <= SONAR_COLLATZ_OUT_ADDS, SONAR_ERR_ARG, "%s: output %d", who, output);
    SONAR_REQUIRE((flags & ~(SONAR_COLLATZ_INTEGER_MATH | SONAR_COLLATZ_BREAK_LOOPS | SONAR_COLLATZ_KEEP_SIGN)) == 0, SONAR_ERR_ARG,
                  "%s: flags 0x%x", who, flags);
    if (v.empty) return SONAR_OK;
    ChainParams p;
    p.span = (float)span, p.rmin = (float)rmin;
    p.emul = (float)emul, p.eadd = (float)eadd, p.omul = (float)omul, p.oadd = (float)oadd;
    p.emul_one = emul == 1.0, p.omul_one = omul == 1.0, p.mul_any = !(p.emul_one && p.omul_one);
    p.eadd_zero = eadd == 0.0, p.oadd_zero = oadd == 0.0, p.add_any = !(p.eadd_zero && p.oadd_zero);
    p.integer_math = (flags & SONAR_COLLATZ_INTEGER_MATH) != 0;
    p.break_loops = (flags & SONAR_COLLATZ_BREAK_LOOPS) != 0;
    p.keep_sign = (flags & SONAR_COLLATZ_KEEP_SIGN) != 0;
    p.seed_mode = seed_mode, p.output = output;
    const dim3 grid(grid_for(v.chains, kBlock)), block(kBlock);
    const hipStream_t st = (hipStream_t)stream;
    if (v.inner == 1 && v.cl > 1)
        hipLaunchKernelGGL(collatz_chain_kernel<true>, grid, block, 0, st, seeds, seed_ext, out, v.chains, v.n_chunks, v.inner, v.cl, chain_offset, p);
    else
        hipLaunchKernelGGL(collatz_chain_kernel<false>, grid, block, 0, st, seeds, seed_ext, out, v.chains, v.n_chunks, v.inner, v.cl, chain_offset, p);
    return check_launch(who);
}

extern "C" int sonar_collatz_mix_f32(float* acc, const float* out1, const float* second, int second_mode, int64_t outer, int64_t len,
                                     int64_t inner, int64_t chain_length, float scale, void* stream) {
    using namespace sonar;
    const char* who = "sonar_collatz_mix_f32";
    SONAR_REQUIRE(acc != nullptr && out1 != nullptr, SONAR_ERR_ARG, "%s: NULL tensor", who);
    SONAR_REQUIRE(second_mode >= SONAR_COLLATZ_SECOND_ONE && second_mode <= SONAR_COLLATZ_SECOND_MIX, SONAR_ERR_ARG, "%s: second_mode %d", who,
                  second_mode);
    SONAR_REQUIRE(second_mode == SONAR_COLLATZ_SECOND_ONE || second != nullptr, SONAR_ERR_ARG, "%s: NULL second factor", who);
    SONAR_REQUIRE(acc != out1 && acc != second, SONAR_ERR_ARG, "%s: acc must not be an input", who);
    View v;
    if (const int rc = view(who, outer, len, inner, chain_length, v)) return rc;
    if (v.empty) return SONAR_OK;
    const int64_t total = v.outer * v.len * v.inner;
    const dim3 grid(grid_for(total, kBlock)), block(kBlock);
    const hipStream_t st = (hipStream_t)stream;
    if (second_mode == SONAR_COLLATZ_SECOND_SEEDS)
        hipLaunchKernelGGL(collatz_mix_kernel<SONAR_COLLATZ_SECOND_SEEDS>, grid, block, 0, st, acc, out1, second, total, v.len, v.inner, v.cl, v.n_chunks, scale);
    else if (second_mode == SONAR_COLLATZ_SECOND_MIX)
        hipLaunchKernelGGL(collatz_mix_kernel<SONAR_COLLATZ_SECOND_MIX>, grid, block, 0, st, acc, out1, second, total, v.len, v.inner, v.cl, v.n_chunks, scale);
    else
        hipLaunchKernelGGL(collatz_mix_kernel<SONAR_COLLATZ_SECOND_ONE>, grid, block, 0, st, acc, out1, second, total, v.len, v.inner, v.cl, v.n_chunks, scale);
    return check_launch(who);
}
