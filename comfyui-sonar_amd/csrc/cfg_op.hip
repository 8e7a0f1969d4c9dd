// SonarApplyLatentOperationCFG (py/nodes/latent_operations.py:246-300): the arithmetic around the latent operations, two launches.
//   prepare: f(t) = (x - t) / sigma[sample] (prediction flip) or t;  t2_out = f(t2);  result = f(t1) - f(t2)   (or f(t1) without t2)
//   finish:  r = result + t2;  flip: r = x - sigma[sample] * r;  out = blend(t1_orig, r, w)  (or r), written once in t1_orig's dtype
// Between the two everything is fp32; x / t1 / t2 / t1_orig arrive in fp32, fp16 or bf16 and are widened at load.  Both are HBM-bound (with
// flip and t2: 3 reads + 2 writes, and 4 reads + 1 write): the shape of ew_driver.h's ew_kernel -- one 4-element item per thread (16 bytes
// of fp32, 8 of a half type), grid-stride, scalar tail, and the scalar route for buffers that are not 16-byte aligned.  Every operation is rounded
// on its own (-ffp-contract=off) in the reference's order, the division is a true division: on fp32 inputs the bits are the reference's.
#include <math.h>

#include "ew_driver.h"

namespace sonar {

// 16-bit storage types (bit patterns; arithmetic is fp32)
struct F16 {
    uint16_t bits;
};
struct BF16 {
    uint16_t bits;
};

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(F16 v) { return (float)__builtin_bit_cast(_Float16, v.bits); }
__device__ __forceinline__ float widen(BF16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

template <typename T>
__device__ __forceinline__ T narrow(float v);
template <>
__device__ __forceinline__ float narrow<float>(float v) { return v; }
template <>
__device__ __forceinline__ F16 narrow<F16>(float v) { return F16{__builtin_bit_cast(uint16_t, (_Float16)v)}; }  // v_cvt_f16_f32: nearest even
template <>
__device__ __forceinline__ BF16 narrow<BF16>(float v) {  // nearest even; NaN -> the quiet NaN torch writes
    const uint32_t u = __float_as_uint(v);
    if (v != v) return BF16{0x7FC0};
    return BF16{(uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16)};
}

template <int V>
struct Vals {
    float v[V];
};

// V consecutive elements from index i (V == 4: one 16-byte access for float, one 8-byte access for the half types)
template <int V, typename T>
__device__ __forceinline__ Vals<V> load_vals(const T* __restrict__ p, int64_t i) {
    Vals<V> r;
    if constexpr (V == 1) {
        r.v[0] = widen(p[i]);
    } else if constexpr (sizeof(T) == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p + i);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        const uint2 t = *reinterpret_cast<const uint2*>(p + i);
        r.v[0] = widen(T{(uint16_t)(t.x & 0xFFFFu)}); r.v[1] = widen(T{(uint16_t)(t.x >> 16)});
        r.v[2] = widen(T{(uint16_t)(t.y & 0xFFFFu)}); r.v[3] = widen(T{(uint16_t)(t.y >> 16)});
    }
    return r;
}

template <int V, typename T>
__device__ __forceinline__ void store_vals(T* __restrict__ p, int64_t i, const Vals<V>& r) {
    if constexpr (V == 1) {
        p[i] = narrow<T>(r.v[0]);
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p + i) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
        uint2 t;
        t.x = (uint32_t)narrow<T>(r.v[0]).bits | ((uint32_t)narrow<T>(r.v[1]).bits << 16);
        t.y = (uint32_t)narrow<T>(r.v[2]).bits | ((uint32_t)narrow<T>(r.v[3]).bits << 16);
        *reinterpret_cast<uint2*>(p + i) = t;
    }
}

// sigma of elements i .. i + V - 1: one value for the tensor, or one per sample of `inner` elements -- a vector may straddle a sample
// boundary (inner need not be a multiple of V, and may be smaller than V), so the row is tracked per lane.  Reads sigma[row] only for rows
// of elements the caller owns (i + V <= n).
template <int V>
__device__ __forceinline__ Vals<V> load_sigma(const float* __restrict__ sigma, int per_sample, int64_t inner, int64_t i) {
    Vals<V> s;
    if (!per_sample) {
        const float one = sigma[0];
#pragma unroll
        for (int k = 0; k < V; ++k) s.v[k] = one;
        return s;
    }
    int64_t row = i / inner;
    int64_t rem = i - row * inner;
    float cur = sigma[row];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        s.v[k] = cur;
        if (k + 1 < V && ++rem == inner) {  // element i + k + 1 opens the next sample (it exists: it belongs to this vector)
            rem = 0;
            cur = sigma[++row];
        }
    }
    return s;
}

template <typename T>
struct CfgPrepareOp {
    const T *x, *t1, *t2;   // x: null without flip; t2: nullable
    const float* sigma;     // null: no flip
    float *result, *t2_out; // t2_out: written when t2 is given
    int64_t inner;
    int per_sample;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Vals<V> a = load_vals<V>(t1, i), b{};
        if (t2) b = load_vals<V>(t2, i);
        if (sigma) {
            const Vals<V> px = load_vals<V>(x, i), s = load_sigma<V>(sigma, per_sample, inner, i);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                a.v[k] = (px.v[k] - a.v[k]) / s.v[k];
                if (t2) b.v[k] = (px.v[k] - b.v[k]) / s.v[k];
            }
        }
        if (t2) {
            store_vals<V>(t2_out, i, b);
#pragma unroll
            for (int k = 0; k < V; ++k) a.v[k] = a.v[k] - b.v[k];
        }
        store_vals<V>(result, i, a);
    }
};

template <typename T>
struct CfgFinishOp {
    const float *result, *t2;  // t2: nullable (the buffer prepare wrote)
    const T* x;                // null without flip
    const float* sigma;        // null: no flip
    const T* t1_orig;          // null when blend_mode < 0
    T* out;
    int64_t inner;
    int per_sample, blend_mode;  // blend_mode < 0: out = r
    float w;
    template <int V>
    __device__ __forceinline__ void run(int64_t i) const {
        Vals<V> r = load_vals<V>(result, i);
        if (t2) {
            const Vals<V> b = load_vals<V>(t2, i);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = r.v[k] + b.v[k];
        }
        if (sigma) {
            const Vals<V> px = load_vals<V>(x, i), s = load_sigma<V>(sigma, per_sample, inner, i);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = px.v[k] - s.v[k] * r.v[k];
        }
        if (blend_mode >= 0) {
            const Vals<V> o = load_vals<V>(t1_orig, i);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = blend<float>(blend_mode, o.v[k], r.v[k], w);
        }
        store_vals<V>(out, i, r);
    }
};

// Both ops run on ew_driver.h's driver (ew_kernel through launch_ew); a null pointer counts as aligned.
template <typename T>
static int prepare_typed(const void* x, const void* t1, const void* t2, const float* sigma, int per_sample, float* result, float* t2_out,
                         int64_t n, int64_t inner, hipStream_t st) {
    CfgPrepareOp<T> op{(const T*)x, (const T*)t1, (const T*)t2, sigma, result, t2_out, inner, per_sample};
    const bool vec_ok = aligned16(x) && aligned16(t1) && aligned16(t2) && aligned16(result) && aligned16(t2_out);
    return launch_ew(op, n, vec_ok, st, "sonar_cfg_op_prepare");
}

template <typename T>
static int finish_typed(const float* result, const float* t2, const void* x, const float* sigma, int per_sample, const void* t1_orig,
                        int blend_mode, float w, void* out, int64_t n, int64_t inner, hipStream_t st) {
    CfgFinishOp<T> op{result, t2, (const T*)x, sigma, (const T*)t1_orig, (T*)out, inner, per_sample, blend_mode, w};
    const bool vec_ok = aligned16(result) && aligned16(t2) && aligned16(x) && aligned16(t1_orig) && aligned16(out);
    return launch_ew(op, n, vec_ok, st, "sonar_cfg_op_finish");
}

// n, inner and sigma_n against each other (sigma_n is looked at only with a sigma)
static inline bool cfg_shape_ok(int64_t n, int64_t inner, const float* sigma, int64_t sigma_n) {
    if (n < 0 || inner <= 0 || n % inner != 0) return false;
    return sigma == nullptr || sigma_n == 1 || sigma_n == n / inner;
}

}  // namespace sonar

using namespace sonar;

extern "C" int sonar_cfg_op_prepare(int dtype, const void* x, const void* t1, const void* t2, const float* sigma, int64_t sigma_n, float* result,
                                    float* t2_out, int64_t n, int64_t inner, void* stream) {
    SONAR_REQUIRE(dtype >= SONAR_DTYPE_F32 && dtype <= SONAR_DTYPE_BF16, SONAR_ERR_ARG, "sonar_cfg_op_prepare: unknown dtype %d", dtype);
    SONAR_REQUIRE(cfg_shape_ok(n, inner, sigma, sigma_n), SONAR_ERR_ARG, "sonar_cfg_op_prepare: bad n / inner / sigma_n");
    if (n == 0) return SONAR_OK;  // nothing to read or write: an empty tensor's buffers may be null
    SONAR_REQUIRE(t1 && result && (sigma == nullptr || x) && (t2 == nullptr || t2_out), SONAR_ERR_ARG, "sonar_cfg_op_prepare: null pointer");
    const int per_sample = sigma != nullptr && sigma_n > 1;
    const hipStream_t st = (hipStream_t)stream;
    if (t2 == nullptr) t2_out = nullptr;
    if (sigma == nullptr) x = nullptr;
    if (dtype == SONAR_DTYPE_F32) return prepare_typed<float>(x, t1, t2, sigma, per_sample, result, t2_out, n, inner, st);
    if (dtype == SONAR_DTYPE_F16) return prepare_typed<F16>(x, t1, t2, sigma, per_sample, result, t2_out, n, inner, st);
    return prepare_typed<BF16>(x, t1, t2, sigma, per_sample, result, t2_out, n, inner, st);
}

extern "C" int sonar_cfg_op_finish(int dtype, const float* result, const float* t2, const void* x, const float* sigma, int64_t sigma_n,
                                   const void* t1_orig, int blend_mode, float w, void* out, int64_t n, int64_t inner, void* stream) {
    SONAR_REQUIRE(dtype >= SONAR_DTYPE_F32 && dtype <= SONAR_DTYPE_BF16, SONAR_ERR_ARG, "sonar_cfg_op_finish: unknown dtype %d", dtype);
    SONAR_REQUIRE(blend_mode >= SONAR_CFG_BLEND_NONE && blend_mode <= SONAR_BLEND_SUBTRACT_B, SONAR_ERR_ARG,
                  "sonar_cfg_op_finish: unknown blend mode %d", blend_mode);
    SONAR_REQUIRE(cfg_shape_ok(n, inner, sigma, sigma_n), SONAR_ERR_ARG, "sonar_cfg_op_finish: bad n / inner / sigma_n");
    if (n == 0) return SONAR_OK;  // nothing to read or write: an empty tensor's buffers may be null
    SONAR_REQUIRE(result && out && (sigma == nullptr || x) && (blend_mode == SONAR_CFG_BLEND_NONE || t1_orig), SONAR_ERR_ARG,
                  "sonar_cfg_op_finish: null pointer");
    const int per_sample = sigma != nullptr && sigma_n > 1;
    const hipStream_t st = (hipStream_t)stream;
    if (sigma == nullptr) x = nullptr;
    if (blend_mode == SONAR_CFG_BLEND_NONE) t1_orig = nullptr;
    if (dtype == SONAR_DTYPE_F32) return finish_typed<float>(result, t2, x, sigma, per_sample, t1_orig, blend_mode, w, out, n, inner, st);
    if (dtype == SONAR_DTYPE_F16) return finish_typed<F16>(result, t2, x, sigma, per_sample, t1_orig, blend_mode, w, out, n, inner, st);
    return finish_typed<BF16>(result, t2, x, sigma, per_sample, t1_orig, blend_mode, w, out, n, inner, st);
}
