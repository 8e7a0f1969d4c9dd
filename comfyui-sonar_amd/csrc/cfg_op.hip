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

// sigma of elements i .. i + V - 1: one value for the tensor, or one per sample of `inner` elements -- a vector may straddle a sample
// boundary (inner need not be a multiple of V, and may be smaller than V), so the row is tracked per lane.  Reads sigma[row] only for rows
// of elements the caller owns (i + V <= n).
template <int V>
__device__ __forceinline__ Pack<V> load_sigma(const float* __restrict__ sigma, int per_sample, int64_t inner, int64_t i) {
    Pack<V> s;
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
        Pack<V> a = load<V>(t1, i), b{};
        if (t2) b = load<V>(t2, i);
        if (sigma) {
            const Pack<V> px = load<V>(x, i), s = load_sigma<V>(sigma, per_sample, inner, i);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                a.v[k] = (px.v[k] - a.v[k]) / s.v[k];
                if (t2) b.v[k] = (px.v[k] - b.v[k]) / s.v[k];
            }
        }
        if (t2) {
            store<V>(t2_out, i, b);
#pragma unroll
            for (int k = 0; k < V; ++k) a.v[k] = a.v[k] - b.v[k];
        }
        store<V>(result, i, a);
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
        Pack<V> r = load<V>(result, i);
        if (t2) {
            const Pack<V> b = load<V>(t2, i);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = r.v[k] + b.v[k];
        }
        if (sigma) {
            const Pack<V> px = load<V>(x, i), s = load_sigma<V>(sigma, per_sample, inner, i);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = px.v[k] - s.v[k] * r.v[k];
        }
        if (blend_mode >= 0) {
            const Pack<V> o = load<V>(t1_orig, i);
#pragma unroll
            for (int k = 0; k < V; ++k) r.v[k] = blend<float>(blend_mode, o.v[k], r.v[k], w);
        }
        store<V>(out, i, r);
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
    SONAR_REQUIRE_DTYPE(dtype, "sonar_cfg_op_prepare");
    SONAR_REQUIRE(cfg_shape_ok(n, inner, sigma, sigma_n), SONAR_ERR_ARG, "sonar_cfg_op_prepare: bad n / inner / sigma_n");
    if (n == 0) return SONAR_OK;  // nothing to read or write: an empty tensor's buffers may be null
    SONAR_REQUIRE(t1 && result && (sigma == nullptr || x) && (t2 == nullptr || t2_out), SONAR_ERR_ARG, "sonar_cfg_op_prepare: null pointer");
    const int per_sample = sigma != nullptr && sigma_n > 1;
    const hipStream_t st = (hipStream_t)stream;
    if (t2 == nullptr) t2_out = nullptr;
    if (sigma == nullptr) x = nullptr;
    return with_dtype(dtype, "sonar_cfg_op_prepare", [&](auto elem) {
        return prepare_typed<typename decltype(elem)::type>(x, t1, t2, sigma, per_sample, result, t2_out, n, inner, st);
    });
}

extern "C" int sonar_cfg_op_finish(int dtype, const float* result, const float* t2, const void* x, const float* sigma, int64_t sigma_n,
                                   const void* t1_orig, int blend_mode, float w, void* out, int64_t n, int64_t inner, void* stream) {
    SONAR_REQUIRE_DTYPE(dtype, "sonar_cfg_op_finish");
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
    return with_dtype(dtype, "sonar_cfg_op_finish", [&](auto elem) {
        return finish_typed<typename decltype(elem)::type>(result, t2, x, sigma, per_sample, t1_orig, blend_mode, w, out, n, inner, st);
    });
}
