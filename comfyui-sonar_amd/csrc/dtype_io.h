// The element layer of the kernels that take fp32, fp16 or bf16 tensors (SONAR_DTYPE_*) and compute in fp32: the two 16-bit storage
// types, widen / narrow, the V-wide pack with its typed load / store, and with_dtype, which turns a run-time dtype code into the element
// type.  The rules, stated here once: narrowing rounds to nearest even; a NaN narrowed to bf16 is 0x7FC0, the quiet NaN torch writes (fp16
// is v_cvt_f16_f32's); V == 4 is ONE access, 16 bytes of fp32 or 8 bytes of a 16-bit type, and V == 1 one element.
#pragma once
#include <stdint.h>

#include "common.h"

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

// V-wide pack of floats (V = 4 -> one access per lane; V = 1 for unaligned buffers and tails).
template <int V>
struct Pack {
    float v[V];
};
// V consecutive elements from index i, widened
template <int V, typename T>
__device__ __forceinline__ Pack<V> load(const T* p, int64_t i) {
    Pack<V> r;
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
// ... narrowed with one rounding and written (NT: the 16-byte stores of fp32 with the non-temporal hint)
template <int V, bool NT = false, typename T>
__device__ __forceinline__ void store(T* p, int64_t i, const Pack<V>& r) {
    if constexpr (V == 1) {
        p[i] = narrow<T>(r.v[0]);
    } else if constexpr (sizeof(T) == 4) {
        store4<NT>(p + i, r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
        uint2 t;
        t.x = (uint32_t)narrow<T>(r.v[0]).bits | ((uint32_t)narrow<T>(r.v[1]).bits << 16);
        t.y = (uint32_t)narrow<T>(r.v[2]).bits | ((uint32_t)narrow<T>(r.v[3]).bits << 16);
        *reinterpret_cast<uint2*>(p + i) = t;
    }
}

// ---- host side: the dtype code of an entry point --------------------------------------------------------------------------------------
static inline int elem_bytes(int dtype) { return dtype == SONAR_DTYPE_F32 ? 4 : 2; }

// the range check of every entry point that takes a dtype code, and its message
#define SONAR_REQUIRE_DTYPE(code, who) \
    SONAR_REQUIRE((code) >= SONAR_DTYPE_F32 && (code) <= SONAR_DTYPE_BF16, SONAR_ERR_ARG, "%s: unknown dtype %d", (who), (int)(code))

template <typename T>
struct ElemTag {
    using type = T;
};
// f(ElemTag<element type>) for a valid code, its result returned; SONAR_ERR_ARG in `who`'s name for any other
template <typename F>
static inline int with_dtype(int code, const char* who, F&& f) {
    SONAR_REQUIRE_DTYPE(code, who);
    if (code == SONAR_DTYPE_F32) return f(ElemTag<float>{});
    if (code == SONAR_DTYPE_F16) return f(ElemTag<F16>{});
    return f(ElemTag<BF16>{});
}

}  // namespace sonar
