// The streaming driver of the elementwise units (elementwise.hip, sampler_steps.hip, cfg_op.hip): an Op struct says what happens to V
// consecutive elements (read and written through dtype_io.h's Pack / load / store), ew_kernel walks the tensor with it and launch_ew picks
// the 4-element or the scalar route.  Also the one definition of aligned16, which the generator units take from here through noise_stream.h.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "dtype_io.h"  // Pack, load, store

namespace sonar {

// Generic driver: op.template run<V>(elem_index) handles V consecutive elements.
template <int V, typename Op>
__global__ void __launch_bounds__(kBlock) ew_kernel(Op op, int64_t n) {
    kernarg_touch_for(op, n);
    const int64_t nv = n / V;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nv; i += stride) op.template run<V>(i * V);
    if constexpr (V > 1) {
        if (blockIdx.x == 0)
            for (int64_t i = nv * V + threadIdx.x; i < n; i += kBlock) op.template run<1>(i);
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Pure streaming kernels: one 16-byte item per thread (measured on MI355X, 3 reads + 2 writes of 134 MB each:
// 32768 blocks x 1 item 5.8 TB/s, 2048 persistent blocks x 16 items 5.3 TB/s -- scratch/stream5.cpp)
static inline int grid_stream(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + kBlock - 1) / kBlock, 1 << 20)); }

template <typename Op>
static int launch_ew(Op op, int64_t n, bool vec_ok, hipStream_t st, const char* what) {
    if (n == 0) return SONAR_OK;
    if (vec_ok) {
        hipLaunchKernelGGL((ew_kernel<4, Op>), dim3(grid_stream(n / 4 + 1)), dim3(kBlock), 0, st, op, n);
    } else {
        hipLaunchKernelGGL((ew_kernel<1, Op>), dim3(grid_stream(n)), dim3(kBlock), 0, st, op, n);
    }
    return check_launch(what);
}

}  // namespace sonar
