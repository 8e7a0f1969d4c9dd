// SDXL bucket kernels, first half, and the dispatcher (see power_buckets.h).
#include "power_buckets.h"

namespace sonar {

int launch_power_bucket(SONAR_BUCKET_ARGS) {
#define SONAR_BUCKET_CASE(HH, WW, A, B, C, D) \
    if (H == HH && W == WW) return launch_power_any_t<A, B, C, D>(SONAR_BUCKET_PASS);
    SONAR_BUCKETS_A(SONAR_BUCKET_CASE)
#undef SONAR_BUCKET_CASE
    return launch_power_bucket_b(SONAR_BUCKET_PASS);
}

// a bucket out of step with its size (the products) is no bucket: the size takes the run-time-size kernels
bool power_bucket_pairs(int64_t H, int64_t W, int* pairs) {
#define SONAR_BUCKET_CASE(HH, WW, A, B, C, D)                     \
    if (H == HH && W == WW && A * B == HH && 2 * C * D == WW) {   \
        pairs[0] = A, pairs[1] = B, pairs[2] = C, pairs[3] = D;   \
        return true;                                              \
    }
    SONAR_BUCKETS_A(SONAR_BUCKET_CASE)
    SONAR_BUCKETS_B(SONAR_BUCKET_CASE)
#undef SONAR_BUCKET_CASE
    return false;
}

}  // namespace sonar

#ifdef SONAR_ANY_TRACE
extern "C" int sonar_debug_any_trace_a(unsigned long long* host_out) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(sonar::g_any_trace), sizeof(sonar::g_any_trace));
}
#endif
