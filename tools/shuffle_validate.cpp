// Host-side check of the argument validation of csrc/shuffle.hip: both entry points are called with bad arguments only, so every call must
// come back with its error code before anything touches the HIP runtime -- no launch, no GPU needed.  Built with the host sanitizers
// ("Shuffled noise"):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/shuffle_validate.cpp comfyui-sonar_amd/csrc/shuffle.hip comfyui-sonar_amd/csrc/runtime.hip -o shuffle_validate
//   ASAN_OPTIONS=detect_leaks=0 ./shuffle_validate
#include <cstdint>
#include <cstdio>

#include "../include/sonar_hip.h"

static int bad = 0, calls = 0;

static void expect(const char* what, int rc, int want) {
    ++calls;
    if (rc != want) {
        std::printf("%s: returned %d, expected %d (%s)\n", what, rc, want, sonar_last_error());
        ++bad;
    }
}

int main() {
    // never dereferenced: the checks refuse every call below
    float* const a = reinterpret_cast<float*>(0x1000);
    float* const b = reinterpret_cast<float*>(0x2000);
    const int32_t* const idx = reinterpret_cast<const int32_t*>(0x3000);
    const int64_t big = SONAR_SHUFFLE_MAX_N + 1;

    expect("gather: NULL src", sonar_shuffle_gather_f32(nullptr, b, 4, 2, 3, 5, 7, 1, 3, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: NULL out", sonar_shuffle_gather_f32(a, nullptr, 4, 2, 3, 5, 7, 1, 3, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: NULL idx", sonar_shuffle_gather_f32(a, b, 4, 2, 3, 5, 7, 1, 3, nullptr, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: out == src", sonar_shuffle_gather_f32(a, a, 4, 2, 3, 5, 7, 1, 3, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: dim == ndim", sonar_shuffle_gather_f32(a, b, 4, 2, 3, 5, 7, 1, 4, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: dim < 0", sonar_shuffle_gather_f32(a, b, 4, 2, 3, 5, 7, 1, -1, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: ndim 0", sonar_shuffle_gather_f32(a, b, 0, 1, 1, 1, 1, 1, 0, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: ndim 6", sonar_shuffle_gather_f32(a, b, 6, 1, 1, 1, 1, 1, 0, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: n == 0", sonar_shuffle_gather_f32(a, b, 4, 2, 3, 5, 0, 1, 3, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: n == 1 with offsets", sonar_shuffle_gather_f32(a, b, 4, 2, 3, 5, 1, 1, 3, idx, 1, nullptr), SONAR_ERR_ARG);
    expect("gather: negative size", sonar_shuffle_gather_f32(a, b, 4, 2, -3, 5, 7, 1, 3, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: size beyond int32", sonar_shuffle_gather_f32(a, b, 2, (int64_t)1 << 40, 2, 1, 1, 1, 1, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: more than 2^31 rows", sonar_shuffle_gather_f32(a, b, 3, 1 << 16, 2, (1 << 15) + 1, 1, 1, 1, idx, 0, nullptr), SONAR_ERR_ARG);
    expect("gather: no rows", sonar_shuffle_gather_f32(a, b, 4, 2, 0, 5, 7, 1, 3, idx, 0, nullptr), SONAR_OK);

    expect("generate: NULL src", sonar_shuffle_generate_f32(nullptr, b, 4, 2, 3, 5, 7, 1, 3, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: NULL out", sonar_shuffle_generate_f32(a, nullptr, 4, 2, 3, 5, 7, 1, 3, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: out == src", sonar_shuffle_generate_f32(a, a, 4, 2, 3, 5, 7, 1, 3, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: dim == ndim", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 7, 1, 4, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: dim < 0", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 7, 1, -2, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: n == 0", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 0, 1, 3, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: n == 1 with no_identity", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 1, 1, 3, 0.5f, 1, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: prob NaN", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 7, 1, 3, __builtin_nanf(""), 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: negative row offset", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 7, 1, 3, 0.5f, 0, 1, 2, -1, nullptr), SONAR_ERR_ARG);
    expect("generate: stream id beyond 48 bits", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 7, 1, 3, 0.5f, 0, 1, (uint64_t)1 << 48, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: row offset beyond 48 bits", sonar_shuffle_generate_f32(a, b, 4, 2, 3, 5, 7, 1, 3, 0.5f, 0, 1, 2, (int64_t)1 << 48, nullptr), SONAR_ERR_ARG);
    expect("generate: more than 2^31 rows", sonar_shuffle_generate_f32(a, b, 3, 1 << 16, 2, (1 << 15) + 1, 1, 1, 1, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_ARG);
    expect("generate: n over the bound", sonar_shuffle_generate_f32(a, b, 2, 3, big, 1, 1, 1, 1, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_UNSUPPORTED);
    expect("generate: n over the bound, other dim", sonar_shuffle_generate_f32(a, b, 3, big, 2, 3, 1, 1, 0, 0.5f, 0, 1, 2, 0, nullptr), SONAR_ERR_UNSUPPORTED);
    expect("generate: no rows", sonar_shuffle_generate_f32(a, b, 4, 2, 0, 5, 7, 1, 3, 0.5f, 0, 1, 2, 0, nullptr), SONAR_OK);

    std::printf("%d calls into the shuffle entry points' validation, %d unexpected return codes\n", calls, bad);
    return bad != 0;
}
