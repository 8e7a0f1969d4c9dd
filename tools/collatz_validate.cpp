// Host-side check of the argument validation of csrc/collatz.hip: both entry points are called with bad arguments and with empty views only,
// so every call must come back with its code before anything touches the HIP runtime -- no launch, no GPU needed.  Built with the host
// sanitizers ("Collatz noise"):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/collatz_validate.cpp comfyui-sonar_amd/csrc/collatz.hip comfyui-sonar_amd/csrc/runtime.hip -o collatz_validate
//   ASAN_OPTIONS=detect_leaks=0 ./collatz_validate
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

// the scalars of a default call: span, rmin, the four multipliers / additions, flags, seed_mode, output, stream
#define DEFAULTS 16001.0, -8000.0, 0.5, 0.0, 3.0, 1.0, 7, 0, 0, nullptr

int main() {
    // never dereferenced: the checks refuse every call below, or the view is empty
    float* const s = reinterpret_cast<float*>(0x1000);
    float* const e = reinterpret_cast<float*>(0x2000);
    float* const o = reinterpret_cast<float*>(0x3000);
    const int64_t two16 = (int64_t)1 << 16, two32 = (int64_t)1 << 32;

    expect("chain: NULL seeds", sonar_collatz_chain_f32(nullptr, e, o, 6, 10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: NULL seed_ext", sonar_collatz_chain_f32(s, nullptr, o, 6, 10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: NULL out", sonar_collatz_chain_f32(s, e, nullptr, 6, 10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: out == seeds", sonar_collatz_chain_f32(s, e, s, 6, 10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: out == seed_ext", sonar_collatz_chain_f32(s, e, e, 6, 10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: outer < 0", sonar_collatz_chain_f32(s, e, o, -6, 10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: len < 0", sonar_collatz_chain_f32(s, e, o, 6, -10, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: inner < 0", sonar_collatz_chain_f32(s, e, o, 6, 10, -1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: a size beyond 2^31", sonar_collatz_chain_f32(s, e, o, 1, two32, 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: chain_length 0", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, 0, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: chain_length < 0", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, -4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: chain_offset < 0", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, 4, -1, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: chain_offset beyond 2^31", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, 4, two32, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: more than 2^31 (outer, inner) pairs", sonar_collatz_chain_f32(s, e, o, two16, 4, (1 << 15) + 1, 4, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: more than 2^31 chains", sonar_collatz_chain_f32(s, e, o, two16, two16, 1, 1, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: more than 2^40 values", sonar_collatz_chain_f32(s, e, o, two16, (int64_t)1 << 30, 1, (int64_t)1 << 16, 5, DEFAULTS), SONAR_ERR_ARG);
    expect("chain: an unknown flag", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, 4, 5, 16001.0, -8000.0, 0.5, 0.0, 3.0, 1.0, 8, 0, 0, nullptr), SONAR_ERR_ARG);
    expect("chain: an unknown seed mode", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, 4, 5, 16001.0, -8000.0, 0.5, 0.0, 3.0, 1.0, 7, 3, 0, nullptr), SONAR_ERR_ARG);
    expect("chain: an unknown output", sonar_collatz_chain_f32(s, e, o, 6, 10, 1, 4, 5, 16001.0, -8000.0, 0.5, 0.0, 3.0, 1.0, 7, 0, -1, nullptr), SONAR_ERR_ARG);
    expect("chain: outer == 0", sonar_collatz_chain_f32(s, e, o, 0, 10, 1, 4, 5, DEFAULTS), SONAR_OK);
    expect("chain: len == 0", sonar_collatz_chain_f32(s, e, o, 6, 0, 1, 4, 5, DEFAULTS), SONAR_OK);
    expect("chain: inner == 0", sonar_collatz_chain_f32(s, e, o, 6, 10, 0, 4, 5, DEFAULTS), SONAR_OK);

    expect("mix: NULL acc", sonar_collatz_mix_f32(nullptr, o, s, SONAR_COLLATZ_SECOND_SEEDS, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: NULL out1", sonar_collatz_mix_f32(e, nullptr, s, SONAR_COLLATZ_SECOND_SEEDS, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: NULL seeds", sonar_collatz_mix_f32(e, o, nullptr, SONAR_COLLATZ_SECOND_SEEDS, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: NULL mix noise", sonar_collatz_mix_f32(e, o, nullptr, SONAR_COLLATZ_SECOND_MIX, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: acc == out1", sonar_collatz_mix_f32(o, o, s, SONAR_COLLATZ_SECOND_SEEDS, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: acc == second", sonar_collatz_mix_f32(s, o, s, SONAR_COLLATZ_SECOND_MIX, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: an unknown mode", sonar_collatz_mix_f32(e, o, s, 3, 6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: outer < 0", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_SEEDS, -6, 10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: len < 0", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_SEEDS, 6, -10, 1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: inner < 0", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_SEEDS, 6, 10, -1, 4, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: chain_length 0", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_SEEDS, 6, 10, 1, 0, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: more than 2^31 chains", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_SEEDS, two16, two16, 1, 1, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("mix: outer == 0", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_SEEDS, 0, 10, 1, 4, 0.25f, nullptr), SONAR_OK);
    expect("mix: len == 0", sonar_collatz_mix_f32(e, o, nullptr, SONAR_COLLATZ_SECOND_ONE, 6, 0, 1, 4, 0.25f, nullptr), SONAR_OK);
    expect("mix: inner == 0", sonar_collatz_mix_f32(e, o, s, SONAR_COLLATZ_SECOND_MIX, 6, 10, 0, 4, 0.25f, nullptr), SONAR_OK);

    std::printf("%d calls into the Collatz entry points' validation, %d unexpected return codes\n", calls, bad);
    return bad != 0;
}
