// Host-side check of the argument validation of csrc/pattern_break.hip: the entry point is called with bad arguments only, so every call
// must come back with its error code before anything touches the HIP runtime -- no launch, no GPU needed.  Built with the host sanitizers
// ("Pattern-break"):
//
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/pattern_break_validate.cpp comfyui-sonar_amd/csrc/pattern_break.hip \
//       comfyui-sonar_amd/csrc/runtime.hip -o pattern_break_validate
//   ASAN_OPTIONS=detect_leaks=0 ./pattern_break_validate
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
    float* const x = reinterpret_cast<float*>(0x1000);
    float* const out = reinterpret_cast<float*>(0x2000);
    float* const ws = reinterpret_cast<float*>(0x3000);
    double* const st = reinterpret_cast<double*>(0x4000);
    float* const odd = reinterpret_cast<float*>(0x1002);
    double* const odd8 = reinterpret_cast<double*>(0x4004);
    const int64_t W = SONAR_PATTERN_BREAK_WS;
    const int L = SONAR_BLEND_LERP, A = SONAR_PATTERN_BREAK_AUTO;

    expect("NULL x", sonar_pattern_break_f32(nullptr, out, 100, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("NULL out", sonar_pattern_break_f32(x, nullptr, 100, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("NULL ws", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, nullptr, W, st, nullptr), SONAR_ERR_ARG);
    expect("misaligned x", sonar_pattern_break_f32(odd, out, 100, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("misaligned out", sonar_pattern_break_f32(x, odd, 100, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("misaligned ws", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, odd, W, st, nullptr), SONAR_ERR_ARG);
    expect("misaligned stats", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, ws, W, odd8, nullptr), SONAR_ERR_ARG);
    expect("out == x", sonar_pattern_break_f32(x, x, 100, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("ws == x", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, x, W, st, nullptr), SONAR_ERR_ARG);
    expect("ws == out", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, out, W, st, nullptr), SONAR_ERR_ARG);
    expect("n == 0", sonar_pattern_break_f32(x, out, 0, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("n < 0", sonar_pattern_break_f32(x, out, -7, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("n = INT64_MIN", sonar_pattern_break_f32(x, out, INT64_MIN, 1.0f, 0.5f, L, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("blend mode 3", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, 3, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("blend mode -1", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, -1, 1, A, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("route 3", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, 3, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("route -1", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, -1, ws, W, st, nullptr), SONAR_ERR_ARG);
    expect("workspace one float short", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, ws, W - 1, st, nullptr), SONAR_ERR_ARG);
    expect("workspace of 0", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, ws, 0, st, nullptr), SONAR_ERR_ARG);
    expect("workspace negative", sonar_pattern_break_f32(x, out, 100, 1.0f, 0.5f, L, 1, A, ws, -W, st, nullptr), SONAR_ERR_ARG);
    for (int route = SONAR_PATTERN_BREAK_ONE; route <= SONAR_PATTERN_BREAK_THREE; ++route)
        for (int restore = 0; restore < 2; ++restore) {
            expect("forced route: NULL x", sonar_pattern_break_f32(nullptr, out, 100, 1.0f, 0.5f, L, restore, route, ws, W, nullptr, nullptr), SONAR_ERR_ARG);
            expect("forced route: n == 0", sonar_pattern_break_f32(x, out, 0, 1.0f, 0.5f, L, restore, route, ws, W, nullptr, nullptr), SONAR_ERR_ARG);
        }

    // the route query is pure host arithmetic
    expect("route(1)", sonar_pattern_break_route(1), SONAR_PATTERN_BREAK_ONE);
    expect("route(limit)", sonar_pattern_break_route(SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX), SONAR_PATTERN_BREAK_ONE);
    expect("route(limit + 1)", sonar_pattern_break_route((int64_t)SONAR_PATTERN_BREAK_ONE_LAUNCH_MAX + 1), SONAR_PATTERN_BREAK_THREE);
    expect("route(INT64_MAX)", sonar_pattern_break_route(INT64_MAX), SONAR_PATTERN_BREAK_THREE);

    std::printf("%d calls into the pattern-break entry points' validation, %d unexpected return codes\n", calls, bad);
    return bad != 0;
}
