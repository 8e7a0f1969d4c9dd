// Host-side check of the argument validation of csrc/voronoi.hip: the entry points are called with bad arguments and with empty outputs only,
// so every call must come back with its code before anything touches the HIP runtime -- no launch, no GPU needed.  Built with the host
// sanitizers ("Voronoi noise"):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/voronoi_validate.cpp comfyui-sonar_amd/csrc/voronoi.hip comfyui-sonar_amd/csrc/runtime.hip -o voronoi_validate
//   ASAN_OPTIONS=detect_leaks=0 ./voronoi_validate
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/sonar_hip.h"

static int bad = 0, calls = 0;

static void expect(const char* what, int rc, int want) {
    ++calls;
    if (rc != want) {
        std::printf("%s: returned %d, expected %d (%s)\n", what, rc, want, sonar_last_error());
        ++bad;
    }
}

// euclidean distance, diff2 result: one term each
static sonar_voronoi_program plain() {
    sonar_voronoi_program p;
    std::memset(&p, 0, sizeof p);
    p.n_d = p.n_r = 1;
    p.d[0].metric = SONAR_VORONOI_D_EUCLIDEAN, p.d[0].idx = 2, p.d[0].scale = 1.0f;
    p.r[0].op = SONAR_VORONOI_R_DIFF2, p.r[0].idx2 = 1, p.r[0].scale = 1.0f;
    return p;
}

// never dereferenced: the checks refuse every call below, or the output is empty
static float* const f = reinterpret_cast<float*>(0x1000);
static float* const o = reinterpret_cast<float*>(0x2000);
static float* const a = reinterpret_cast<float*>(0x3000);

static int run(const sonar_voronoi_program& p, const float* aux = nullptr, int64_t N = 33, int flags = 0) {
    return sonar_voronoi_octave_f32(f, o, aux, 2, 3, 8, 12, N, 1.0f, 0.25f, 1.0f, 1.0f, flags, &p, nullptr);
}

int main() {
    const int64_t two31 = (int64_t)1 << 31;
    const sonar_voronoi_program p = plain();
    expect("NULL fp", sonar_voronoi_octave_f32(nullptr, o, a, 2, 3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("NULL out", sonar_voronoi_octave_f32(f, nullptr, a, 2, 3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("NULL program", sonar_voronoi_octave_f32(f, o, a, 2, 3, 8, 12, 33, 1, 0, 1, 1, 0, nullptr, nullptr), SONAR_ERR_ARG);
    expect("out == fp", sonar_voronoi_octave_f32(f, f, a, 2, 3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("out == aux", run(p, o), SONAR_ERR_ARG);
    expect("B < 0", sonar_voronoi_octave_f32(f, o, a, -2, 3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("C < 0", sonar_voronoi_octave_f32(f, o, a, 2, -3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("H < 0", sonar_voronoi_octave_f32(f, o, a, 2, 3, -8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("W < 0", sonar_voronoi_octave_f32(f, o, a, 2, 3, 8, -12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("N < 0", run(p, nullptr, -1), SONAR_ERR_ARG);
    expect("B = 2^31", sonar_voronoi_octave_f32(f, o, a, two31, 3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("W = 2^31", sonar_voronoi_octave_f32(f, o, a, 2, 3, 8, two31, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("N = 2^31", run(p, nullptr, two31), SONAR_ERR_ARG);
    expect("2^31 planes", sonar_voronoi_octave_f32(f, o, a, 1 << 16, 1 << 15, 1, 1, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("2^31 pixels", sonar_voronoi_octave_f32(f, o, a, 1, 1, 1 << 16, 1 << 15, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("2^31 outputs", sonar_voronoi_octave_f32(f, o, a, 1 << 10, 1 << 10, 1 << 10, 2, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_ERR_ARG);
    expect("N = 0", run(p, nullptr, 0), SONAR_ERR_ARG);
    expect("N = 1", run(p, nullptr, 1), SONAR_ERR_ARG);
    expect("N beyond the cap", run(p, nullptr, SONAR_VORONOI_MAX_POINTS + 1), SONAR_ERR_UNSUPPORTED);
    expect("an unknown flag", run(p, nullptr, 33, 2), SONAR_ERR_ARG);
    sonar_voronoi_program q = p;
    q.n_d = 0; expect("no distance term", run(q), SONAR_ERR_ARG);
    q.n_d = 5; expect("five distance terms", run(q), SONAR_ERR_ARG);
    q = p; q.n_r = 0; expect("no result term", run(q), SONAR_ERR_ARG);
    q.n_r = 5; expect("five result terms", run(q), SONAR_ERR_ARG);
    q = p; q.d[0].metric = 8; expect("an unknown metric", run(q), SONAR_ERR_ARG);
    q.d[0].metric = -1; expect("a negative metric", run(q), SONAR_ERR_ARG);
    q = p; q.d[0].idx = 3; expect("component 3", run(q), SONAR_ERR_ARG);
    q = p; q.d[0].n_xform = 5; expect("five transforms", run(q), SONAR_ERR_ARG);
    q = p; q.d[0].n_xform = 1, q.d[0].xform[0] = 3; expect("an unknown transform", run(q), SONAR_ERR_ARG);
    q = p; q.n_d = 2, q.d[1].metric = 99; expect("an unknown metric in the second term", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].op = 7; expect("an unknown op", run(q), SONAR_ERR_ARG);
    q.r[0].op = -1; expect("a negative op", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].idx1 = 4; expect("idx1 = 4", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].idx2 = -1; expect("idx2 = -1", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].n_fn = 5; expect("five fractal_norms", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].n_ridge = -1; expect("a negative ridge count", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].n_fn = 1, q.r[0].fn[0] = SONAR_VORONOI_X_WEIGHT; expect("weight as a result function", run(q), SONAR_ERR_ARG);
    q = p; q.r[0].op = SONAR_VORONOI_R_CELLID; expect("cellid without aux", run(q), SONAR_ERR_ARG);
    expect("B == 0", sonar_voronoi_octave_f32(f, o, a, 0, 3, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_OK);
    expect("C == 0", sonar_voronoi_octave_f32(f, o, a, 2, 0, 8, 12, 33, 1, 0, 1, 1, 0, &p, nullptr), SONAR_OK);
    expect("H == 0", sonar_voronoi_octave_f32(f, o, a, 2, 3, 0, 12, 0, 1, 0, 1, 1, 0, &p, nullptr), SONAR_OK);
    expect("W == 0", sonar_voronoi_octave_f32(f, o, nullptr, 2, 3, 8, 0, 33, 1, 0, 1, 1, SONAR_VORONOI_FINAL_DIV, &p, nullptr), SONAR_OK);

    uint32_t* const st = reinterpret_cast<uint32_t*>(0x4000);
#define FUZZ(fp_, out_, u_, st_, B_, N_, pass_, term_, fuzz_, sid_, off_) \
    sonar_voronoi_fuzz_octave_f32(fp_, out_, nullptr, u_, st_, B_, 3, 8, 12, N_, 1.0f, 0.25f, 1.0f, 1.0f, 0, &p, pass_, term_, fuzz_, 7, sid_, off_, nullptr)
    expect("fuzz: NULL stats", FUZZ(f, o, a, nullptr, 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: stats == out", FUZZ(f, o, a, reinterpret_cast<uint32_t*>(o), 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: stats == fp", FUZZ(f, o, a, reinterpret_cast<uint32_t*>(f), 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: stats == u", FUZZ(f, o, a, reinterpret_cast<uint32_t*>(a), 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: u == out", FUZZ(f, o, o, st, 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: pass -1", FUZZ(f, o, a, st, 2, 33, -1, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: pass 3", FUZZ(f, o, a, st, 2, 33, 3, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: term beyond the program", FUZZ(f, o, a, st, 2, 33, 2, 1, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: term -1", FUZZ(f, o, a, st, 2, 33, 2, -1, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: fuzz NaN", FUZZ(f, o, a, st, 2, 33, 2, 0, 0.0 / 0.0, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: elem_offset < 0", FUZZ(f, o, a, st, 2, 33, 2, 0, 0.1, 5, -1), SONAR_ERR_ARG);
    expect("fuzz: elem_offset 2^48", FUZZ(f, o, a, st, 2, 33, 2, 0, 0.1, 5, (int64_t)1 << 48), SONAR_ERR_ARG);
    expect("fuzz: stream id 2^48", FUZZ(f, o, a, st, 2, 33, 2, 0, 0.1, (uint64_t)1 << 48, 0), SONAR_ERR_ARG);
    expect("fuzz: NULL fp", FUZZ(nullptr, o, a, st, 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: NULL out in the real pass", FUZZ(f, nullptr, a, st, 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: out == fp", FUZZ(f, f, a, st, 2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: N = 1", FUZZ(f, o, a, st, 2, 1, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: N beyond the cap", FUZZ(f, o, a, st, 2, SONAR_VORONOI_MAX_POINTS + 1, 2, 0, 0.1, 5, 0), SONAR_ERR_UNSUPPORTED);
    expect("fuzz: B < 0", FUZZ(f, o, a, st, -2, 33, 2, 0, 0.1, 5, 0), SONAR_ERR_ARG);
    expect("fuzz: B == 0, pass 0 without an output", FUZZ(f, nullptr, nullptr, st, 0, 33, 0, 0, 0.1, 5, 0), SONAR_OK);
    expect("fuzz: B == 0, pass 1", FUZZ(f, nullptr, a, st, 0, 33, 1, 0, 0.1, 5, 0), SONAR_OK);
    expect("fuzz: B == 0, pass 2", FUZZ(f, o, a, st, 0, 33, 2, 0, 0.1, 5, 0), SONAR_OK);
#undef FUZZ
    expect("gradient: NULL r1", sonar_voronoi_gradient_f32(nullptr, f, o, 6, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: NULL r2", sonar_voronoi_gradient_f32(f, nullptr, o, 6, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: NULL acc", sonar_voronoi_gradient_f32(f, f, nullptr, 6, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: acc == r1", sonar_voronoi_gradient_f32(f, a, f, 6, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: acc == r2", sonar_voronoi_gradient_f32(a, f, f, 6, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: planes < 0", sonar_voronoi_gradient_f32(f, f, o, -6, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: H < 0", sonar_voronoi_gradient_f32(f, f, o, 6, -8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: W < 0", sonar_voronoi_gradient_f32(f, f, o, 6, 8, -12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: planes = 2^31", sonar_voronoi_gradient_f32(f, f, o, two31, 8, 12, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: 2^31 pixels", sonar_voronoi_gradient_f32(f, f, o, 1, 1 << 16, 1 << 15, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: 2^31 values", sonar_voronoi_gradient_f32(f, f, o, 1 << 10, 1 << 11, 1 << 10, 1.0f, nullptr), SONAR_ERR_ARG);
    expect("gradient: planes == 0", sonar_voronoi_gradient_f32(f, f, o, 0, 8, 12, 1.0f, nullptr), SONAR_OK);
    expect("gradient: W == 0", sonar_voronoi_gradient_f32(f, f, o, 6, 8, 0, 1.0f, nullptr), SONAR_OK);
    expect("fuzz_add: NULL x", sonar_voronoi_fuzz_add_f32(nullptr, f, 8, 0.5f, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("fuzz_add: NULL u", sonar_voronoi_fuzz_add_f32(o, nullptr, 8, 0.5f, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("fuzz_add: x == u", sonar_voronoi_fuzz_add_f32(o, o, 8, 0.5f, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("fuzz_add: n < 0", sonar_voronoi_fuzz_add_f32(o, f, -1, 0.5f, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("fuzz_add: n = 2^31", sonar_voronoi_fuzz_add_f32(o, f, two31, 0.5f, 0.25f, nullptr), SONAR_ERR_ARG);
    expect("fuzz_add: n == 0", sonar_voronoi_fuzz_add_f32(o, f, 0, 0.5f, 0.25f, nullptr), SONAR_OK);
    expect("acc: NULL acc", sonar_voronoi_acc_f32(nullptr, f, 8, 1.0f, 1.0f, 0, nullptr), SONAR_ERR_ARG);
    expect("acc: NULL x", sonar_voronoi_acc_f32(o, nullptr, 8, 1.0f, 1.0f, 0, nullptr), SONAR_ERR_ARG);
    expect("acc: acc == x", sonar_voronoi_acc_f32(o, o, 8, 1.0f, 1.0f, 0, nullptr), SONAR_ERR_ARG);
    expect("acc: n < 0", sonar_voronoi_acc_f32(o, f, -1, 1.0f, 1.0f, 0, nullptr), SONAR_ERR_ARG);
    expect("acc: n = 2^31", sonar_voronoi_acc_f32(o, f, two31, 1.0f, 1.0f, 0, nullptr), SONAR_ERR_ARG);
    expect("acc: an unknown flag", sonar_voronoi_acc_f32(o, f, 8, 1.0f, 1.0f, 2, nullptr), SONAR_ERR_ARG);
    expect("acc: n == 0", sonar_voronoi_acc_f32(o, f, 0, 1.0f, 1.0f, SONAR_VORONOI_FINAL_DIV, nullptr), SONAR_OK);

    std::printf("%d calls into the Voronoi entry points' validation, %d unexpected return codes\n", calls, bad);
    return bad != 0;
}
