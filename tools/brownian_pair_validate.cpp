// Host-side check of the argument validation of sonar_brownian_pair_f32 (csrc/noise_brownian.hip): the entry point is called with bad
// arguments and with empty outputs only, so every call must come back with its code before anything touches the HIP runtime -- no launch,
// no GPU needed.  Built with the host sanitizers ("Two points from one launch"):
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/brownian_pair_validate.cpp comfyui-sonar_amd/csrc/noise_brownian.hip comfyui-sonar_amd/csrc/runtime.hip -o scratch/bin/brownian_pair_validate
//   ASAN_OPTIONS=detect_leaks=0 scratch/bin/brownian_pair_validate
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/sonar_hip.h"

static int bad = 0, calls = 0;

static void expect(const char* what, int rc, int want) {
    ++calls;
    if (rc != want) {
        std::printf("%s: returned %d, expected %d (%s)\n", what, rc, want, sonar_last_error());
        ++bad;
    }
}

// never dereferenced: the checks refuse every call below, or the output is empty
static float* P(uintptr_t v) { return reinterpret_cast<float*>(v); }

struct Args {
    float *out_1 = P(0x1000), *out_2 = P(0x2000), *w_1 = P(0x3000), *w_2 = P(0x4000);
    const float *prev = P(0x5000), *a_1 = P(0x6000), *b_1 = P(0x7000), *a_2 = P(0x6000), *b_2 = P(0x7000);
    int64_t n = 4096, offs = 0, latent_elems = 4096;
    std::vector<uint64_t> shared, p1{17, 35}, p2{17, 34};
    const uint64_t* latent_seeds = nullptr;
    double *part_1 = nullptr, *part_2 = nullptr;
    int run() const {
        const std::vector<float> c(128, 0.5f);
        return sonar_brownian_pair_f32(out_1, out_2, w_1, w_2, prev, 1.0f, -1.0f, a_1, 0.5f, b_1, 0.5f, a_2, 0.25f, b_2, 0.75f, n, offs, shared.data(),
                                       c.data(), (int)shared.size(), p1.data(), c.data(), (int)p1.size(), p2.data(), c.data(), (int)p2.size(), 5,
                                       latent_seeds, latent_elems, part_1, part_2, nullptr);
    }
};

int main() {
    Args a;
    a = Args(); a.n = 0; expect("n == 0", a.run(), SONAR_OK);
    a = Args(); a.n = 0; a.w_1 = a.w_2 = nullptr; a.prev = nullptr; a.p1.clear(); a.p2.clear(); expect("n == 0, nothing optional", a.run(), SONAR_OK);
    a = Args(); a.out_1 = nullptr; expect("NULL out_1", a.run(), SONAR_ERR_ARG);
    a = Args(); a.out_2 = nullptr; expect("NULL out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.out_2 = a.out_1; expect("out_1 == out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.w_1 = a.out_1; expect("w_out_1 == out_1", a.run(), SONAR_ERR_ARG);
    a = Args(); a.w_2 = a.out_2; expect("w_out_2 == out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.w_2 = a.w_1; expect("w_out_1 == w_out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.prev = a.out_1; expect("prev == out_1", a.run(), SONAR_ERR_ARG);
    a = Args(); a.prev = a.w_2; expect("prev == w_out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.a_1 = a.out_2; expect("base_a_1 == out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.b_1 = a.w_1; expect("base_b_1 == w_out_1", a.run(), SONAR_ERR_ARG);
    a = Args(); a.a_2 = a.out_1; expect("base_a_2 == out_1", a.run(), SONAR_ERR_ARG);
    a = Args(); a.b_2 = a.out_2; expect("base_b_2 == out_2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.n = -1; expect("n < 0", a.run(), SONAR_ERR_ARG);
    a = Args(); a.n = (int64_t)1 << 31; expect("n = 2^31", a.run(), SONAR_ERR_ARG);
    a = Args(); a.offs = -4; expect("elem_offset < 0", a.run(), SONAR_ERR_ARG);
    a = Args(); a.p1 = {35, 17}; expect("a descending private list", a.run(), SONAR_ERR_ARG);
    a = Args(); a.p2 = {17, 17}; expect("a repeated node", a.run(), SONAR_ERR_ARG);
    a = Args(); a.shared = {3, 2}; expect("a descending shared list", a.run(), SONAR_ERR_ARG);
    a = Args(); a.shared = {17}; expect("a shared node on a private list", a.run(), SONAR_ERR_ARG);
    a = Args(); a.p1 = {(uint64_t)1 << 48}; expect("a 49-bit node id", a.run(), SONAR_ERR_ARG);
    a = Args(); a.latent_seeds = reinterpret_cast<const uint64_t*>(0x9000); a.offs = 2; expect("per-latent seeds, offset 2", a.run(), SONAR_ERR_ARG);
    a = Args(); a.latent_seeds = reinterpret_cast<const uint64_t*>(0x9000); a.latent_elems = 6; expect("per-latent seeds, latents of 6", a.run(), SONAR_ERR_ARG);
    std::vector<uint64_t> many;
    for (uint64_t k = 100; k < 148; ++k) many.push_back(k);
    a = Args(); a.n = 0; a.p1 = a.p2 = many; expect("96 terms, empty output", a.run(), SONAR_OK);
    a = Args(); a.p1 = a.p2 = many; a.shared = {7}; expect("97 terms", a.run(), SONAR_ERR_UNSUPPORTED);
    a = Args(); a.n = 0; a.p1 = a.p2 = many; a.p1.push_back(999); expect("97 terms, empty output", a.run(), SONAR_ERR_UNSUPPORTED);
    a = Args(); a.part_1 = reinterpret_cast<double*>(0xA000); a.p1 = {17}; a.p2 = {17, 34, 68, 136};
    expect("statistics across the long-expansion length", a.run(), SONAR_ERR_UNSUPPORTED);

    std::printf("%d calls into sonar_brownian_pair_f32's validation, %d unexpected return codes\n", calls, bad);
    return bad != 0;
}
