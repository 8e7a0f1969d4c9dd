// ShuffledNoise (utils.elementwise_shuffle_by_dim, py/utils.py:599-657): every row of a contiguous fp32 tensor permuted along one dimension,
// on the tensor as it lies.  A contiguous tensor shuffled along `dim` is [outer][n][inner]: row r = o * inner + i holds the values at
// (o * n + j) * inner + i, j < n.  Two kernels:
//   shuffle_gather_kernel    replay mode: the permutation is the host's (an index table or one rotation per row).  One thread per OUTPUT
//                            element in memory order, so the stores are whole lines whatever `dim` is: with inner > 1 the lanes of a wave are
//                            adjacent rows, with inner == 1 they walk along one row.
//   shuffle_generate_kernel  generate mode: the mask variate, the rotation or the n sort keys of a row are Philox4x32-10 words of
//                            (seed, stream, global row) -- INTEGRATION.md 3b.  A workgroup owns `tr` consecutive rows; the keys live in LDS
//                            ([j][row] for inner > 1, where lanes are rows; [row][j] for inner == 1, where lanes walk a row), each value is
//                            read once, ranked by (key, j) against the row's keys and stored at its rank.  No table reaches memory.
// Every output value is an input value: nothing here rounds.
#include "common.h"

namespace sonar {

namespace {

constexpr int kMaxN = SONAR_SHUFFLE_MAX_N;
constexpr int kKeyBudget = 8192;  // key words of LDS per workgroup (32 KB): rows per tile x n
constexpr int kMaxTileRows = 64;
static_assert(kMaxN <= kKeyBudget, "one row of the longest dimension fits the key tile");

struct Geometry {
    int64_t outer, n, inner, rows;
};

// (counter, key) of the shuffle's Philox blocks: the distro kernels' layout under a domain of its own
struct ShuffleKey {
    uint32_t c0, c1, c3, k0, k1;
    __device__ __forceinline__ ShuffleKey(uint64_t seed, uint64_t stream_id, uint64_t row)
        : c0((uint32_t)row), c1((uint32_t)(row >> 32) | ((uint32_t)(stream_id >> 32) << 16)), c3((uint32_t)stream_id), k0((uint32_t)seed),
          k1((uint32_t)(seed >> 32) ^ SONAR_SHUFFLE_DOMAIN) {}
    __device__ __forceinline__ Philox4 block(uint32_t b) const { return philox4x32_10(c0, c1, b, c3, k0, k1); }
};

template <typename I, bool OFFSETS>
__global__ void __launch_bounds__(kBlock) shuffle_gather_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                                const int32_t* __restrict__ idx, I total, I n, I inner) {
    for (I f = (I)blockIdx.x * kBlock + threadIdx.x; f < total; f += (I)gridDim.x * kBlock) {
        const I oj = inner == 1 ? f : f / inner, i = inner == 1 ? 0 : f - oj * inner;
        const I o = oj / n, j = oj - o * n;
        const I r = o * inner + i;
        I sj;
        if constexpr (OFFSETS) {
            const int32_t off = idx[r];
            sj = off < 0 ? j : (j + (I)off % n) % n;
        } else {
            const int32_t e = idx[r * n + j];
            sj = e < 0 ? 0 : ((I)e < n ? (I)e : n - 1);  // the table is the caller's: an entry outside [0, n) must not become an address
        }
        out[f] = src[(o * n + sj) * inner + i];
    }
}

// `tr` rows per tile and kBlock / tr lanes per row, both powers of two.  LAST (inner == 1): a row's lanes are adjacent threads.  Otherwise the
// rows of a tile are adjacent threads, and a row's lanes are kBlock / tr waves or parts of waves apart.
template <bool LAST>
__global__ void __launch_bounds__(kBlock) shuffle_generate_kernel(const float* __restrict__ src, float* __restrict__ out, int64_t rows, int n,
                                                                  int64_t inner, int tr, float prob, int no_identity, uint64_t seed,
                                                                  uint64_t stream_id, int64_t row_offset) {
    kernarg_touch_for(src, out, rows, n, inner, tr, prob, no_identity, seed, stream_id, row_offset);
    __shared__ uint32_t keys[kKeyBudget];
    __shared__ int what[kMaxTileRows];  // per row of the tile: -1 copy, 0 rank the keys, > 0 the rotation
    const int per_row = kBlock / tr;
    const int rl = LAST ? (int)threadIdx.x / per_row : (int)threadIdx.x % tr;
    const int sl = LAST ? (int)threadIdx.x % per_row : (int)threadIdx.x / tr;
    const int64_t tiles = (rows + tr - 1) / tr;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if ((int)threadIdx.x < tr) {
            const int64_t r = tile * tr + threadIdx.x;
            int w = -1;
            if (r < rows) {
                const uint64_t row = (uint64_t)(row_offset + r);
                const bool shuffled = prob >= 1.0f || u01(ShuffleKey(seed, stream_id, row).block(0).v[0]) < prob;
                if (shuffled)
                    w = no_identity ? 1 + (int)(((uint64_t)(ShuffleKey(seed, stream_id + 1, row).block(0).v[0] >> 8) * (uint64_t)(n - 1)) >> 24) : 0;
            }
            what[threadIdx.x] = w;
        }
        __syncthreads();
        const int64_t r = tile * tr + rl;
        const bool live = r < rows;
        const int w = what[rl];
        uint32_t* const mine = LAST ? keys + rl * n : keys + rl;  // key j of this thread's row: mine[j * kstride]
        const int kstride = LAST ? 1 : tr;
        if (!no_identity) {
            if (live && w == 0) {
                const ShuffleKey key(seed, stream_id + 2, (uint64_t)(row_offset + r));
                for (int b = sl; 4 * b < n; b += per_row) {
                    const Philox4 p = key.block((uint32_t)b);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (4 * b + q < n) mine[(4 * b + q) * kstride] = p.v[q] >> 8;
                }
            }
            __syncthreads();
        }
        if (live) {
            const int64_t o = r / inner;
            const int64_t base = o * n * inner + (r - o * inner);
            for (int j = sl; j < n; j += per_row) {
                const float v = src[base + j * inner];
                int dst;
                if (w < 0) {
                    dst = j;
                } else if (w > 0) {  // out[j] = src[(j + w) % n]: value j goes to j - w
                    dst = j - w;
                    if (dst < 0) dst += n;
                } else {  // the rank of (key j, j) among the row's keys: ties go to the lower index
                    // keys are 24 bits: "key k <= key j" below j is "key k < key j + 1"; key j itself counts nothing
                    const uint32_t kj = mine[j * kstride];
                    dst = 0;
#pragma unroll 8
                    for (int k = 0; k < n; ++k) dst += mine[k * kstride] < kj + (uint32_t)(k < j);
                }
                out[base + dst * inner] = v;
            }
        }
        __syncthreads();  // the next tile overwrites the keys
    }
}

// the checks both entry points share; fills `g`
int geometry(const char* who, const void* src, const void* out, int ndim, const int64_t (&s)[5], int dim, Geometry& g) {
    SONAR_REQUIRE(src != nullptr && out != nullptr, SONAR_ERR_ARG, "%s: NULL tensor", who);
    SONAR_REQUIRE(src != out, SONAR_ERR_ARG, "%s: out must not be src", who);
    SONAR_REQUIRE(ndim >= 1 && ndim <= 5, SONAR_ERR_ARG, "%s: %d dimensions (1..5)", who, ndim);
    SONAR_REQUIRE(dim >= 0 && dim < ndim, SONAR_ERR_ARG, "%s: dim %d outside [0, %d)", who, dim, ndim);
    g.outer = g.inner = 1;
    for (int d = 0; d < ndim; ++d) {
        SONAR_REQUIRE(s[d] >= 0 && s[d] <= INT32_MAX, SONAR_ERR_ARG, "%s: size %lld of dimension %d", who, (long long)s[d], d);
        if (d == dim) continue;
        int64_t& part = d < dim ? g.outer : g.inner;
        part *= s[d];
        SONAR_REQUIRE(g.outer * g.inner <= ((int64_t)1 << 31), SONAR_ERR_ARG, "%s: more than 2^31 rows", who);
    }
    g.n = s[dim];
    g.rows = g.outer * g.inner;
    SONAR_REQUIRE(g.n >= 1, SONAR_ERR_ARG, "%s: dimension %d is empty", who, dim);
    return SONAR_OK;
}

}  // namespace

}  // namespace sonar

extern "C" int sonar_shuffle_gather_f32(const float* src, float* out, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                        int dim, const int32_t* idx, int idx_is_offset, void* stream) {
    using namespace sonar;
    const int64_t s[5] = {s0, s1, s2, s3, s4};
    Geometry g;
    if (const int rc = geometry("sonar_shuffle_gather_f32", src, out, ndim, s, dim, g)) return rc;
    SONAR_REQUIRE(idx != nullptr, SONAR_ERR_ARG, "sonar_shuffle_gather_f32: NULL index");
    SONAR_REQUIRE(!idx_is_offset || g.n >= 2, SONAR_ERR_ARG, "sonar_shuffle_gather_f32: a rotation needs at least 2 values per row");
    if (g.rows == 0) return SONAR_OK;
    const int64_t total = g.rows * g.n;
    const dim3 grid(grid_for(total, kBlock)), block(kBlock);
    const hipStream_t st = (hipStream_t)stream;
    if (total <= (int64_t)INT32_MAX) {  // (the grid stride added to an index below the total stays below 2^32)
        if (idx_is_offset)
            hipLaunchKernelGGL((shuffle_gather_kernel<uint32_t, true>), grid, block, 0, st, src, out, idx, (uint32_t)total, (uint32_t)g.n, (uint32_t)g.inner);
        else
            hipLaunchKernelGGL((shuffle_gather_kernel<uint32_t, false>), grid, block, 0, st, src, out, idx, (uint32_t)total, (uint32_t)g.n, (uint32_t)g.inner);
    } else {
        if (idx_is_offset)
            hipLaunchKernelGGL((shuffle_gather_kernel<int64_t, true>), grid, block, 0, st, src, out, idx, total, g.n, g.inner);
        else
            hipLaunchKernelGGL((shuffle_gather_kernel<int64_t, false>), grid, block, 0, st, src, out, idx, total, g.n, g.inner);
    }
    return check_launch("sonar_shuffle_gather_f32");
}

extern "C" int sonar_shuffle_generate_f32(const float* src, float* out, int ndim, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int64_t s4,
                                          int dim, float prob, int no_identity, uint64_t seed, uint64_t stream_id, int64_t row_offset,
                                          void* stream) {
    using namespace sonar;
    const int64_t s[5] = {s0, s1, s2, s3, s4};
    Geometry g;
    if (const int rc = geometry("sonar_shuffle_generate_f32", src, out, ndim, s, dim, g)) return rc;
    SONAR_REQUIRE(!no_identity || g.n >= 2, SONAR_ERR_ARG, "sonar_shuffle_generate_f32: a rotation needs at least 2 values per row");
    SONAR_REQUIRE(prob == prob, SONAR_ERR_ARG, "sonar_shuffle_generate_f32: prob is NaN");
    SONAR_REQUIRE(row_offset >= 0 && (uint64_t)row_offset + (uint64_t)g.rows < ((uint64_t)1 << 48) && stream_id < ((uint64_t)1 << 48) - 2,
                  SONAR_ERR_ARG, "sonar_shuffle_generate_f32: row offset or stream id beyond 48 bits");
    SONAR_REQUIRE(no_identity || g.n <= kMaxN, SONAR_ERR_UNSUPPORTED, "sonar_shuffle_generate_f32: %lld values per row, at most %d",
                  (long long)g.n, kMaxN);
    if (g.rows == 0) return SONAR_OK;
    const bool last = g.inner == 1;
    int tr;
    if (last) {  // a row to the smallest power of two of lanes that covers it, at most the workgroup
        int per_row = kBlock / kMaxTileRows;
        while (per_row < kBlock && per_row < g.n) per_row *= 2;
        tr = kBlock / per_row;
    } else {     // lanes across rows: as many rows as the key tile holds
        tr = kMaxTileRows;
        while (!no_identity && (int64_t)tr * g.n > kKeyBudget) tr /= 2;
    }
    const dim3 grid(grid_for((g.rows + tr - 1) / tr, 1)), block(kBlock);
    if (last)
        hipLaunchKernelGGL(shuffle_generate_kernel<true>, grid, block, 0, (hipStream_t)stream, src, out, g.rows, (int)g.n, g.inner, tr, prob,
                           no_identity ? 1 : 0, seed, stream_id, row_offset);
    else
        hipLaunchKernelGGL(shuffle_generate_kernel<false>, grid, block, 0, (hipStream_t)stream, src, out, g.rows, (int)g.n, g.inner, tr, prob,
                           no_identity ? 1 : 0, seed, stream_id, row_offset);
    return check_launch("sonar_shuffle_generate_f32");
}
