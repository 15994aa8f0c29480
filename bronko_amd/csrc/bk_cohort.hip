// bk_cohort.hip -- pairwise distances of a cohort of consensus sequences (bk_cohort_set, bk_cohort_distances, bk_cohort_clear;
// `bronko call --distances`): for every pair of samples the positions at which both letters are one of ACGT (compared) and those of
// them at which the two differ (diff).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section W; bronko_amd/host/cohort.cpp and tests/cohort_ref.py restate it.
//   cohort_pack_kernel    letters -> three bit planes per sample: valid, b0, b1 ((b0, b1) = the 2-bit base code A C G T = 0 1 2 3, zero where
//                         not valid).  One wave takes 64 consecutive positions of one sample: a lane per position (a byte load; a sample's
//                         row starts at s * positions, aligned to nothing), three ballots, lane 0 stores the three words.  A lane at or
//                         behind `positions` loads nothing and votes 0, so the tail word's upper bits are zero whatever follows the row.
//                         The planes lie word-major, [plane][word][n_stride]: the 64 samples of a tile's side are 512 contiguous bytes of
//                         every word.  n_stride = n rounded up to 64, plus 64; the padding is zero (valid = 0: it counts nothing), so the
//                         pairs kernel loads whole tiles from any row0 without a bound check.
//   cohort_pairs_kernel   shaped like a GEMM over popcounts.  A workgroup of 256 lanes owns 64 row samples x 64 column samples over one
//                         slice of the words; lane (tx, ty) = (t & 15, t >> 4) holds the 4 x 4 pairs of rows ty + 16 i and columns
//                         tx + 16 j in registers (32 counters).  Per step it stages kChunk words of the 128 samples' three planes in LDS
//                         (24 KB, word-major like the planes: coalesced loads, consecutive LDS writes) and then reads, per word, 12 row and
//                         12 column words (ds_read_b64) for 16 pairs.  In a half wave the 16 tx read 16 consecutive 8-byte words (32 banks,
//                         each once; the two ty of the half wave read them again: a broadcast) and the rows are two addresses read by 16
//                         lanes each (broadcasts): no bank conflict, and no padding needed for it.  Per pair and word
//                         c = v_i & v_j, d = c & ((b0_i ^ b0_j) | (b1_i ^ b1_j)), compared += popcount(c), diff += popcount(d).
//                         The grid is tiles x position slices: with few samples the tiles alone do not fill the device, so the words are
//                         cut into slices and every workgroup adds its partial sums to the output block, which is zeroed on the stream
//                         before the launch, with one atomicAdd per pair and counter (none for a zero).  Integer sums: exact in any order.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "bk_engine.h"

namespace bk {
namespace {

constexpr int kCohortBlock = 256;
constexpr int kTile = 64;                   // samples of a tile's side
constexpr int kChunk = 8;                   // words staged per step, at most
constexpr uint64_t kTargetGroups = 2048;    // workgroups wanted in a launch: slices are cut until tiles x slices reaches it

__global__ __launch_bounds__(kCohortBlock) void cohort_pack_kernel(const uint8_t* __restrict__ letters, uint64_t s0, uint64_t ns, uint64_t positions,
                                                                   uint64_t W, uint64_t n_stride, unsigned long long* __restrict__ planes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * (kCohortBlock / 64) + (threadIdx.x >> 6);   // (wave-uniform)
    const uint64_t pos = w * 64 + lane;
    const bool in = w < W && pos < positions;
    for (uint64_t s = blockIdx.y; s < ns; s += gridDim.y) {
        const uint8_t ch = in ? letters[s * positions + pos] : (uint8_t)0;
        const bool a = ch == 'A', c = ch == 'C', g = ch == 'G', t = ch == 'T';
        const unsigned long long v = __ballot(a || c || g || t), b0 = __ballot(c || t), b1 = __ballot(g || t);
        if (lane == 0 && w < W) {
            const size_t at = (size_t)w * n_stride + (size_t)(s0 + s), plane = (size_t)W * n_stride;
            planes[at] = v; planes[plane + at] = b0; planes[2 * plane + at] = b1;
        }
    }
}

struct PairsArgs {
    const unsigned long long* planes;       // [3][W][n_stride]
    uint64_t n, n_stride, W;
    uint64_t row0, n_rows;
    uint32_t n_col_tiles;
    uint32_t slice_words, chunk;            // words of a slice; words staged per step (1..kChunk)
    unsigned int* diff;                     // [n_rows][n]
    unsigned int* compared;                 // [n_rows][n]
};

__global__ __launch_bounds__(kCohortBlock) void cohort_pairs_kernel(PairsArgs a) {
    __shared__ unsigned long long lds[3 * kChunk * 2 * kTile];   // [plane][word of the chunk][rows 0..63 | columns 0..63]
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t ct = blockIdx.x % a.n_col_tiles, rt = blockIdx.x / a.n_col_tiles;
    const uint64_t row_base = a.row0 + (uint64_t)rt * kTile, col_base = (uint64_t)ct * kTile;   // (both + 63 < n_stride)
    const uint64_t w_lo = (uint64_t)blockIdx.y * a.slice_words, w_hi = std::min<uint64_t>(a.W, w_lo + a.slice_words);
    const size_t plane = (size_t)a.W * a.n_stride;

    unsigned int cmp[4][4], dif[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { cmp[i][j] = 0; dif[i][j] = 0; }

    for (uint64_t w0 = w_lo; w0 < w_hi; w0 += a.chunk) {
        const uint32_t L = (uint32_t)std::min<uint64_t>(a.chunk, w_hi - w0);
        __syncthreads();   // (the previous step's reads are done)
        for (uint32_t idx = t; idx < L * 2 * kTile; idx += kCohortBlock) {
            const uint32_t s = idx & 63u, side = (idx >> 6) & 1u, w = idx >> 7;
            const size_t at = (size_t)(w0 + w) * a.n_stride + (side ? col_base : row_base) + s;
#pragma unroll
            for (int p = 0; p < 3; p++) lds[p * kChunk * 2 * kTile + idx] = a.planes[p * plane + at];
        }
        __syncthreads();
        for (uint32_t w = 0; w < L; w++) {
            const unsigned long long* v = lds + w * 2 * kTile;
            const unsigned long long* b0 = v + kChunk * 2 * kTile;
            const unsigned long long* b1 = b0 + kChunk * 2 * kTile;
            unsigned long long rv[4], r0[4], r1[4], cv[4], c0[4], c1[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                rv[i] = v[ty + 16 * i]; r0[i] = b0[ty + 16 * i]; r1[i] = b1[ty + 16 * i];
                cv[i] = v[kTile + tx + 16 * i]; c0[i] = b0[kTile + tx + 16 * i]; c1[i] = b1[kTile + tx + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const unsigned long long c = rv[i] & cv[j];
                    const unsigned long long d = c & ((r0[i] ^ c0[j]) | (r1[i] ^ c1[j]));
                    cmp[i][j] += (unsigned int)__popcll(c);
                    dif[i][j] += (unsigned int)__popcll(d);
                }
        }
    }

#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t row = row_base + ty + 16 * i;
        if (row >= a.row0 + a.n_rows) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t col = col_base + tx + 16 * j;
            if (col >= a.n) continue;
            const size_t at = (size_t)(row - a.row0) * a.n + col;
            if (cmp[i][j]) atomicAdd(a.compared + at, cmp[i][j]);
            if (dif[i][j]) atomicAdd(a.diff + at, dif[i][j]);
        }
    }
}

}  // namespace
}  // namespace bk

// ---- the C ABI (extern "C" by the declarations in bronko_hip.h) ---------------------------------------------------------------------
int bk_cohort_clear(bk_engine* e) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_clear: e is null");
    if (!e->cohort) return BK_OK;
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));
    e->cohort.reset();
    return BK_OK;
}

int bk_cohort_set(bk_engine* e, const uint8_t* letters, uint64_t n_samples, uint64_t positions) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_set: e is null");
    if (!letters) return fail(BK_ERR_INVALID, "bk_cohort_set: letters is null");
    if (n_samples == 0) return fail(BK_ERR_INVALID, "bk_cohort_set: n_samples must be at least 1");
    if (n_samples > BK_COHORT_MAX_SAMPLES) return fail(BK_ERR_INVALID, "bk_cohort_set: n_samples must be at most %llu, got %llu", (unsigned long long)BK_COHORT_MAX_SAMPLES, (unsigned long long)n_samples);
    if (positions == 0) return fail(BK_ERR_INVALID, "bk_cohort_set: positions must be at least 1");
    if (positions >= (1ull << 32)) return fail(BK_ERR_INVALID, "bk_cohort_set: positions must be below 2^32, got %llu", (unsigned long long)positions);
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_cohort_set inside a sample: it comes before bk_sample_begin or after the sample's downloads");
    if (int rc = bk_cohort_clear(e)) return rc;   // (nothing of the old cohort stays, whatever happens below)
    BK_HIP(hipSetDevice(e->device));
    std::unique_ptr<Cohort> c(new Cohort());
    c->n = n_samples; c->positions = positions; c->W = (positions + 63) / 64;
    c->n_stride = (n_samples + 63) / 64 * 64 + 64;
    const size_t words = (size_t)3 * c->W * c->n_stride;
    BK_HIP(c->planes.alloc(words));
    BK_HIP(hipMemsetAsync(c->planes.p, 0, words * sizeof(unsigned long long), e->stream));
    // the letters pass through a device buffer of at most 256 MB, a batch of whole samples at a time
    const uint64_t batch = std::max<uint64_t>(1, std::min<uint64_t>(n_samples, (256ull << 20) / positions));
    DevBuf<uint8_t> d_letters;
    BK_HIP(d_letters.alloc((size_t)(batch * positions)));
    for (uint64_t s0 = 0; s0 < n_samples; s0 += batch) {
        const uint64_t ns = std::min<uint64_t>(batch, n_samples - s0);
        BK_HIP(hipMemcpyAsync(d_letters.p, letters + s0 * positions, (size_t)(ns * positions), hipMemcpyHostToDevice, e->stream));
        const dim3 grid((unsigned)((c->W + 3) / 4), (unsigned)std::min<uint64_t>(ns, 65535));
        hipLaunchKernelGGL(bk::cohort_pack_kernel, grid, dim3(bk::kCohortBlock), 0, e->stream, d_letters.p, s0, ns, positions, c->W, c->n_stride, c->planes.p);
        BK_HIP(hipGetLastError());
    }
    BK_HIP(hipStreamSynchronize(e->stream));   // (the caller's letters and d_letters are free again)
    e->cohort = std::move(c);
    return BK_OK;
}

int bk_cohort_distances(bk_engine* e, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_distances: e is null");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_cohort_distances inside a sample: it comes before bk_sample_begin or after the sample's downloads");
    if (!e->cohort) return fail(BK_ERR_STATE, "bk_cohort_distances comes after bk_cohort_set");
    Cohort& c = *e->cohort;
    if (n_rows == 0) return fail(BK_ERR_INVALID, "bk_cohort_distances: n_rows must be at least 1");
    if (row0 >= c.n || n_rows > c.n - row0)
        return fail(BK_ERR_INVALID, "bk_cohort_distances: row0 = %llu, n_rows = %llu lie beyond the cohort's %llu samples", (unsigned long long)row0, (unsigned long long)n_rows, (unsigned long long)c.n);
    BK_HIP(hipSetDevice(e->device));
    const size_t block = (size_t)n_rows * c.n;
    BK_HIP(grow(c.out, 2 * block, 0, e->stream));
    bk::PairsArgs a{};
    a.planes = c.planes.p; a.n = c.n; a.n_stride = c.n_stride; a.W = c.W; a.row0 = row0; a.n_rows = n_rows;
    a.n_col_tiles = (uint32_t)((c.n + bk::kTile - 1) / bk::kTile);
    const uint64_t n_row_tiles = (n_rows + bk::kTile - 1) / bk::kTile, tiles = n_row_tiles * a.n_col_tiles;
    if (tiles > 0x7fffffffull) return fail(BK_ERR_INVALID, "bk_cohort_distances: n_rows = %llu is too many rows for one block of %llu columns", (unsigned long long)n_rows, (unsigned long long)c.n);
    uint64_t slice_words, chunk = bk::kChunk;
    const char* forced = test_env("BK_COHORT_SLICE_WORDS");   // (testing build: small inputs cross slice and chunk borders)
    if (forced && atoi(forced) >= 1) {
        slice_words = (uint64_t)atoi(forced);
        chunk = std::min<uint64_t>(slice_words, bk::kChunk);
    } else {
        const uint64_t chunks = (c.W + bk::kChunk - 1) / bk::kChunk;
        const uint64_t want = std::min<uint64_t>(chunks, std::max<uint64_t>(1, bk::kTargetGroups / tiles));
        slice_words = (chunks + want - 1) / want * bk::kChunk;
    }
    slice_words = std::max<uint64_t>(slice_words, (c.W + 65534) / 65535);   // (the grid's y)
    a.slice_words = (uint32_t)slice_words; a.chunk = (uint32_t)chunk;
    a.diff = c.out.p; a.compared = c.out.p + block;
    BK_HIP(hipMemsetAsync(c.out.p, 0, 2 * block * sizeof(unsigned int), e->stream));
    const dim3 grid((unsigned)tiles, (unsigned)((c.W + slice_words - 1) / slice_words));
    hipLaunchKernelGGL(bk::cohort_pairs_kernel, grid, dim3(bk::kCohortBlock), 0, e->stream, a);
    BK_HIP(hipGetLastError());
    if (diff) BK_HIP(hipMemcpyAsync(diff, a.diff, block * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    if (compared) BK_HIP(hipMemcpyAsync(compared, a.compared, block * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    return BK_OK;
}
