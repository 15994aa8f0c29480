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
// bk_cohort_mst (`--mst`) finds the cohort's minimum spanning forest by Boruvka rounds over the same row blocks (rule: bronko_hip.h,
// DESIGN.md section Y; bronko_amd/host/cohort.cpp and tests/mst_ref.py find the same forest by Prim and by Kruskal):
//   cohort_row_best_kernel   a workgroup of four waves per row of the block the pairs kernel left: lanes stride the columns (coalesced
//                            loads of diff, compared and label), keep the least diff << 32 | j over the admissible columns of another
//                            component and that pair's compared; a wave reduction (__shfl_xor on the key's halves), the four waves
//                            meet in LDS, lane 0 stores.  The loop's bound is n.
//   cohort_comp_diff_kernel, cohort_comp_pair_kernel   a lane per row: atomicMin of the row's diff at its label, then, among the rows
//                            that have that diff, atomicMin of lo << 32 | hi: the component's least edge under (diff, lo, hi).
// bk_cohort_set_minor and bk_cohort_explained (`--contamination`) count, per ordered pair, the positions at which the column's consensus
// base is a minor allele of the row (rule: bronko_hip.h; bronko_amd/host/cohort.cpp and tests/contamination_ref.py
// restate it):
//   cohort_minor_pack_kernel   present masks -> four minor planes per sample, M_X = "X is present, the consensus is a base and not X",
//                              laid out like the letters' planes, [4][W][n_stride].  The wave and lane of cohort_pack_kernel; a lane
//                              takes its bit of the sample's valid, b0 and b1 words, which are there, clears its consensus base from the
//                              mask's low four bits, four ballots, lane 0 stores the four words and adds the popcount of their OR to
//                              the sample's minor_sites (one atomicAdd per word and sample that has any).
//   cohort_explained_kernel    the tile and slice geometry of cohort_pairs_kernel: 64 rows x 64 columns over a slice of words, a lane
//                              holds 4 x 4 pairs interleaved by 16 (16 counters).  The row side stages M_A..M_T as they lie; the column
//                              side stages the one-hot planes C_X = "the consensus is X", made of valid, b0 and b1 while staging:
//                              32 KB of LDS per chunk of 8 words, word-major and read exactly as the pairs kernel reads its image (no
//                              bank conflict).  Per pair and word explained += popcount((M_A & C_A) | (M_C & C_C) | (M_G & C_G) |
//                              (M_T & C_T)): the four terms are disjoint (C is one-hot), M_X & C_X says "the column's base X is present
//                              in the row and the row's consensus is another base" -- both are bases and differ.  Not symmetric, so
//                              the two sides hold different planes; partial sums go to the zeroed block with one atomicAdd per
//                              non-zero pair.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

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

// masks -> the minor planes, and minor_sites (zeroed by the caller)
__global__ __launch_bounds__(kCohortBlock) void cohort_minor_pack_kernel(const uint8_t* __restrict__ masks, uint64_t s0, uint64_t ns, uint64_t positions, uint64_t W,
                                                                         uint64_t n_stride, const unsigned long long* __restrict__ planes,
                                                                         unsigned long long* __restrict__ minor, unsigned int* __restrict__ minor_sites) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * (kCohortBlock / 64) + (threadIdx.x >> 6);   // (wave-uniform)
    const uint64_t pos = w * 64 + lane;
    const bool in = w < W && pos < positions;
    const size_t plane = (size_t)W * n_stride;
    for (uint64_t s = blockIdx.y; s < ns; s += gridDim.y) {
        unsigned m = 0;
        if (in) {
            const size_t at = (size_t)w * n_stride + (size_t)(s0 + s);
            const unsigned long long v = planes[at], b0 = planes[plane + at], b1 = planes[2 * plane + at];   // (one address a wave: a broadcast)
            const unsigned code = (unsigned)((b0 >> lane) & 1ull) | (unsigned)((b1 >> lane) & 1ull) << 1;
            if ((v >> lane) & 1ull) m = (unsigned)masks[s * positions + pos] & 15u & ~(1u << code);
        }
        const unsigned long long ma = __ballot(m & 1u), mc = __ballot(m & 2u), mg = __ballot(m & 4u), mt = __ballot(m & 8u);
        if (lane == 0 && w < W) {
            const size_t at = (size_t)w * n_stride + (size_t)(s0 + s);
            minor[at] = ma; minor[plane + at] = mc; minor[2 * plane + at] = mg; minor[3 * plane + at] = mt;
            const unsigned int sites = (unsigned int)__popcll(ma | mc | mg | mt);
            if (sites) atomicAdd(minor_sites + (s0 + s), sites);
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

struct ExplainedArgs {
    const unsigned long long* planes;       // [3][W][n_stride] the columns' letters
    const unsigned long long* minor;        // [4][W][n_stride] the rows' minor planes
    uint64_t n, n_stride, W;
    uint64_t row0, n_rows;
    uint32_t n_col_tiles;
    uint32_t slice_words, chunk;            // as PairsArgs
    unsigned int* explained;                // [n_rows][n]
};

__global__ __launch_bounds__(kCohortBlock) void cohort_explained_kernel(ExplainedArgs a) {
    __shared__ unsigned long long lds[4 * kChunk * 2 * kTile];   // [A C G T][word of the chunk][rows 0..63: M_X | columns 0..63: C_X]
    const uint32_t t = threadIdx.x, tx = t & 15u, ty = t >> 4;
    const uint32_t ct = blockIdx.x % a.n_col_tiles, rt = blockIdx.x / a.n_col_tiles;
    const uint64_t row_base = a.row0 + (uint64_t)rt * kTile, col_base = (uint64_t)ct * kTile;   // (both + 63 < n_stride)
    const uint64_t w_lo = (uint64_t)blockIdx.y * a.slice_words, w_hi = std::min<uint64_t>(a.W, w_lo + a.slice_words);
    const size_t plane = (size_t)a.W * a.n_stride;

    unsigned int ex[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) ex[i][j] = 0;

    for (uint64_t w0 = w_lo; w0 < w_hi; w0 += a.chunk) {
        const uint32_t L = (uint32_t)std::min<uint64_t>(a.chunk, w_hi - w0);
        __syncthreads();   // (the previous step's reads are done)
        for (uint32_t idx = t; idx < L * 2 * kTile; idx += kCohortBlock) {   // (side is wave-uniform: 64 consecutive idx share it)
            const uint32_t s = idx & 63u, side = (idx >> 6) & 1u, w = idx >> 7;
            unsigned long long x[4];
            if (side) {
                const size_t at = (size_t)(w0 + w) * a.n_stride + col_base + s;
                const unsigned long long v = a.planes[at], b0 = a.planes[plane + at], b1 = a.planes[2 * plane + at];
                x[0] = v & ~b0 & ~b1; x[1] = v & b0 & ~b1; x[2] = v & ~b0 & b1; x[3] = v & b0 & b1;
            } else {
                const size_t at = (size_t)(w0 + w) * a.n_stride + row_base + s;
#pragma unroll
                for (int p = 0; p < 4; p++) x[p] = a.minor[p * plane + at];
            }
#pragma unroll
            for (int p = 0; p < 4; p++) lds[p * kChunk * 2 * kTile + idx] = x[p];
        }
        __syncthreads();
        for (uint32_t w = 0; w < L; w++) {
            const unsigned long long* q = lds + w * 2 * kTile;
            unsigned long long r[4][4], c[4][4];   // [A C G T][i or j]
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    r[p][i] = q[p * kChunk * 2 * kTile + ty + 16 * i];
                    c[p][i] = q[p * kChunk * 2 * kTile + kTile + tx + 16 * i];
                }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    ex[i][j] += (unsigned int)__popcll((r[0][i] & c[0][j]) | (r[1][i] & c[1][j]) | (r[2][i] & c[2][j]) | (r[3][i] & c[3][j]));
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
            if (ex[i][j]) atomicAdd(a.explained + (size_t)(row - a.row0) * a.n + col, ex[i][j]);
        }
    }
}

// ---- bk_cohort_mst ------------------------------------------------------------------------------------------------------------------
constexpr unsigned long long kNoKey = ~0ull;

struct RowBestArgs {
    const unsigned int* diff;               // [n_rows][n] the block cohort_pairs_kernel left
    const unsigned int* compared;           // [n_rows][n]
    const unsigned int* label;              // [n]
    uint64_t n, row0, n_rows;
    uint32_t need;                          // compared a pair must reach: max(1, min_compared)
    unsigned long long* row_key;            // [n]
    unsigned int* row_cmp;                  // [n]
};

// the lesser key of two lanes, 32 bits at a time, and the compared that goes with it
__device__ __forceinline__ void wave_min_key(unsigned long long& key, unsigned int& cmp) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)key, m, 64), hi = (unsigned int)__shfl_xor((int)(unsigned int)(key >> 32), m, 64);
        const unsigned int oc = (unsigned int)__shfl_xor((int)cmp, m, 64);
        const unsigned long long other = (unsigned long long)hi << 32 | lo;
        if (other < key) { key = other; cmp = oc; }   // (keys of different lanes differ in j, or both are kNoKey)
    }
}

__global__ __launch_bounds__(kCohortBlock) void cohort_row_best_kernel(RowBestArgs a) {
    __shared__ unsigned long long s_key[kCohortBlock / 64];
    __shared__ unsigned int s_cmp[kCohortBlock / 64];
    const uint64_t r = blockIdx.x;                                // (the grid is n_rows workgroups: r < n_rows)
    const uint64_t i = a.row0 + r;
    const unsigned int mine = a.label[i];
    const unsigned int* __restrict__ drow = a.diff + (size_t)r * a.n;
    const unsigned int* __restrict__ crow = a.compared + (size_t)r * a.n;
    unsigned long long key = kNoKey;
    unsigned int cmp = 0;
    for (uint64_t j = threadIdx.x; j < a.n; j += kCohortBlock) {   // (ascending j: the first of equal diffs stays)
        const unsigned int c = crow[j], d = drow[j], l = a.label[j];
        const unsigned long long k = (unsigned long long)d << 32 | (unsigned long long)j;
        if (l != mine && c >= a.need && k < key) { key = k; cmp = c; }
    }
    wave_min_key(key, cmp);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { s_key[wave] = key; s_cmp[wave] = cmp; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kCohortBlock / 64; w++)
            if (s_key[w] < key) { key = s_key[w]; cmp = s_cmp[w]; }
        a.row_key[i] = key; a.row_cmp[i] = cmp;
    }
}

// every component's least edge under (diff, lo, hi) from its rows' bests, in two passes over the n rows: the least diff, then the
// least lo << 32 | hi among the rows that have it
__global__ __launch_bounds__(kCohortBlock) void cohort_comp_diff_kernel(const unsigned long long* __restrict__ row_key, const unsigned int* __restrict__ label, uint64_t n,
                                                                        unsigned int* __restrict__ comp_diff) {
    const uint64_t i = (uint64_t)blockIdx.x * kCohortBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = row_key[i];
    if (key != kNoKey) atomicMin(comp_diff + label[i], (unsigned int)(key >> 32));
}

__global__ __launch_bounds__(kCohortBlock) void cohort_comp_pair_kernel(const unsigned long long* __restrict__ row_key, const unsigned int* __restrict__ label, uint64_t n,
                                                                        const unsigned int* __restrict__ comp_diff, unsigned long long* __restrict__ comp_pair) {
    const uint64_t i = (uint64_t)blockIdx.x * kCohortBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = row_key[i];
    if (key == kNoKey) return;
    const unsigned int l = label[i];
    if ((unsigned int)(key >> 32) != comp_diff[l]) return;
    const unsigned long long j = key & 0xffffffffull;
    atomicMin(comp_pair + l, i < j ? (unsigned long long)i << 32 | j : j << 32 | (unsigned long long)i);
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

static int launch_pairs(bk_engine* e, Cohort& c, const char* who, uint64_t row0, uint64_t n_rows);

int bk_cohort_distances(bk_engine* e, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_distances: e is null");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_cohort_distances inside a sample: it comes before bk_sample_begin or after the sample's downloads");
    if (!e->cohort) return fail(BK_ERR_STATE, "bk_cohort_distances comes after bk_cohort_set");
    Cohort& c = *e->cohort;
    if (n_rows == 0) return fail(BK_ERR_INVALID, "bk_cohort_distances: n_rows must be at least 1");
    if (row0 >= c.n || n_rows > c.n - row0)
        return fail(BK_ERR_INVALID, "bk_cohort_distances: row0 = %llu, n_rows = %llu lie beyond the cohort's %llu samples", (unsigned long long)row0, (unsigned long long)n_rows, (unsigned long long)c.n);
    BK_HIP(hipSetDevice(e->device));
    if (int rc = launch_pairs(e, c, "bk_cohort_distances", row0, n_rows)) return rc;
    const size_t block = (size_t)n_rows * c.n;
    if (diff) BK_HIP(hipMemcpyAsync(diff, c.out.p, block * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    if (compared) BK_HIP(hipMemcpyAsync(compared, c.out.p + block, block * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    return BK_OK;
}

// The words of a slice and the words staged per step for a launch of `tiles` tiles (the pairs kernel's and the explained kernel's):
// slices are cut until tiles x slices reaches kTargetGroups
static void cut_slices(const Cohort& c, uint64_t tiles, uint64_t& slice_words, uint64_t& chunk) {
    chunk = bk::kChunk;
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
}

// diff and compared of the rows [row0, row0 + n_rows) against all columns into c.out, [2][n_rows][n], on the engine's stream: the
// zeroing and cohort_pairs_kernel.  The rows lie inside the cohort (the callers' check).
static int launch_pairs(bk_engine* e, Cohort& c, const char* who, uint64_t row0, uint64_t n_rows) {
    const size_t block = (size_t)n_rows * c.n;
    BK_HIP(grow(c.out, 2 * block, 0, e->stream));
    bk::PairsArgs a{};
    a.planes = c.planes.p; a.n = c.n; a.n_stride = c.n_stride; a.W = c.W; a.row0 = row0; a.n_rows = n_rows;
    a.n_col_tiles = (uint32_t)((c.n + bk::kTile - 1) / bk::kTile);
    const uint64_t n_row_tiles = (n_rows + bk::kTile - 1) / bk::kTile, tiles = n_row_tiles * a.n_col_tiles;
    if (tiles > 0x7fffffffull) return fail(BK_ERR_INVALID, "%s: n_rows = %llu is too many rows for one block of %llu columns", who, (unsigned long long)n_rows, (unsigned long long)c.n);
    uint64_t slice_words, chunk;
    cut_slices(c, tiles, slice_words, chunk);
    a.slice_words = (uint32_t)slice_words; a.chunk = (uint32_t)chunk;
    a.diff = c.out.p; a.compared = c.out.p + block;
    BK_HIP(hipMemsetAsync(c.out.p, 0, 2 * block * sizeof(unsigned int), e->stream));
    const dim3 grid((unsigned)tiles, (unsigned)((c.W + slice_words - 1) / slice_words));
    hipLaunchKernelGGL(bk::cohort_pairs_kernel, grid, dim3(bk::kCohortBlock), 0, e->stream, a);
    BK_HIP(hipGetLastError());
    return BK_OK;
}

// Boruvka by row blocks (the rule: include/bronko_hip.h).  Per round: for every block of rows the pairs kernel and the row-best kernel
// over the block where it lies, then every component's least edge from the rows' bests (two launches over the n rows); the O(n)
// component bests come down, the host merges them (a union-find whose root is the component's first sample) and the new labels go up.
// Launch order on the engine's stream and the one synchronise per round carry every dependence.
int bk_cohort_mst(bk_engine* e, uint32_t min_compared, bk_mst_edge* edges, uint64_t cap_edges, uint64_t* n_edges, bk_mst_nearest* nearest, uint32_t* rounds) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_mst: e is null");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_cohort_mst inside a sample: it comes before bk_sample_begin or after the sample's downloads");
    if (!e->cohort) return fail(BK_ERR_STATE, "bk_cohort_mst comes after bk_cohort_set");
    Cohort& c = *e->cohort;
    const uint64_t n = c.n;
    if (!edges) return fail(BK_ERR_INVALID, "bk_cohort_mst: edges is null");
    if (!n_edges) return fail(BK_ERR_INVALID, "bk_cohort_mst: n_edges is null");
    if (cap_edges < n - 1) return fail(BK_ERR_INVALID, "bk_cohort_mst: cap_edges = %llu is less than the %llu edges a cohort of %llu samples may have", (unsigned long long)cap_edges, (unsigned long long)(n - 1), (unsigned long long)n);
    *n_edges = 0;
    if (rounds) *rounds = 0;
    if (nearest)
        for (uint64_t i = 0; i < n; i++) nearest[i] = bk_mst_nearest{0xffffffffu, 0, 0};
    if (n == 1) return BK_OK;
    BK_HIP(hipSetDevice(e->device));
    if (c.mst_label.n < n) {
        BK_HIP(c.mst_label.alloc((size_t)n)); BK_HIP(c.mst_row_key.alloc((size_t)n)); BK_HIP(c.mst_row_cmp.alloc((size_t)n));
        BK_HIP(c.mst_comp_diff.alloc((size_t)n)); BK_HIP(c.mst_comp_pair.alloc((size_t)n));
    }
    // a block's two u32 arrays together stay under 256 MB, as the blocks of `bronko call --distances` do
    uint64_t block_rows = std::max<uint64_t>(1, std::min<uint64_t>(n, (256ull << 20) / (8 * n)));
    const char* forced = test_env("BK_COHORT_MST_BLOCK_ROWS");   // (testing build: small cohorts cross block borders)
    if (forced && atoi(forced) >= 1) block_rows = std::min<uint64_t>(n, (uint64_t)atoi(forced));
    uint32_t max_passes = 1;                                     // ceil(log2 n) + 1
    while ((1ull << (max_passes - 1)) < n) max_passes++;

    std::vector<uint32_t> parent((size_t)n), label((size_t)n), comp_diff((size_t)n), row_cmp((size_t)n);
    std::vector<unsigned long long> comp_pair((size_t)n), row_key;
    for (uint64_t i = 0; i < n; i++) parent[i] = (uint32_t)i;
    auto find = [&parent](uint32_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    const unsigned n_groups = (unsigned)((n + bk::kCohortBlock - 1) / bk::kCohortBlock);
    uint64_t n_found = 0, components = n;
    uint32_t n_rounds = 0;
    bool done = false;
    for (uint32_t pass = 0; pass < max_passes && !done; pass++) {
        for (uint64_t i = 0; i < n; i++) label[i] = find((uint32_t)i);
        BK_HIP(hipMemcpyAsync(c.mst_label.p, label.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        BK_HIP(hipMemsetAsync(c.mst_comp_diff.p, 0xff, (size_t)n * sizeof(unsigned int), e->stream));
        BK_HIP(hipMemsetAsync(c.mst_comp_pair.p, 0xff, (size_t)n * sizeof(unsigned long long), e->stream));
        for (uint64_t row0 = 0; row0 < n; row0 += block_rows) {
            const uint64_t rows = std::min(block_rows, n - row0);
            if (int rc = launch_pairs(e, c, "bk_cohort_mst", row0, rows)) return rc;
            bk::RowBestArgs a{};
            a.diff = c.out.p; a.compared = c.out.p + (size_t)rows * n; a.label = c.mst_label.p;
            a.n = n; a.row0 = row0; a.n_rows = rows; a.need = std::max<uint32_t>(1, min_compared);
            a.row_key = c.mst_row_key.p; a.row_cmp = c.mst_row_cmp.p;
            hipLaunchKernelGGL(bk::cohort_row_best_kernel, dim3((unsigned)rows), dim3(bk::kCohortBlock), 0, e->stream, a);
            BK_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(bk::cohort_comp_diff_kernel, dim3(n_groups), dim3(bk::kCohortBlock), 0, e->stream, c.mst_row_key.p, c.mst_label.p, n, c.mst_comp_diff.p);
        BK_HIP(hipGetLastError());
        hipLaunchKernelGGL(bk::cohort_comp_pair_kernel, dim3(n_groups), dim3(bk::kCohortBlock), 0, e->stream, c.mst_row_key.p, c.mst_label.p, n, c.mst_comp_diff.p, c.mst_comp_pair.p);
        BK_HIP(hipGetLastError());
        BK_HIP(hipMemcpyAsync(comp_diff.data(), c.mst_comp_diff.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        BK_HIP(hipMemcpyAsync(comp_pair.data(), c.mst_comp_pair.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        BK_HIP(hipMemcpyAsync(row_cmp.data(), c.mst_row_cmp.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
        if (pass == 0 && nearest) {                              // (with label[i] = i a row's best is its nearest)
            row_key.resize((size_t)n);
            BK_HIP(hipMemcpyAsync(row_key.data(), c.mst_row_key.p, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        }
        BK_HIP(hipStreamSynchronize(e->stream));
        if (pass == 0 && nearest)
            for (uint64_t i = 0; i < n; i++)
                if (row_key[i] != ~0ull) nearest[i] = bk_mst_nearest{(uint32_t)(row_key[i] & 0xffffffffull), (uint32_t)(row_key[i] >> 32), row_cmp[i]};
        uint64_t added = 0;
        for (uint64_t l = 0; l < n; l++) {                       // (label: the components' bests, of this round's labels)
            if (label[l] != l || comp_pair[l] == ~0ull) continue;
            const uint32_t lo = (uint32_t)(comp_pair[l] >> 32), hi = (uint32_t)(comp_pair[l] & 0xffffffffull);
            if (lo >= hi || hi >= n || (label[lo] == l) == (label[hi] == l)) return fail(BK_ERR_INTERNAL, "bk_cohort_mst: a component's best edge does not leave it");
            const uint32_t ra = find(lo), rb = find(hi);
            if (ra == rb) continue;                              // (the edge was picked from both sides: it counts once)
            if (n_found >= n - 1) return fail(BK_ERR_INTERNAL, "bk_cohort_mst: more than n - 1 edges");
            parent[std::max(ra, rb)] = std::min(ra, rb);
            edges[n_found++] = bk_mst_edge{lo, hi, comp_diff[l], row_cmp[label[lo] == l ? lo : hi]};
            added++;
        }
        components -= added;
        if (added) n_rounds++;
        done = added == 0 || components == 1;
    }
    if (!done) return fail(BK_ERR_INTERNAL, "bk_cohort_mst: no end after ceil(log2 n) + 1 = %u rounds", max_passes);
    std::sort(edges, edges + n_found, [](const bk_mst_edge& x, const bk_mst_edge& y) {
        return x.diff != y.diff ? x.diff < y.diff : x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi;
    });
    *n_edges = n_found;
    if (rounds) *rounds = n_rounds;
    return BK_OK;
}

// ---- bk_cohort_set_minor, bk_cohort_explained -------------------------------------------------------------------------------------
int bk_cohort_set_minor(bk_engine* e, const uint8_t* masks, uint64_t n_samples, uint64_t positions) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_set_minor: e is null");
    if (!masks) return fail(BK_ERR_INVALID, "bk_cohort_set_minor: masks is null");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_cohort_set_minor inside a sample: it comes before bk_sample_begin or after the sample's downloads");
    if (!e->cohort) return fail(BK_ERR_STATE, "bk_cohort_set_minor comes after bk_cohort_set");
    Cohort& c = *e->cohort;
    if (n_samples != c.n) return fail(BK_ERR_INVALID, "bk_cohort_set_minor: n_samples = %llu, the cohort has %llu", (unsigned long long)n_samples, (unsigned long long)c.n);
    if (positions != c.positions) return fail(BK_ERR_INVALID, "bk_cohort_set_minor: positions = %llu, the cohort has %llu", (unsigned long long)positions, (unsigned long long)c.positions);
    BK_HIP(hipSetDevice(e->device));
    const size_t words = (size_t)4 * c.W * c.n_stride;
    DevBuf<unsigned long long> minor;       // (the cohort's own only once they are whole)
    DevBuf<unsigned int> sites;
    BK_HIP(minor.alloc(words));
    BK_HIP(sites.alloc((size_t)c.n));
    BK_HIP(hipMemsetAsync(minor.p, 0, words * sizeof(unsigned long long), e->stream));
    BK_HIP(hipMemsetAsync(sites.p, 0, (size_t)c.n * sizeof(unsigned int), e->stream));
    // the masks pass through a device buffer of at most 256 MB, a batch of whole samples at a time, as bk_cohort_set's letters do
    const uint64_t batch = std::max<uint64_t>(1, std::min<uint64_t>(c.n, (256ull << 20) / positions));
    DevBuf<uint8_t> d_masks;
    BK_HIP(d_masks.alloc((size_t)(batch * positions)));
    for (uint64_t s0 = 0; s0 < c.n; s0 += batch) {
        const uint64_t ns = std::min<uint64_t>(batch, c.n - s0);
        BK_HIP(hipMemcpyAsync(d_masks.p, masks + s0 * positions, (size_t)(ns * positions), hipMemcpyHostToDevice, e->stream));
        const dim3 grid((unsigned)((c.W + 3) / 4), (unsigned)std::min<uint64_t>(ns, 65535));
        hipLaunchKernelGGL(bk::cohort_minor_pack_kernel, grid, dim3(bk::kCohortBlock), 0, e->stream, d_masks.p, s0, ns, positions, c.W, c.n_stride, c.planes.p, minor.p, sites.p);
        BK_HIP(hipGetLastError());
    }
    BK_HIP(hipStreamSynchronize(e->stream));   // (the caller's masks and d_masks are free again)
    std::swap(c.minor.p, minor.p); std::swap(c.minor.n, minor.n);   // (planes of an earlier call go with the locals)
    std::swap(c.minor_sites.p, sites.p); std::swap(c.minor_sites.n, sites.n);
    return BK_OK;
}

int bk_cohort_explained(bk_engine* e, uint64_t row0, uint64_t n_rows, uint32_t* explained, uint32_t* minor_sites) {
    if (!e) return fail(BK_ERR_INVALID, "bk_cohort_explained: e is null");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_cohort_explained inside a sample: it comes before bk_sample_begin or after the sample's downloads");
    if (!e->cohort) return fail(BK_ERR_STATE, "bk_cohort_explained comes after bk_cohort_set and bk_cohort_set_minor");
    Cohort& c = *e->cohort;
    if (!c.minor.p) return fail(BK_ERR_STATE, "bk_cohort_explained comes after bk_cohort_set_minor");
    if (n_rows == 0) return fail(BK_ERR_INVALID, "bk_cohort_explained: n_rows must be at least 1");
    if (row0 >= c.n || n_rows > c.n - row0)
        return fail(BK_ERR_INVALID, "bk_cohort_explained: row0 = %llu, n_rows = %llu lie beyond the cohort's %llu samples", (unsigned long long)row0, (unsigned long long)n_rows, (unsigned long long)c.n);
    BK_HIP(hipSetDevice(e->device));
    if (explained) {
        const size_t block = (size_t)n_rows * c.n;
        BK_HIP(grow(c.ex_out, block, 0, e->stream));
        bk::ExplainedArgs a{};
        a.planes = c.planes.p; a.minor = c.minor.p; a.n = c.n; a.n_stride = c.n_stride; a.W = c.W; a.row0 = row0; a.n_rows = n_rows;
        a.n_col_tiles = (uint32_t)((c.n + bk::kTile - 1) / bk::kTile);
        const uint64_t n_row_tiles = (n_rows + bk::kTile - 1) / bk::kTile, tiles = n_row_tiles * a.n_col_tiles;
        if (tiles > 0x7fffffffull) return fail(BK_ERR_INVALID, "bk_cohort_explained: n_rows = %llu is too many rows for one block of %llu columns", (unsigned long long)n_rows, (unsigned long long)c.n);
        uint64_t slice_words, chunk;
        cut_slices(c, tiles, slice_words, chunk);
        a.slice_words = (uint32_t)slice_words; a.chunk = (uint32_t)chunk;
        a.explained = c.ex_out.p;
        BK_HIP(hipMemsetAsync(c.ex_out.p, 0, block * sizeof(unsigned int), e->stream));
        const dim3 grid((unsigned)tiles, (unsigned)((c.W + slice_words - 1) / slice_words));
        hipLaunchKernelGGL(bk::cohort_explained_kernel, grid, dim3(bk::kCohortBlock), 0, e->stream, a);
        BK_HIP(hipGetLastError());
        BK_HIP(hipMemcpyAsync(explained, c.ex_out.p, block * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    }
    if (minor_sites) BK_HIP(hipMemcpyAsync(minor_sites, c.minor_sites.p + row0, (size_t)n_rows * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    return BK_OK;
}
