// bk_read_pileup.hip -- per cell of the genome file, how many placed records lie over it, which base each carries there, on which strand,
// and how many of them have the cell within E positions of one of their ends (bk_sample_read_pileup; `bronko call --read-pileup`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section U; bronko_amd/host/read_pileup.cpp and tests/read_pileup_ref.py
// restate it.  The rows are bk_link_enable's (bk_linkage.hip): this file only reads the store.
//   read_pileup_count_kernel   a lane per row (two 16-byte loads, unpacked by bk_link_row.h).  A row covers some 150 cells and differs
//                              from the reference in at most eight of them, so it does not touch 150 counters: it adds +1 at its first
//                              cell and -1 (0xffffffff: the prefix sum is exact modulo 2^32) behind its last to its strand's cover
//                              difference array, the same for the one or two stretches in which it is near an end to the near-end
//                              difference array, and 1 per substitution to mm[cell][base][strand] and, near an end, to
//                              mm_near[cell][base]: O(1 + n_mm) adds.  Amplicon reads share their first and last cell by the thousand and
//                              a fixed variant puts every row on one mm word, so the lanes of a wave that add to the same word are
//                              merged first: a ballot on the leader's index, one add of the popcount, at most kMergeRounds rounds and
//                              none after a round in which the leader stood alone; what is left takes single adds.  No LDS: the indices
//                              range over fifteen words a cell of a genome of up to 2^22 cells, which no dense table in LDS holds.
//   read_pileup_finish_kernel  one workgroup, as span_prefix_kernel (bk_event_pass.hip): a thread sums its stretch of the three difference arrays,
//                              the stretches' sums are scanned through LDS, the thread walks its stretch again and writes per cell one
//                              bk_read_pileup_cell (three 16-byte stores): a base other than the reference's takes its mm counts, the
//                              reference's base cover - sum mm per strand and near_cover - sum mm_near.  A cell whose reference letter
//                              is not ACGT lies under no row (cells_placed, bk_anchor.h): its cover and its mm words are zero, and so
//                              are its twelve counters.  The workgroup tallies the covered cells and the bases and stores both.
// The eight substitutions stay in registers under static indices.  Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kPileBlock = 256;
constexpr int kPileFinishBlock = 1024;
constexpr int kMergeRounds = 4;

// `val` more at table[idx] for every lane that is `on`.  Called by all lanes of the wave together, with one table.  Lanes with equal idx are merged:
// the first lane that still waits is the leader, the lanes with its idx are counted by a ballot and the leader adds for all of them.
__device__ __forceinline__ void merged_add(unsigned int* __restrict__ table, bool on, uint32_t idx, uint32_t val, uint32_t lane) {
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int round = 0; round < kMergeRounds; ++round) {
        if (todo == 0ull) break;                                  // (wave-uniform)
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)leader);
        const bool mine = on && idx == key;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(table + key, val * (uint32_t)__popcll(same));
        if (mine) on = false;
        todo &= ~same;
        if ((same & (same - 1ull)) == 0ull) break;                // the leader stood alone: the wave's rows are spread out
    }
    if (on) atomicAdd(table + idx, val);
}

__global__ __launch_bounds__(kPileBlock) void read_pileup_count_kernel(ReadPileupArgs a) {
    const uint64_t n_rows = a.store.rows_in_store();
    const uint32_t lane = threadIdx.x & 63u, E = a.end_dist, n1 = a.total_cells + 1u;
    unsigned int* __restrict__ near_diff = a.diff + 2ull * n1;
    // every lane of a wave goes round together (merged_add is the whole wave's): the loop's bound is the wave's first row
    for (uint64_t r0 = (uint64_t)blockIdx.x * kPileBlock + (threadIdx.x & ~63u); r0 < n_rows; r0 += (uint64_t)gridDim.x * kPileBlock) {
        const uint64_t r = r0 + lane;
        RowRegs row{};
        bool live = r < n_rows;
        if (live) row = a.store.load(r);
        const uint32_t c0 = row.cell0, end = row.end, n = end - c0;
        live = live && n != 0u && end >= c0 && end <= a.total_cells;   // (a placed record lies inside the cells)
        const uint32_t cover = (row.strand & 1u) * n1;               // the strand's difference array (the table is the wave's, the index the lane's)
        merged_add(a.diff, live, cover + c0, 1u, lane);
        merged_add(a.diff, live, cover + end, 0xffffffffu, lane);
        const bool whole = n <= 2u * E;                            // near an end at every cell
        const bool near_on = live && E != 0u;
        merged_add(near_diff, near_on, c0, 1u, lane);
        merged_add(near_diff, near_on, whole ? end : c0 + E, 0xffffffffu, lane);
        merged_add(near_diff, near_on && !whole, end - E, 1u, lane);
        merged_add(near_diff, near_on && !whole, end, 0xffffffffu, lane);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (__ballot(live && (uint32_t)s < row.n_mm) == 0ull) break;   // (wave-uniform: the mismatches are packed from slot 0 up)
            const uint32_t off = row.e[s] & 0xffffu, base = (row.e[s] >> 16) & 3u;
            const bool there = live && (uint32_t)s < row.n_mm && off < n;
            const uint32_t cell = there ? c0 + off : 0u;
            merged_add(a.mm, there, cell * 8u + base * 2u + (row.strand & 1u), 1u, lane);
            merged_add(a.mm_near, there && min(off, n - 1u - off) < E, cell * 4u + base, 1u, lane);
        }
    }
}

__global__ __launch_bounds__(kPileFinishBlock) void read_pileup_finish_kernel(ReadPileupArgs a) {
    __shared__ unsigned int part_s[2][3][kPileFinishBlock];
    __shared__ unsigned long long tally_s[2][kPileFinishBlock / 64];
    const uint32_t tid = threadIdx.x, n = a.total_cells, n1 = n + 1u;
    const uint32_t per = (n + kPileFinishBlock - 1) / kPileFinishBlock;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    const unsigned int* __restrict__ d0 = a.diff;
    const unsigned int* __restrict__ d1 = a.diff + n1;
    const unsigned int* __restrict__ d2 = a.diff + 2ull * n1;
    unsigned int sum[3] = {0u, 0u, 0u};
    for (uint32_t i = lo; i < hi; ++i) { sum[0] += d0[i]; sum[1] += d1[i]; sum[2] += d2[i]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) part_s[0][j][tid] = sum[j];
    __syncthreads();
    int cur = 0;
    for (uint32_t off = 1; off < (uint32_t)kPileFinishBlock; off <<= 1) {   // inclusive scan of the stretches' sums
#pragma unroll
        for (int j = 0; j < 3; ++j) part_s[cur ^ 1][j][tid] = part_s[cur][j][tid] + (tid >= off ? part_s[cur][j][tid - off] : 0u);
        __syncthreads();
        cur ^= 1;
    }
    unsigned int acc[3];                                           // what precedes this thread's stretch
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = part_s[cur][j][tid] - sum[j];
    unsigned long long covered = 0ull, bases = 0ull;
    for (uint32_t i = lo; i < hi; ++i) {
        acc[0] += d0[i]; acc[1] += d1[i]; acc[2] += d2[i];
        const uint4 m0 = reinterpret_cast<const uint4*>(a.mm)[2ull * i], m1 = reinterpret_cast<const uint4*>(a.mm)[2ull * i + 1u];
        const uint4 mn = reinterpret_cast<const uint4*>(a.mm_near)[i];
        uint32_t f[4] = {m0.x, m0.z, m1.x, m1.z}, v[4] = {m0.y, m0.w, m1.y, m1.w}, e[4] = {mn.x, mn.y, mn.z, mn.w};
        const uint32_t ref = sym_at(a.ref_words, i);
        const uint32_t rf = acc[0] - (f[0] + f[1] + f[2] + f[3]), rv = acc[1] - (v[0] + v[1] + v[2] + v[3]), re = acc[2] - (e[0] + e[1] + e[2] + e[3]);
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b)
            if (b == ref) { f[b] += rf; v[b] += rv; e[b] += re; }   // (no row carries a substitution to the reference's base: these were zero)
        uint4* __restrict__ out = reinterpret_cast<uint4*>(a.cells + i);
        out[0] = make_uint4(f[0], f[1], f[2], f[3]);
        out[1] = make_uint4(v[0], v[1], v[2], v[3]);
        out[2] = make_uint4(e[0], e[1], e[2], e[3]);
        covered += (acc[0] + acc[1]) != 0u ? 1ull : 0ull;
        bases += (unsigned long long)acc[0] + acc[1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        covered += (unsigned long long)__shfl_xor((long long)covered, off);
        bases += (unsigned long long)__shfl_xor((long long)bases, off);
    }
    if ((tid & 63u) == 0u) { tally_s[0][tid >> 6] = covered; tally_s[1][tid >> 6] = bases; }
    __syncthreads();
    if (tid < 2u) {
        unsigned long long t = 0ull;
        for (int w = 0; w < kPileFinishBlock / 64; ++w) t += tally_s[tid][w];
        a.tallies[tid] = t;
    }
}

}  // namespace

void launch_read_pileup_count(const ReadPileupArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream) {
    if (a.total_cells == 0 || rows_upper == 0) return;
    hipLaunchKernelGGL(read_pileup_count_kernel, dim3(row_grid(rows_upper, kPileBlock, n_cus, 8)), dim3(kPileBlock), 0, stream, a);
}

void launch_read_pileup_finish(const ReadPileupArgs& a, hipStream_t stream) {
    if (a.total_cells == 0) return;
    hipLaunchKernelGGL(read_pileup_finish_kernel, dim3(1), dim3(kPileFinishBlock), 0, stream, a);
}

}  // namespace bk
