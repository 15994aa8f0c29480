// bk_codons.hip -- how many placed records carry each of the 64 triplets at every codon of the caller's coding regions
// (bk_sample_codons; `bronko call --codons`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section T; bronko_amd/host/codons.cpp and tests/codons_ref.py restate it.
// The rows are bk_link_enable's (bk_linkage.hip): this file only reads the store.
//   codon_count_kernel   a lane per row (two 16-byte loads, unpacked by bk_link_row.h).  A row covers some fifty codons of every
//                        region it overlaps and differs from the reference in at most eight cells, so it does not touch fifty
//                        counters: per region it adds +1 / -1 to a cover difference array (at its first wholly covered codon and one
//                        behind its last), and only for a codon that holds one of its mismatches it forms its triplet and adds 1 to
//                        count[codon][triplet] -- once per codon, at the codon's first mismatch.  The regions a row overlaps: a
//                        binary search over the regions sorted by first cell for the last one that starts before the row's end,
//                        then a walk back while the running maximum of the regions' ends lies behind the row's first cell.  A
//                        difference array of at most kCodonLdsCodons entries is privatised in LDS (zeroed, LDS atomics, one global
//                        add per non-zero entry behind a barrier): amplicon reads share their first cell by the thousand.  A larger
//                        one, and the sparse triplet counters, take global atomics.
//   codon_finish_kernel  a workgroup per 256 codons.  Its carry is the sum of the difference array in front of its tile, which it
//                        reads again itself (at most 1 MiB, from L2) -- no workgroup waits for another; a scan of the tile gives
//                        cover[codon]; then sixteen lanes per codon sum its 64 counters (one 16-byte load each) and the first of
//                        them stores count[codon][reference triplet] = cover - sum.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kCodonBlock = 256;

template <bool kLds>
__device__ __forceinline__ void codon_count_rows(const CodonArgs& a, unsigned int* __restrict__ diff) {
    const uint64_t n_rows = a.store.rows_in_store();
    for (uint64_t r = (uint64_t)blockIdx.x * kCodonBlock + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * kCodonBlock) {
        const RowRegs row = a.store.load(r);
        const uint32_t cell0 = row.cell0, end = row.end, n_mm = row.n_mm;
        const uint32_t (&e)[8] = row.e;
        const uint32_t s0 = first_not_below(0u, a.n_regions, end, [&](uint32_t i) { return a.sorted[i].x; });   // the regions that start before the row's end
        for (uint32_t i = s0; i-- > 0u;) {
            const uint4 reg = a.sorted[i];
            if (reg.w <= cell0) break;                 // (no region up to here reaches the row)
            const uint32_t c0 = reg.x, nc = reg.y, base = reg.z;
            if (c0 + 3u * nc <= cell0) continue;
            const uint32_t f = cell0 <= c0 ? 0u : (cell0 - c0 + 2u) / 3u;   // the codons [f, l) lie wholly under the row
            const uint32_t l = min(nc, (end - c0) / 3u);
            if (f >= l || (uint64_t)base + l > a.n_codons) continue;       // (the host numbered every codon below n_codons)
            if (kLds) { atomicAdd(diff + base + f, 1u); atomicAdd(diff + base + l, 0xffffffffu); }
            else { atomicAdd(a.cover_diff + base + f, 1u); atomicAdd(a.cover_diff + base + l, 0xffffffffu); }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if ((uint32_t)s >= n_mm) continue;
                const uint32_t cell = cell0 + (e[s] & 0xffffu);
                if (cell < c0) continue;
                const uint32_t j = (cell - c0) / 3u;
                if (j < f || j >= l) continue;
                const uint32_t first = c0 + 3u * j;
                if (s > 0 && cell0 + (e[s > 0 ? s - 1 : 0] & 0xffffu) >= first) continue;   // (the codon's first mismatch adds for all of them)
                uint32_t trip = 0;
#pragma unroll
                for (uint32_t t = 0; t < 3u; ++t) trip = trip * 4u + row_base(row, first + t - cell0, sym_at(a.ref_words, first + t));
                atomicAdd(a.counts + (uint64_t)(base + j) * 64u + trip, 1u);
            }
        }
    }
}

__global__ __launch_bounds__(kCodonBlock) void codon_count_lds_kernel(CodonArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned int diff_s[];
    const uint32_t n = a.n_codons + 1u;               // at most kCodonLdsCodons
    lds_table_zero<kCodonBlock>(diff_s, n);
    codon_count_rows<true>(a, diff_s);
    lds_table_add_to<kCodonBlock>(diff_s, n, a.cover_diff);
}

__global__ __launch_bounds__(kCodonBlock) void codon_count_kernel(CodonArgs a) { codon_count_rows<false>(a, nullptr); }

__global__ __launch_bounds__(kCodonBlock) void codon_finish_kernel(CodonArgs a) {
    __shared__ unsigned int wave_s[8];
    __shared__ unsigned int cover_s[kCodonBlock];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tile0 = blockIdx.x * kCodonBlock;
    uint32_t part = 0;                                 // the carry: everything in front of the tile
    for (uint32_t i = tid; i < tile0; i += kCodonBlock) part += a.cover_diff[i];
    part = wave_total(part);
    const uint32_t c = tile0 + tid;
    const uint32_t incl = wave_incl_add(c < a.n_codons ? a.cover_diff[c] : 0u);
    if (lane == 0) wave_s[wave] = part;
    if (lane == 63) wave_s[4 + wave] = incl;
    __syncthreads();
    uint32_t cover = wave_s[0] + wave_s[1] + wave_s[2] + wave_s[3] + incl;
    for (uint32_t w = 0; w < wave; ++w) cover += wave_s[4 + w];
    cover_s[tid] = cover;
    __syncthreads();
    const uint32_t q = tid & 15u;                      // sixteen lanes a codon: its 64 counters are sixteen 16-byte loads
    for (uint32_t j = tid >> 4; j < (uint32_t)kCodonBlock; j += kCodonBlock / 16) {
        const uint32_t cd = tile0 + j;
        if (cd >= a.n_codons) break;
        const uint4 v = reinterpret_cast<const uint4*>(a.counts + (uint64_t)cd * 64u)[q];
        uint32_t sum = v.x + v.y + v.z + v.w;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) sum += (uint32_t)__shfl_xor((int)sum, off);
        if (q != 0) continue;
        uint32_t r0 = 0, r1 = a.n_regions;             // the codon's region: the last whose first codon is not behind it
        while (r0 + 1u < r1) {
            const uint32_t mid = (r0 + r1) >> 1;
            if (a.regions[mid].y <= cd) r0 = mid; else r1 = mid;
        }
        const uint2 reg = a.regions[r0];
        const uint32_t cell = reg.x + 3u * (cd - reg.y);
        if (cell + 2u >= a.total_cells) continue;   // (the host refused a region beyond the cells)
        const uint32_t trip = sym_at(a.ref_words, cell) * 16u + sym_at(a.ref_words, cell + 1u) * 4u + sym_at(a.ref_words, cell + 2u);
        a.counts[(uint64_t)cd * 64u + trip] = cover_s[j] - sum;
    }
}

}  // namespace

void launch_codon_count(const CodonArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream) {
    if (a.n_codons == 0 || rows_upper == 0) return;
    if (a.n_codons + 1u <= kCodonLdsCodons) {         // (up to 64 KiB of LDS a workgroup: two fit a CU)
        hipLaunchKernelGGL(codon_count_lds_kernel, dim3(row_grid(rows_upper, kCodonBlock, n_cus, 2)), dim3(kCodonBlock), (size_t)(a.n_codons + 1u) * sizeof(unsigned int), stream, a);
    } else {
        hipLaunchKernelGGL(codon_count_kernel, dim3(row_grid(rows_upper, kCodonBlock, n_cus, 8)), dim3(kCodonBlock), 0, stream, a);
    }
}

void launch_codon_finish(const CodonArgs& a, hipStream_t stream) {
    if (a.n_codons == 0) return;
    hipLaunchKernelGGL(codon_finish_kernel, dim3((a.n_codons + kCodonBlock - 1) / kCodonBlock), dim3(kCodonBlock), 0, stream, a);
}

}  // namespace bk
