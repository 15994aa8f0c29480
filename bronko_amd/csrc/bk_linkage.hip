// bk_linkage.hip -- which substitutions the same records carry (bk_link_enable; `bronko call --linkage`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section L; bronko_amd/host/linkage.cpp and tests/linkage_ref.py restate it.
//   link_scan_kernel    behind the scan of the same records, a lane per record.  The anchors and the placement checks are
//                       indel_scan_kernel's (bk_anchor.h, over LinkArgs::ix); a record is placed only on one diagonal (delta = 0 exactly).  The
//                       sixteen-base XOR / fold / popcount pass keeps what indel_scan_kernel's delta = 0 branch throws away: the
//                       set bits of the folded word are the mismatches' positions (ctz).  A record against the reference is
//                       compared with rc_words at the mirrored cell; its position i is cell dL + n - 1 - i and its base there
//                       the complement -- nothing is reverse-complemented in memory.  A placed record leaves one row of 32 bytes
//                       (bk_link_row, packed by bk_link_row.h) in the sample's row store: one returning add per wave (ballot +
//                       mbcnt), two 16-byte stores per row.  The sample's tallies: one add per wave and tally.
//   link_count_kernel   at the sample's end, given the sites: a lane per row (bk_link_row.h) binary-searches the first site
//                       at or behind the row's first cell, walks the sites the row covers and adds 1 to count[bA][bB] of every
//                       pair of them within max_dist.  A counter table of at most kLinkLdsPairs pairs is privatised in LDS
//                       (zeroed, LDS atomics, one global add per non-zero counter behind a barrier); a larger one takes global
//                       atomics.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kLinkBlock = 256;

struct LinkTally { uint32_t records = 0, unplaced = 0, discordant = 0; };

// A record's row, or false with the tally that says why not.  lo / hi: the row's two halves.
__device__ __forceinline__ bool link_place(const LinkArgs& a, uint32_t r, LinkTally& t, uint4& lo, uint4& hi) {
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    if (n < k) return false;                          // (trimmed away: no record any more)
    t.records++;
    if (n < 2 * k) { t.unplaced++; return false; }
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    Anchors an;
    if (!anchors_of(a.ix, w, n, an)) { t.unplaced++; return false; }
    const int32_t dL = (int32_t)an.ca - an.pa, dR = (int32_t)an.cb - an.pb;
    if (dL != dR || !cells_placed(a.ix, an.ca, an.cb, dL, dL + n)) { t.unplaced++; return false; }
    const bool against = an.against;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const uint32_t* __restrict__ text = against ? a.ix.rc_words : a.ix.ref_words;
    const int64_t diag = against ? (int64_t)a.ix.total_cells - dL - n : (int64_t)dL;
    RowRegs row{};                                    // e: the mismatches, ascending by offset (static indices only)
    uint32_t (&e)[8] = row.e;
    uint32_t m = 0;
    for (uint32_t i = 0; i < (uint32_t)n; i += 16u) {
        uint32_t x = mismatch_bits16(w, last_word, i, (uint32_t)n, text, diag);
        const uint32_t have = m;
        m += (uint32_t)__popc(x);
        if (m > a.max_mismatches) break;              // (no row: the positions are not needed; below, all m <= 8 of them are kept)
        uint32_t slot = have;
        while (x) {
            const uint32_t pos = i + ((uint32_t)__builtin_ctz(x) >> 1);
            x &= x - 1u;
            const uint32_t sym = sym_at(w, pos);
            if (against) {                            // found from the last cell down: each goes in front
                const uint32_t entry = ((uint32_t)n - 1u - pos) | ((3u - sym) << 16);
#pragma unroll
                for (int s = 7; s > 0; --s) e[s] = e[s - 1];
                e[0] = entry;
            } else {
                const uint32_t entry = pos | (sym << 16);
#pragma unroll
                for (int s = 0; s < 8; ++s) if (slot == (uint32_t)s) e[s] = entry;
            }
            ++slot;
        }
    }
    if (m > a.max_mismatches) { t.discordant++; return false; }
    row.cell0 = (uint32_t)dL; row.end = (uint32_t)(dL + n); row.strand = against ? 1u : 0u; row.n_mm = m;
    row_pack(row, lo, hi);
    return true;
}

__global__ __launch_bounds__(kLinkBlock) void link_scan_kernel(LinkArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n = a.rec.n_records_dev ? std::min<uint64_t>(a.rec.n_records, *a.rec.n_records_dev) : a.rec.n_records;
    const uint64_t stride = (uint64_t)gridDim.x * kLinkBlock;
    LinkTally t;
    for (uint64_t base = (uint64_t)blockIdx.x * kLinkBlock + wave * 64u; base < n; base += stride) {
        const uint64_t r = base + lane;
        uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
        const bool row = r < n && link_place(a, (uint32_t)r, t, lo, hi);
        const unsigned long long mask = __ballot(row);
        if (mask == 0ull) continue;
        const uint32_t cnt = (uint32_t)__popcll(mask);
        unsigned long long at = 0ull;
        if (lane == 0) at = atomicAdd(a.store.placed, (unsigned long long)cnt);
        at = __shfl(at, 0);
        if (row) {
            const uint64_t o = at + lane_prefix(mask);
            if (o < a.store.cap) a.store.store(o, lo, hi);   // (the engine made room for every record of the batch)
        }
    }
    const uint32_t sums[3] = {wave_total(t.records), wave_total(t.unplaced), wave_total(t.discordant)};
    if (lane == 0) {
        if (sums[0]) atomicAdd(a.tallies + 0, (unsigned long long)sums[0]);
        if (sums[1]) atomicAdd(a.tallies + 2, (unsigned long long)sums[1]);
        if (sums[2]) atomicAdd(a.tallies + 3, (unsigned long long)sums[2]);
    }
}

template <bool kLds>
__device__ __forceinline__ void link_count_rows(const LinkArgs& a, unsigned int* __restrict__ table) {
    const uint64_t n_rows = a.store.rows_in_store();
    for (uint64_t r = (uint64_t)blockIdx.x * kLinkBlock + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * kLinkBlock) {
        const RowRegs row = a.store.load(r);
        const uint32_t cell0 = row.cell0, end = row.end;
        const uint32_t s0 = first_not_below(0u, a.n_sites, cell0, [&](uint32_t i) { return a.sites[i]; });   // the first site at or behind cell0
        for (uint32_t i = s0; i < a.n_sites; ++i) {
            const uint32_t ci = a.sites[i];
            if (ci >= end) break;
            uint32_t j = i + 1u;
            if (j >= a.n_sites) break;
            uint32_t cj = a.sites[j];
            if (cj >= end) break;                      // (the row's last site: no pair begins here or behind)
            if (cj - ci > a.max_dist) continue;
            const uint32_t ba = row_base(row, ci - cell0, sym_at(a.ix.ref_words, ci));
            const uint64_t p0 = (uint64_t)a.pair_lo[i];
            for (;;) {
                const uint32_t bb = row_base(row, cj - cell0, sym_at(a.ix.ref_words, cj));
                const uint64_t at = (p0 + (j - i - 1u)) * 16u + ba * 4u + bb;
                if (at < a.n_pairs * 16u) {            // (the host enumerated every pair that a row can cover)
                    if (kLds) atomicAdd(table + (uint32_t)at, 1u);
                    else atomicAdd(a.counts + at, 1u);
                }
                if (++j >= a.n_sites) break;
                cj = a.sites[j];
                if (cj >= end || cj - ci > a.max_dist) break;
            }
        }
    }
}

__global__ __launch_bounds__(kLinkBlock) void link_count_lds_kernel(LinkArgs a) {
    extern __shared__ unsigned int table_s[];
    const uint32_t n_counters = (uint32_t)a.n_pairs * 16u;   // at most kLinkLdsPairs * 16
    lds_table_zero<kLinkBlock>(table_s, n_counters);
    link_count_rows<true>(a, table_s);
    lds_table_add_to<kLinkBlock>(table_s, n_counters, a.counts);
}

__global__ __launch_bounds__(kLinkBlock) void link_count_kernel(LinkArgs a) { link_count_rows<false>(a, nullptr); }

}  // namespace

void launch_link_scan(const LinkArgs& a, int n_cus, hipStream_t stream) {
    if (a.rec.n_records == 0) return;
    hipLaunchKernelGGL(link_scan_kernel, dim3(row_grid(a.rec.n_records, kLinkBlock, n_cus, 8)), dim3(kLinkBlock), 0, stream, a);
}

void launch_link_count(const LinkArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream) {
    if (a.n_pairs == 0 || rows_upper == 0) return;
    const unsigned grid = row_grid(rows_upper, kLinkBlock, n_cus, 8);
    if (a.n_pairs <= kLinkLdsPairs)
        hipLaunchKernelGGL(link_count_lds_kernel, dim3(grid), dim3(kLinkBlock), (size_t)a.n_pairs * 16u * sizeof(unsigned int), stream, a);
    else
        hipLaunchKernelGGL(link_count_kernel, dim3(grid), dim3(kLinkBlock), 0, stream, a);
}

}  // namespace bk
