// bk_haplotypes.hip -- which combinations of substitutions single placed records carry across each of the caller's regions, and how
// often (bk_sample_haplotypes; `bronko call --haplotypes`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section H; bronko_amd/host/haplotypes.cpp and tests/haplotypes_ref.py restate
// it.  The rows are bk_link_enable's (bk_linkage.hip): this file only reads the store.
//   hap_count_kernel    a lane per row (two 16-byte loads, unpacked by bk_link_row.h).  Two binary searches over the regions
//                       sorted by first cell give those that begin under the row; of them the ones that end at or before the row's
//                       end are spanned.  Nearly every (row, region) is the reference haplotype and amplicon reads share their first
//                       cell by the thousand, so cover and ref_count are privatised in LDS (8 bytes a region, at most 32 KiB;
//                       zeroed, LDS atomics, one global add per non-zero entry behind a barrier).  A non-empty haplotype goes into
//                       an open-addressing table that stores no key: a slot's owner word names the first row that claimed it and
//                       the region it claimed it for, and the list is read back from that row -- the store was written by earlier
//                       launches and is read-only here, so whoever sees an owner word can read its row at once.  One relaxed load,
//                       at most one CAS, then either the slot is the lane's own or the owner's list in the region is compared with
//                       the lane's; equal: one add to the slot's count, else the next slot.  The probe loop is bounded by the
//                       table's size and a lane that finds no slot adds 1 to `dropped`.  No lane waits for another lane's write.
//   hap_finish_kernel   a lane per slot, four groups of 64 slots a wave: an occupied slot appends one bk_hap_entry (ballot + mbcnt, one
//                       returning add per wave for its 256 slots -- the adds all go to one address, and one per 64 slots was what the
//                       kernel's time consisted of), its list rebuilt from the owner's row with offsets from the region's first cell.
// The eight substitutions stay in registers under static indices.  Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kHapBlock = 256;
constexpr int kHapFinishSlots = 4;             // groups of 64 slots a wave of hap_finish_kernel appends with one returning add
constexpr uint32_t kHapNone = 0xffffffffu;   // no entry: its cell lies behind every region

// the row's mismatches as cell | base << 28 (a cell is below 2^27), kHapNone from n_mm on
__device__ __forceinline__ void hap_cells(const RowRegs& row, uint32_t (&q)[8]) {
#pragma unroll
    for (int s = 0; s < 8; ++s) q[s] = (uint32_t)s < row.n_mm ? (row.cell0 + (row.e[s] & 0xffffu)) | (((row.e[s] >> 16) & 3u) << 28) : kHapNone;
}

// the list of a row inside the cells [c0, c1): the entries in front of c0 shifted out (they are ascending, so those inside are one
// run), the ones at or behind c1 blanked; returns how many are left
__device__ __forceinline__ uint32_t hap_list(const uint32_t (&q)[8], uint32_t c0, uint32_t c1, uint32_t (&l)[8]) {
#pragma unroll
    for (int s = 0; s < 8; ++s) l[s] = q[s];
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        if ((l[0] & 0x0fffffffu) < c0) {
#pragma unroll
            for (int s = 0; s < 7; ++s) l[s] = l[s + 1];
            l[7] = kHapNone;
        }
    }
    uint32_t n = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if ((l[s] & 0x0fffffffu) < c1) ++n; else l[s] = kHapNone;
    }
    return n;
}

// one more row with the list `l` in region `region` (the caller's index; cells [c0, c1)): the table
__device__ __forceinline__ void hap_insert(const HapArgs& a, uint64_t row, uint32_t region, uint32_t c0, uint32_t c1, const uint32_t (&l)[8]) {
    const unsigned long long mine = (((unsigned long long)row << 12) | region) + 1ull;
    unsigned long long hw = (unsigned long long)region * 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int s = 0; s < 8; ++s) hw = (hw ^ l[s]) * 0xD6E8FEB86659FD93ull;
    hw ^= hw >> 32;
    const uint64_t mask = (1ull << a.table_log2) - 1ull;
    uint64_t h = (hw * 0x9E3779B97F4A7C15ull) >> (64u - a.table_log2);
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        unsigned long long o = __hip_atomic_load(a.owner + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o == 0ull) { o = atomicCAS(a.owner + h, 0ull, mine); if (o == 0ull) o = mine; }
        bool same = o == mine;
        if (!same && (uint32_t)((o - 1ull) & 0xfffull) == region) {   // the owner's row: written by an earlier launch
            const uint64_t r2 = (o - 1ull) >> 12;
            if (r2 < a.store.cap) {
                uint32_t q2[8], l2[8];
                hap_cells(a.store.load(r2), q2);
                hap_list(q2, c0, c1, l2);
                same = true;
#pragma unroll
                for (int s = 0; s < 8; ++s) same = same && l2[s] == l[s];
            }
        }
        if (same) { atomicAdd(a.count + h, 1u); return; }
        h = (h + 1) & mask;
    }
    atomicAdd(a.tallies + 1, 1ull);   // every slot is another haplotype's: the download says so
}

__global__ __launch_bounds__(kHapBlock) void hap_count_kernel(HapArgs a) {
    extern __shared__ unsigned int hot_s[];            // [n_regions][2] cover, ref_count
    const uint32_t n_hot = 2u * a.n_regions;           // at most 2 * BK_HAP_MAX_REGIONS: 32 KiB
    lds_table_zero<kHapBlock>(hot_s, n_hot);
    const uint64_t n_rows = a.store.rows_in_store();
    for (uint64_t r = (uint64_t)blockIdx.x * kHapBlock + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * kHapBlock) {
        const RowRegs row = a.store.load(r);
        const uint32_t cell0 = row.cell0, end = row.end;
        uint32_t q[8];
        hap_cells(row, q);
        const auto first_cell = [&](uint32_t i) { return a.sorted[i].x; };
        const uint32_t s0 = first_not_below(0u, a.n_regions, cell0, first_cell);   // the first region that begins at or behind cell0
        const uint32_t t0 = first_not_below(s0, a.n_regions, end, first_cell);     // ... and the first that begins at or behind the row's end
        for (uint32_t i = s0; i < t0; ++i) {
            const uint2 reg = a.sorted[i];
            const uint32_t c0 = reg.x, c1 = reg.x + (reg.y & 0xffffu), region = reg.y >> 16;
            if (c1 > end || region >= a.n_regions) continue;      // (not spanned; the host numbered every region below n_regions)
            uint32_t inside = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) inside += ((q[s] & 0x0fffffffu) - c0 < c1 - c0) ? 1u : 0u;
            atomicAdd(hot_s + 2u * region, 1u);
            if (inside == 0u) { atomicAdd(hot_s + 2u * region + 1u, 1u); continue; }
            uint32_t l[8];
            hap_list(q, c0, c1, l);
            hap_insert(a, r, region, c0, c1, l);
        }
    }
    lds_table_add_to<kHapBlock>(hot_s, n_hot, a.hot);
}

__global__ __launch_bounds__(kHapBlock) void hap_finish_kernel(HapArgs a) {
    const uint64_t n_slots = 1ull << a.table_log2;    // (a multiple of kHapFinishSlots * 64: table_log2 is at least 10)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t per_block = (uint64_t)kHapBlock * kHapFinishSlots;
    for (uint64_t base = (uint64_t)blockIdx.x * per_block + (threadIdx.x >> 6) * (64u * kHapFinishSlots); base < n_slots; base += (uint64_t)gridDim.x * per_block) {
        unsigned long long o[kHapFinishSlots], m[kHapFinishSlots];
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < kHapFinishSlots; ++j) o[j] = a.owner[base + 64u * j + lane];
#pragma unroll
        for (int j = 0; j < kHapFinishSlots; ++j) {
            const bool there = o[j] != 0ull && ((o[j] - 1ull) >> 12) < a.store.cap && (uint32_t)((o[j] - 1ull) & 0xfffull) < a.n_regions;
            if (!there) o[j] = 0ull;
            m[j] = __ballot(there);
            total += (uint32_t)__popcll(m[j]);
        }
        if (total == 0u) continue;
        unsigned long long at = 0ull;
        if (lane == 0) at = atomicAdd(a.tallies + 0, (unsigned long long)total);   // one returning add for the wave's 64 * kHapFinishSlots slots
        at = __shfl(at, 0);
#pragma unroll
        for (int j = 0; j < kHapFinishSlots; ++j) {
            const uint64_t out = at + lane_prefix(m[j]);
            at += (unsigned long long)__popcll(m[j]);
            if (o[j] == 0ull || out >= a.entry_cap) continue;   // (the engine made room for an entry of every slot)
            const uint64_t row = (o[j] - 1ull) >> 12;
            const uint32_t region = (uint32_t)((o[j] - 1ull) & 0xfffull);
            const uint2 reg = a.regions[region];
            uint32_t q[8], l[8];
            hap_cells(a.store.load(row), q);
            const uint32_t n = hap_list(q, reg.x, reg.x + reg.y, l);
            uint32_t e[8], mm[6];                       // offset from the region's first cell | base << 16, zero from n on: the row's packing
#pragma unroll
            for (int s = 0; s < 8; ++s) e[s] = (uint32_t)s < n ? ((l[s] & 0x0fffffffu) - reg.x) | ((l[s] >> 28) << 16) : 0u;
            row_mm_words(e, mm);
            uint2* __restrict__ w = reinterpret_cast<uint2*>(a.entries + out);   // bk_hap_entry: five pairs of words
            w[0] = make_uint2(region, a.count[base + 64u * j + lane]);
            w[1] = make_uint2(n, 0u);
            w[2] = make_uint2(mm[0], mm[1]);
            w[3] = make_uint2(mm[2], mm[3]);
            w[4] = make_uint2(mm[4], mm[5]);
        }
    }
}

}  // namespace

void launch_hap_count(const HapArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream) {
    if (a.n_regions == 0 || rows_upper == 0) return;
    hipLaunchKernelGGL(hap_count_kernel, dim3(row_grid(rows_upper, kHapBlock, n_cus, 2)), dim3(kHapBlock), (size_t)a.n_regions * 2u * sizeof(unsigned int), stream, a);
}

void launch_hap_finish(const HapArgs& a, hipStream_t stream) {
    if (a.n_regions == 0) return;
    const uint64_t blocks = ((1ull << a.table_log2) + kHapBlock * kHapFinishSlots - 1) / (kHapBlock * kHapFinishSlots);
    hipLaunchKernelGGL(hap_finish_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 2048)), dim3(kHapBlock), 0, stream, a);
}

}  // namespace bk
