// bk_link_row.h -- the sample's row store (bk_link_enable) as its writer and its readers see it: what link_scan_kernel and
// link_count_kernel (bk_linkage.hip), the codon kernels (bk_codons.hip) and the haplotype kernels (bk_haplotypes.hip) share.
//
// A row is bk_link_row (include/bronko_hip.h), 32 bytes, moved as two uint4:
//   lo.x      cell0: the record's first cell
//   lo.y      n (16 bits) | strand << 16 | n_mm << 24
//   lo.zw hi  the mismatches ascending by offset, three bytes each: offset from cell0 (16 bits), base (A C G T = 0 1 2 3); zero from
//             n_mm on.  bk_hap_entry::mm is the same six words with offsets from its region's first cell.
// The one pack and the one unpack of that layout are here (DESIGN.md sections L, T, H).  bk_kernels.h includes this for RowStoreView.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

namespace bk {

// mismatch t of the bytes bk_link_row::mm / bk_hap_entry::mm, on the host (bronko_amd/host/linkage.hpp has the host twins' pair)
inline uint32_t mm_offset(const uint8_t* mm, uint32_t t) { return (uint32_t)mm[3 * t] | ((uint32_t)mm[3 * t + 1] << 8); }
inline uint32_t mm_base(const uint8_t* mm, uint32_t t) { return mm[3 * t + 2]; }

// A row in registers.  e[s] = offset | base << 16, zero from n_mm on; static indices only, so that the eight stay in registers.
struct RowRegs {
    uint32_t cell0, end;                 // the cells [cell0, end): end = cell0 + n
    uint32_t strand, n_mm;
    uint32_t e[8];
};

// eight mismatches as the six words of bk_link_row::mm and bk_hap_entry::mm
__device__ __forceinline__ void row_mm_words(const uint32_t (&e)[8], uint32_t (&w)[6]) {
    w[0] = e[0] | (e[1] << 24); w[1] = (e[1] >> 8) | (e[2] << 16); w[2] = (e[2] >> 16) | (e[3] << 8);
    w[3] = e[4] | (e[5] << 24); w[4] = (e[5] >> 8) | (e[6] << 16); w[5] = (e[6] >> 16) | (e[7] << 8);
}
__device__ __forceinline__ void row_pack(const RowRegs& r, uint4& lo, uint4& hi) {
    uint32_t w[6];
    row_mm_words(r.e, w);
    lo = make_uint4(r.cell0, (r.end - r.cell0) | (r.strand << 16) | (r.n_mm << 24), w[0], w[1]);
    hi = make_uint4(w[2], w[3], w[4], w[5]);
}
__device__ __forceinline__ RowRegs row_unpack(const uint4 lo, const uint4 hi) {
    RowRegs r;
    r.cell0 = lo.x; r.end = lo.x + (lo.y & 0xffffu); r.strand = (lo.y >> 16) & 0xffu; r.n_mm = min(lo.y >> 24, 8u);
    r.e[0] = lo.z & 0xffffffu; r.e[1] = (lo.z >> 24) | ((lo.w & 0xffffu) << 8); r.e[2] = (lo.w >> 16) | ((hi.x & 0xffu) << 16); r.e[3] = hi.x >> 8;
    r.e[4] = hi.y & 0xffffffu; r.e[5] = (hi.y >> 24) | ((hi.z & 0xffffu) << 8); r.e[6] = (hi.z >> 16) | ((hi.w & 0xffu) << 16); r.e[7] = hi.w >> 8;
    return r;
}
// the row's base at offset `off` from its first cell: one of its mismatches, else the reference's
__device__ __forceinline__ uint32_t row_base(const RowRegs& r, uint32_t off, uint32_t ref_base) {
    uint32_t b = ref_base;
#pragma unroll
    for (int s = 0; s < 8; ++s)
        if ((uint32_t)s < r.n_mm && (r.e[s] & 0xffffu) == off) b = (r.e[s] >> 16) & 3u;
    return b;
}

// The store as every kernel argument struct carries it.  link_scan_kernel appends (one returning add to *placed per wave); every
// other kernel runs in a later launch and only reads.
struct RowStoreView {
    uint4* rows;                         // [2 * cap]
    uint64_t cap;                        // in rows
    unsigned long long* placed;          // the rows appended so far (LinkArgs::tallies + 1); above cap only if the engine's bound was wrong
    __device__ __forceinline__ uint64_t rows_in_store() const { return std::min<uint64_t>(*placed, cap); }
    __device__ __forceinline__ RowRegs load(uint64_t r) const { return row_unpack(rows[2u * r], rows[2u * r + 1u]); }   // two 16-byte loads
    __device__ __forceinline__ void store(uint64_t r, const uint4 lo, const uint4 hi) const { rows[2u * r] = lo; rows[2u * r + 1u] = hi; }
};

// the first index in [lo, n) whose key is not below x (key(i) ascending): the rows' binary searches over sites and sorted regions
template <typename Key>
__device__ __forceinline__ uint32_t first_not_below(uint32_t lo, uint32_t n, uint32_t x, Key key) {
    uint32_t hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key(mid) < x) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// A small table of counters privatised in LDS by a workgroup of kBlock lanes: zeroed before the count ...
template <int kBlock>
__device__ __forceinline__ void lds_table_zero(unsigned int* table, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) table[i] = 0u;
    __syncthreads();
}
// ... and behind it one global add per non-zero word
template <int kBlock>
__device__ __forceinline__ void lds_table_add_to(const unsigned int* table, uint32_t n, unsigned int* global) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
        const unsigned int v = table[i];
        if (v) atomicAdd(global + i, v);
    }
}

// the grid of a kernel that strides over at most rows_upper rows, a lane per row: no more workgroups than rows, per_cu to a CU
inline unsigned row_grid(uint64_t rows_upper, int block, int n_cus, int per_cu) {
    const uint64_t blocks = (rows_upper + (uint64_t)block - 1) / (uint64_t)block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * (uint64_t)per_cu));
}

}  // namespace bk
