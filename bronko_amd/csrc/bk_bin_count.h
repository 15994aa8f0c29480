// bk_bin_count.h -- one bin of the binned scan added up and sent to the plane: the body of bin_count_kernel (bk_scan_items.hip),
// shared with level2_kernel (bk_kernels.hip), whose launch the E bins ride in.  An E bin reads only what the scan wrote and adds
// to the E counters with device atomics; so does Level 2, and nothing between the scan and the finalize reads an E counter: the
// two commute and need no launch boundary between them.
#pragma once
#include <hip/hip_runtime.h>

#include "bk_kernels.h"
#include "bk_scan_common.h"

namespace bk {

constexpr int kBinBlock = 256;
constexpr uint32_t kEBinAccWords = 2u * (kEBinSpan + 1u);   // an E bin's accumulator: [2][kEBinSpan + 1] difference arrays (along / against)

// One workgroup of kBinBlock threads per bin.  E bin b: window cells [128 b, 128 b + 383) -- its items start in its 128 cells and
// reach at most 255 further; cells counted by two bins simply receive two additions.  V bin: counters [bin * size, + size) of the
// plane's V part.  acc: the workgroup's LDS accumulator (E: kEBinAccWords words; V: the bin's counters).  E_ONLY: the caller
// knows that bin < n_ebins (the V half is not compiled).
template <bool E_ONLY>
__device__ __forceinline__ void bin_count_body(const BinArgs& b, const uint32_t bin, unsigned int* const acc) {
    const uint32_t n_eb = b.ig.n_ebins, n_bins = n_eb + b.ig.n_vbins;
    const bool is_e = E_ONLY || bin < n_eb;
    const uint32_t vsize = (6u << b.ig.vq_log2) * b.rl;
    const uint32_t n_acc = is_e ? kEBinAccWords : vsize;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (BK_ABLATE(b, 5)) return;
    const uint32_t cap = is_e ? b.ig.cap_e : b.ig.cap_v;
    const uint32_t G = b.ig.grid_max;
    // this bin's buckets of all scan workgroups: one stretch of device memory, workgroup after workgroup
    const unsigned short* const bin_items = b.items + (is_e ? (size_t)bin * G * b.ig.cap_e : (size_t)n_eb * G * b.ig.cap_e + (size_t)(bin - n_eb) * G * b.ig.cap_v);
    // A thread per scan workgroup: this bin's bucket in that workgroup's region.  The bucket's first 48 / 24 slots are asked for
    // together with the table entry that says how many of them hold items, before anything else is done -- one trip to memory,
    // not two (every bin's workgroup reads what 255 others wrote: nothing of it is in this XCD's L2).  Units past the count were
    // not written by this launch (the scan writes out filled units only): what they hold is never taken.
    const bool mine = threadIdx.x < b.n_wg && !BK_ABLATE(b, 1);
    const unsigned short* reg0 = bin_items + (size_t)(mine ? threadIdx.x : 0u) * cap;
    uint32_t hdr0 = 0u;
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0, v2 = v0, v3 = v0, v4 = v0, v5 = v0;
    if (mine) {
        const uint4* q = reinterpret_cast<const uint4*>(reg0);
        hdr0 = b.tab[(size_t)bin * G + threadIdx.x];
        v0 = q[0]; v1 = q[1]; v2 = q[2];
        if (is_e) { v3 = q[3]; v4 = q[4]; v5 = q[5]; }
    }
    for (uint32_t i = threadIdx.x; i < n_acc; i += kBinBlock) acc[i] = 0u;
    if (BK_ABLATE(b, 6)) return;
    if (bin == 0 && threadIdx.x == 0) b.ov_n[b.ov_par ^ 1u] = 0ull;   // the next launch's overflow count starts at zero (once per scan launch: E bin 0, wherever the E bins run)
    __syncthreads();
    auto take = [&](uint32_t it) __attribute__((always_inline)) {
        if (it == 0xffffu) return;
        if (is_e) {
            const uint32_t c = it & 127u, n = ((it >> 7) & 255u) + 1u;
            unsigned int* d = acc + (it >> 15) * (kEBinSpan + 1u);
            __hip_atomic_fetch_add(d + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(d + c + n, 0u - 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            __hip_atomic_fetch_add(acc + (it & 0x7fffu), (it & 0x8000u) ? 0u - 1u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    // the first `left` of the eight items of one 16-byte unit
    auto take8 = [&](const uint4& v, uint32_t left) __attribute__((always_inline)) {
        if (left > 0u) take(v.x & 0xffffu);
        if (left > 1u) take(v.x >> 16);
        if (left > 2u) take(v.y & 0xffffu);
        if (left > 3u) take(v.y >> 16);
        if (left > 4u) take(v.z & 0xffffu);
        if (left > 5u) take(v.z >> 16);
        if (left > 6u) take(v.w & 0xffffu);
        if (left > 7u) take(v.w >> 16);
    };
    // n items (whole 16-byte units are readable): four units in flight at a time
    auto take_items = [&](const unsigned short* p, uint32_t n) __attribute__((always_inline)) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t i0 = 0; i0 < n; i0 += 32u) {
            const uint32_t u0 = i0 >> 3;
            const uint4 v0 = q[u0];
            const uint4 v1 = i0 + 8u < n ? q[u0 + 1u] : z;
            const uint4 v2 = i0 + 16u < n ? q[u0 + 2u] : z;
            const uint4 v3 = i0 + 24u < n ? q[u0 + 3u] : z;
            take8(v0, n - i0);
            take8(v1, n > i0 + 8u ? n - i0 - 8u : 0u);
            take8(v2, n > i0 + 16u ? n - i0 - 16u : 0u);
            take8(v3, n > i0 + 24u ? n - i0 - 24u : 0u);
        }
    };
    const uint32_t spec = is_e ? 48u : 24u;   // slots asked for above
    uint32_t g_mine = 0u;   // items of this bin in my scan workgroup's extension
    if (mine) {
        const uint32_t n_all = hdr0, n = min(n_all, cap);
        g_mine = min(n_all - n, kItemGCap);
        take8(v0, n);
        take8(v1, n > 8u ? n - 8u : 0u);
        take8(v2, n > 16u ? n - 16u : 0u);
        if (is_e) {
            take8(v3, n > 24u ? n - 24u : 0u);
            take8(v4, n > 32u ? n - 32u : 0u);
            take8(v5, n > 40u ? n - 40u : 0u);
        }
        if (n > spec) take_items(reg0 + spec, n - spec);   // (larger buckets than this kernel was written for)
    }
    for (uint32_t wg = threadIdx.x + kBinBlock; wg < b.n_wg && !BK_ABLATE(b, 1); wg += kBinBlock) {   // (more scan workgroups than threads here: never on this chip)
        const uint32_t n_all = b.tab[(size_t)bin * G + wg], n = min(n_all, cap);
        take_items(bin_items + (size_t)wg * cap, n);
        take_items(b.gext + ((size_t)wg * n_bins + bin) * kItemGCap, min(n_all - n, kItemGCap));
    }
    // The extensions: a hot bin (a true variant site: thousands of reads on the same counters) has a hundred items in every scan
    // workgroup's -- every thread reads its own workgroup's, sixteen 16-byte units in flight at a time (the counts are alike from
    // workgroup to workgroup: the threads finish together).  (Sharing the concatenation of all extensions among the threads with a
    // bisection per item was twice as slow: eight dependent LDS reads per item.)
    if (g_mine) {
        const uint4* q = reinterpret_cast<const uint4*>(b.gext + ((size_t)threadIdx.x * n_bins + bin) * kItemGCap);
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t i0 = 0; i0 < g_mine; i0 += 128u) {
            uint4 u[16];
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) u[j] = i0 + 8u * j < g_mine ? q[(i0 >> 3) + j] : z;
#pragma unroll
            for (uint32_t j = 0; j < 16u; ++j) take8(u[j], g_mine > i0 + 8u * j ? g_mine - i0 - 8u * j : 0u);
        }
    }
    if (!BK_ABLATE(b, 7)) {   // the overflow list: everything there that names this bin
        const unsigned long long n_all = b.ov_n[b.ov_par];
        const uint32_t n_ov = (uint32_t)(n_all < (unsigned long long)b.ov_cap ? n_all : (unsigned long long)b.ov_cap);
        for (uint32_t i = threadIdx.x; i < n_ov; i += kBinBlock) {
            const uint32_t e = b.ov[i];
            if ((e >> 16) == bin) take(e & 0xffffu);
        }
    }
    __syncthreads();
    if (is_e) {
        // difference arrays -> per-cell counts: wave 0 the reads along the reference, wave 1 those against it, six entries per lane
        if (wave < 2) {
            unsigned int* d = acc + (uint32_t)wave * (kEBinSpan + 1u) + (uint32_t)lane * 6u;
            const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3], d4 = d[4], d5 = d[5];
            const uint32_t sum = d0 + d1 + d2 + d3 + d4 + d5;
            uint32_t inc = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, off); if (lane >= off) inc += t; }
            uint32_t run = inc - sum;
            run += d0; d[0] = run; run += d1; d[1] = run; run += d2; d[2] = run; run += d3; d[3] = run; run += d4; d[4] = run; run += d5; d[5] = run;
        }
        __syncthreads();
        const uint32_t win_lo = b.win_dev ? b.win_dev[1] : b.win_lo;
        for (uint32_t i = threadIdx.x; i < kEBinSpan && !BK_ABLATE(b, 2) && !BK_ABLATE(b, 3); i += kBinBlock) {
            const uint32_t s0 = acc[i], s1 = acc[(kEBinSpan + 1u) + i];
            if (s0 | s1) {
                const uint32_t cell = win_lo + (bin << kEBinLog2) + i;
                const uint32_t id = b.id_at[cell];   // a counted cell always has a reference k-mer
                const uint32_t rc = ((b.cell_codes[cell >> 4] >> (2u * (cell & 15u))) & 3u) == 2u ? 1u : 0u;
                if (s0) atomicAdd(b.counters + 2 * (size_t)id + rc, (unsigned long long)s0);
                if (s1) atomicAdd(b.counters + 2 * (size_t)id + (1u - rc), (unsigned long long)s1);
            }
        }
    } else if constexpr (!E_ONLY) {
        const uint64_t first = (uint64_t)(bin - n_eb) * vsize;
        unsigned long long* const vc = b.counters + b.v_off + first;
        const uint32_t n_here = (uint32_t)min((uint64_t)vsize, b.v_real_len > first ? b.v_real_len - first : 0ull);
        // a difference: sign-extended, the plane wraps modulo 2^64.  Nothing else adds to this mate file's plane while this kernel runs
        // (the stream orders it against nbatch / level2 / finalize) and a counter belongs to one thread of one workgroup: plain
        // read-modify-write of whole lines instead of a million scattered atomics; v_mode 2: the V part is known to be all zero
        // (a sample's first launch into a clean plane) -- stores only
        if (BK_ABLATE(b, 2) || BK_ABLATE(b, 4)) {
        } else if (b.v_mode == 2 && b.ov_n[b.ov_par] <= (unsigned long long)b.ov_cap) {   // (past the list's end the scan added to the plane itself: it is not all zero then)
            for (uint32_t i = threadIdx.x; i < n_here; i += kBinBlock) vc[i] = (unsigned long long)(long long)(int32_t)acc[i];
        } else if (b.v_mode == 1 || b.v_mode == 2) {
            for (uint32_t i = threadIdx.x; i < n_here; i += kBinBlock) vc[i] += (unsigned long long)(long long)(int32_t)acc[i];
        } else {
            for (uint32_t i = threadIdx.x; i < n_here; i += kBinBlock) {
                const uint32_t v = acc[i];
                if (v) atomicAdd(vc + i, (unsigned long long)(long long)(int32_t)v);
            }
        }
    }
}

}  // namespace bk
