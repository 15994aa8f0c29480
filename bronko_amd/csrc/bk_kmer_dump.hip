// bk_kmer_dump.hip -- the sample's k-mer count table (bk_kmer_dump_*; `bronko call --keep-kmer-info`).
//
// The reference counts every reads file with KMC3 (-k -b -ci -cs -cx) and, under --keep-kmer-info, keeps the dump of that count
// (call.rs:1152-1233, :1202-1211).  The engine never builds that table -- the binned scan works from each read's diagonal -- so
// this is a counting pass of its own over the same records:
//   kmer_dump_count_kernel   one lane per (record, k-mer start): the strand-specific k-mer, straight from the record's 2-bit
//                            words, into an open-addressing table keyed by k-mer | mate << 62 (u32 counts that saturate);
//   kmer_dump_select_kernel  at finalize, per mate file: the entries with ci <= count <= cx, as (k-mer, min(count, cs)), one
//                            append per wave; and the mate file's distinct k-mers;
//   rocprim radix sort       the selected pairs by k-mer over bits [0, 2k): ascending lexicographic order (A < C < G < T).
// The table grows like full_kmer_stats' table (GrowTable::ensure_room of bk_engine.cpp, ktab_rehash_kernel): same slot hash.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

#include "bk_kernels.h"

namespace bk {
namespace {

constexpr uint32_t kDumpFillWords = 1024;   // = ktab_fill_words(): new-key tallies behind the overflow flag, overflow[4 + i]
constexpr uint32_t kDumpTile = 16;          // records per tile of the count kernel

__device__ __forceinline__ uint32_t lane_rank(unsigned long long m) {   // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The key's slot: the same hash as ktab_insert_key / ktab_rehash_kernel, so that the rehash serves both tables.
// A slot is loaded first: a key already there costs one non-returning add.  Only a slot that looks free is claimed with a CAS --
// a stale "free" (another XCD's L2) is settled by the CAS's return value; keys are never removed, so a key read is never stale.
__device__ __forceinline__ void dump_insert(unsigned long long* __restrict__ keys, unsigned int* __restrict__ cnt, uint32_t log2n,
                                            unsigned long long* overflow, unsigned long long key) {
    const uint64_t mask = (1ull << log2n) - 1ull;
    uint64_t h = (key * 0x9E3779B97F4A7C15ull) >> (64 - log2n);
    for (uint32_t probes = 0; probes < 4096; ++probes) {
        unsigned long long cur = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool fresh = false;
        if (cur == ~0ull) {
            cur = atomicCAS(keys + h, ~0ull, key);
            fresh = cur == ~0ull;
        }
        if (fresh || cur == key) {
            // saturates far above any -cx (a count never wraps: a k-mer seen 2^32 times is still dropped by -cx)
            if (cnt[h] < 0xf0000000u) atomicAdd(cnt + h, 1u);
            if (fresh) atomicAdd(overflow + 4 + (h & (kDumpFillWords - 1u)), 1ull);   // the engine grows the table by its fill
            return;
        }
        h = (h + 1) & mask;
    }
    *overflow = 1ull;   // (the engine keeps the load below one half: unreachable unless the table cannot grow any more)
}

// Records in tiles of kDumpTile; a tile's (record, start) pairs are spread over the workgroup's lanes, neighbouring lanes on
// neighbouring starts of one record (their words are the same few cache lines).  Record r holds lens[r] bases, base i in word
// i / 16 at bits [2 (i % 16), 2 (i % 16) + 2); a k-mer reads at most three words, none past its last base.
__global__ __launch_bounds__(256) void kmer_dump_count_kernel(const uint32_t* __restrict__ words, const uint16_t* __restrict__ lens,
                                                             uint64_t n_records, const unsigned long long* __restrict__ n_records_dev,
                                                             uint32_t stride_words, int k, uint32_t mate, unsigned long long* __restrict__ keys,
                                                             unsigned int* __restrict__ cnt, uint32_t log2n, unsigned long long* overflow) {
    const uint64_t n = n_records_dev ? std::min<uint64_t>(n_records, *n_records_dev) : n_records;
    const uint32_t per = stride_words * 16u - (uint32_t)k + 1u;   // k-mer starts a record slot can hold
    const uint64_t n_tiles = (n + kDumpTile - 1) / kDumpTile;
    const unsigned long long mate_bit = (unsigned long long)mate << 62;
    const unsigned long long kmask = (1ull << (2 * k)) - 1ull;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t r0 = t * kDumpTile;
        const uint32_t n_here = (uint32_t)std::min<uint64_t>(kDumpTile, n - r0);
        for (uint32_t j = threadIdx.x; j < n_here * per; j += 256u) {
            const uint32_t rl = j / per, s = j - rl * per;
            const uint64_t r = r0 + rl;
            const uint32_t len = lens[r];
            if (s + (uint32_t)k > len) continue;
            const uint32_t* w = words + r * stride_words;
            const uint32_t w0 = s >> 4, sh = 2u * (s & 15u), wl = (s + (uint32_t)k - 1u) >> 4;
            unsigned long long x = w[w0];
            if (wl > w0) x |= (unsigned long long)w[w0 + 1] << 32;
            x >>= sh;
            if (wl > w0 + 1) x |= (unsigned long long)w[w0 + 2] << (64u - sh);   // (sh > 0 here: 2k <= 62 bits span three words only off a word's start)
            // base s + i sits at bits [2i, 2i + 2): reverse the 2-bit groups so that base s leads (MSB-first, kmer_to_u64)
            x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
            x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
            x = __builtin_bswap64(x) >> (64 - 2 * k);
            dump_insert(keys, cnt, log2n, overflow, (x & kmask) | mate_bit);
        }
    }
}

// The mate file's entries: distinct keys counted (res[1]), kept ones appended (res[0] = n_kept when the kernel ends) as
// (k-mer, min(count, cs)), at most `cap` written.  A workgroup owns a contiguous range of slots: it counts what it keeps there, takes
// its place with ONE returning add (an add per wave on one word was 22 ms at 2^28 slots: the word takes ~90 adds per us), then
// reads the range again and writes its entries in slot order (wave ballots, a prefix over the workgroup's four waves).
__global__ __launch_bounds__(256) void kmer_dump_select_kernel(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                                                              uint64_t n_slots, uint64_t per_wg, uint32_t mate, unsigned long long ci,
                                                              unsigned long long cs, unsigned long long cx, unsigned long long* __restrict__ out_keys,
                                                              unsigned int* __restrict__ out_cnt, uint64_t cap, unsigned long long* res) {
    __shared__ unsigned int wave_n[4], wave_d[4];
    __shared__ unsigned long long wg_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * per_wg, hi = std::min<uint64_t>(n_slots, lo + per_wg);
    auto kept_at = [&](uint64_t i, unsigned int* c_out) -> int {   // 0 free / other mate, 1 distinct only, 2 kept
        if (i >= hi) return 0;
        const unsigned long long key = keys[i];
        if (key == ~0ull || (uint32_t)(key >> 62) != mate) return 0;
        const unsigned int c = cnt[i];
        *c_out = c;
        return c >= ci && c <= cx ? 2 : 1;
    };
    unsigned int n_kept = 0, n_distinct = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) {
        unsigned int c = 0;
        const int st = kept_at(i, &c);
        n_distinct += st != 0;
        n_kept += st == 2;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        n_kept += (unsigned int)__shfl_xor((int)n_kept, off);
        n_distinct += (unsigned int)__shfl_xor((int)n_distinct, off);
    }
    if (lane == 0) { wave_n[wave] = n_kept; wave_d[wave] = n_distinct; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tk = (unsigned long long)wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        const unsigned long long td = (unsigned long long)wave_d[0] + wave_d[1] + wave_d[2] + wave_d[3];
        wg_base = tk ? atomicAdd(res, tk) : 0ull;
        if (td) atomicAdd(res + 1, td);
    }
    __syncthreads();
    const unsigned long long tk = (unsigned long long)wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    if (tk == 0) return;
    unsigned long long at = wg_base;
    __syncthreads();   // (wave_n is reused below)
    for (uint64_t t = lo; t < hi; t += 256) {
        unsigned int c = 0;
        const bool kept = kept_at(t + threadIdx.x, &c) == 2;
        const unsigned long long m = __ballot(kept);
        if (lane == 0) wave_n[wave] = (unsigned int)__popcll(m);
        __syncthreads();
        unsigned long long before = 0;
        for (uint32_t w = 0; w < wave; w++) before += wave_n[w];
        if (kept) {
            const uint64_t o = at + before + lane_rank(m);
            if (o < cap) { out_keys[o] = keys[t + threadIdx.x] & ~(1ull << 62); out_cnt[o] = (unsigned int)std::min<unsigned long long>(c, cs); }
        }
        at += (unsigned long long)wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        __syncthreads();
    }
}

}  // namespace

void launch_kmer_dump_count(const RecordsView& rec, int k, uint32_t mate, unsigned long long* keys, unsigned int* cnt, uint32_t log2n,
                            unsigned long long* overflow, int n_cus, hipStream_t stream) {
    if (rec.n_records == 0 || rec.stride_words * 16u < (uint32_t)k) return;   // (records too short to hold a k-mer)
    const uint64_t tiles = (rec.n_records + kDumpTile - 1) / kDumpTile;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)n_cus * 8));
    hipLaunchKernelGGL(kmer_dump_count_kernel, dim3(grid), dim3(256), 0, stream, rec.words, rec.lens, rec.n_records, rec.n_records_dev,
                       rec.stride_words, k, mate, keys, cnt, log2n, overflow);
}

void launch_kmer_dump_select(const unsigned long long* keys, const unsigned int* cnt, uint32_t log2n, uint32_t mate, unsigned long long ci,
                             unsigned long long cs, unsigned long long cx, unsigned long long* out_keys, unsigned int* out_cnt, uint64_t cap,
                             unsigned long long* res, hipStream_t stream) {
    const uint64_t n = 1ull << log2n;
    const uint64_t grid = std::min<uint64_t>((n + 255) / 256, 256 * 8), per_wg = (n + grid - 1) / grid;
    hipLaunchKernelGGL(kmer_dump_select_kernel, dim3((unsigned)grid), dim3(256), 0, stream, keys, cnt, n, per_wg, mate, ci, cs, cx, out_keys, out_cnt, cap, res);
}

hipError_t kmer_dump_sort(void* tmp, size_t& tmp_bytes, unsigned long long* keys_in, unsigned long long* keys_out, unsigned int* vals_in,
                          unsigned int* vals_out, uint64_t n, int k, hipStream_t stream) {
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, (unsigned)(2 * k), stream);
}

}  // namespace bk
