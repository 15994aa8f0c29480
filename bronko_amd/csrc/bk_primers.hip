// bk_primers.hip -- amplicon primers trimmed from the read ends (bk_primers_set; `bronko call --primers`).
//
// The definition (include/bronko_hip.h): a primer that lies whole at a read's 5' end, or whose reverse
// complement lies whole at its 3' end, within M mismatches and inside the end's run of valid letters, is treated as N.  Every push
// path ends in 2-bit records on the device, and the packers say which records touch a read end (one byte of end flags a record),
// so there is ONE matcher, on the records, between the packer and the kernels that read them (the scan, kmer_dump_count_kernel):
//   primer_trim_kernel   a lane per record.  The workgroup stages the primer table in LDS; the lane loads the record's first 64
//                        bases and its last 64 (the tail does not start on a word boundary: a funnel shift), compares both with
//                        every primer (XOR, fold the bit pairs, popcount: Hamming distance of 2-bit codes), keeps the longest match
//                        per end, and rewrites the record in place: shifted down by p5 bases, length n - p5 - p3, the words behind
//                        the new length zeroed; a record left with fewer than k bases becomes an empty slot (length 0), which the
//                        scan skips like the slots K0 leaves, and comes off the sample's tally of records that hold a run.
// A primer is the same for every lane of a wave at a time (a broadcast read of LDS); its length selects the words compared.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_kernels.h"

namespace bk {
namespace {

constexpr int kTrimBlock = 256;

// d: XOR of two words of 2-bit codes -> one bit per base that differs (bit 2i for base i)
__device__ __forceinline__ uint32_t diff_bases(uint32_t d) { return (d | (d >> 1)) & 0x55555555u; }
// the even bits of the first nb (0..16) bases of a word
__device__ __forceinline__ uint32_t low_bases(int nb) { return nb >= 16 ? 0x55555555u : nb <= 0 ? 0u : ((1u << (2 * nb)) - 1u) & 0x55555555u; }

__global__ __launch_bounds__(kTrimBlock) void primer_trim_kernel(TrimArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tab_s[];   // [n_primers][kPrimerEntryWords]
    for (uint32_t i = threadIdx.x; i < a.n_primers * kPrimerEntryWords; i += kTrimBlock) tab_s[i] = a.table[i];
    __syncthreads();
    const uint64_t n_rec = a.n_records_dev ? min(a.n_records, (uint64_t)*a.n_records_dev) : a.n_records;
    unsigned long long t5 = 0ull, t3 = 0ull, masked = 0ull, emptied = 0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * kTrimBlock + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * kTrimBlock) {
        const int n = a.lens[r];
        const uint32_t fl = n ? a.ends[r] : 0u;
        if (!(fl & 3u) || n < (int)kPrimerMinLen || (uint32_t)n > a.stride_words * 16u) continue;   // (no end, no room for a primer, a malformed record)
        uint32_t* w = a.words + r * a.stride_words;
        const int nw = (n + 15) >> 4;                          // words that hold bases
        auto gw = [&](int i) -> uint32_t { return i >= 0 && i < nw ? w[i] : 0u; };
        // 16 bases from base b on (b may be negative: what lies in front of the record reads as 0 and is never compared)
        auto from_base = [&](int b) -> uint32_t {
            const int q = b >> 4;
            const uint32_t sh = 2u * (uint32_t)(b & 15);
            const uint32_t lo = gw(q);
            return sh ? (lo >> sh) | (gw(q + 1) << (32u - sh)) : lo;
        };
        uint32_t h[4], t[4];                                   // the first 64 bases; the last 64 (base n - 64 + i at position i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { h[j] = (fl & 1u) ? gw(j) : 0u; t[j] = (fl & 2u) ? from_base(n - 64 + 16 * j) : 0u; }
        int p5 = 0, p3 = 0;
        for (uint32_t p = 0; p < a.n_primers; ++p) {
            const uint32_t* e = tab_s + p * kPrimerEntryWords;
            const int L = (int)__builtin_amdgcn_readfirstlane(e[8]);   // (the same primer in every lane: scalar length, scalar branches)
            const int lw = (L + 15) >> 4;
            uint32_t d5 = 0u, d3 = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < lw) {
                    // the primer at bases [0, L); its reverse complement at positions [64 - L, 64) of the tail window
                    d5 += __builtin_popcount(diff_bases(h[j] ^ e[j]) & low_bases(L - 16 * j));
                    d3 += __builtin_popcount(diff_bases(t[3 - j] ^ e[4 + 3 - j]) & ~low_bases(16 * (j + 1) - L) & 0x55555555u);
                }
            }
            if (L <= n) {
                if ((fl & 1u) && d5 <= a.max_mismatches) p5 = max(p5, L);
                if ((fl & 2u) && d3 <= a.max_mismatches) p3 = max(p3, L);
            }
        }
        if (!(p5 | p3)) continue;
        t5 += p5 > 0; t3 += p3 > 0;
        const int left = n - p5 - p3;                          // (both ends of one run may overlap: the whole read is masked)
        masked += (unsigned long long)(left < 0 ? n : p5 + p3);
        const int nl = left >= a.k ? left : 0;
        if (n >= a.k && nl == 0) ++emptied;
        const int nlw = (nl + 15) >> 4;
        for (int j = 0; j < nlw; ++j) {                        // ascending: word j is made of words j + p5 / 16 and the next
            uint32_t x = from_base(p5 + 16 * j);
            if (nl - 16 * j < 16) x &= (1u << (2 * (nl - 16 * j))) - 1u;
            w[j] = x;
        }
        for (int j = nlw; j < nw; ++j) w[j] = 0u;
        a.lens[r] = (uint16_t)nl;
    }
    // the four tallies: a sum over the wave, one atomic a wave and tally that is not zero
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        t5 += __shfl_xor(t5, off); t3 += __shfl_xor(t3, off); masked += __shfl_xor(masked, off); emptied += __shfl_xor(emptied, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (t5) atomicAdd(a.stats + 0, t5);
        if (t3) atomicAdd(a.stats + 1, t3);
        if (masked) atomicAdd(a.stats + 2, masked);
        if (emptied) atomicAdd(a.n_real, 0ull - emptied);      // (the sample's records that hold a run: one fewer per emptied record)
    }
}

}  // namespace

void launch_primer_trim(const TrimArgs& a, int n_cus, hipStream_t stream) {
    if (a.n_records == 0 || a.n_primers == 0) return;
    const uint64_t blocks = (a.n_records + kTrimBlock - 1) / kTrimBlock;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * 8));
    hipLaunchKernelGGL(primer_trim_kernel, dim3(grid), dim3(kTrimBlock), a.n_primers * kPrimerEntryWords * sizeof(uint32_t), stream, a);
}

}  // namespace bk
