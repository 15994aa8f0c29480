// bk_adapters.hip -- 3' sequencing adapters cut off the reads (bk_adapters_set; `bronko call --adapter`).
//
// The definition (include/bronko_hip.h): R = the read's maximal suffix of valid letters, r its length.  A
// position p <= r - O matches an adapter A when Hamming(R[p : p + l], A[0 : l]) <= floor(E * l), l = min(|A|, r - p): the whole
// adapter anywhere in R, or a prefix of at least O bases at R's end.  The read is truncated at the smallest matching p.
// R is exactly the record whose end flags say "my last base is the read's last letter" (kEndLast), so the matcher runs on the
// records, like primer_trim_kernel and in front of it (a 3' primer is then found at the new end: the record keeps its flags).
// An adapter is searched at EVERY position of the record, and records reach 65,520 bases, so the work is split over positions:
//   adapter_find_kernel  a lane per (record, 16-base word); 2^lg lanes side by side share a record and stride over its words, so
//                        a short record costs its neighbours nothing and a long one is spread over up to a whole block.  The lane
//                        loads its word and the next four (80 bases: a 64-base window at each of its 16 offsets), and per offset
//                        and adapter takes the Hamming distance of the first 16 bases (funnel shift, XOR, fold the bit pairs,
//                        popcount); only a window that is within the allowance there has its other three words compared.  The
//                        lane's leftmost match goes into cut[record] with one atomicMin.
//   adapter_trim_kernel  a lane per record: where cut[record] was set, the record's length becomes p, its last word is masked, the
//                        words behind are zeroed (what the packers and primer_trim_kernel guarantee, and the scan relies on);
//                        fewer than k bases left make it an empty slot that comes off the sample's tally of records that hold a
//                        run.  cut[record] goes back to kNoCut: the array needs no clearing between batches.
// The adapters, their lengths and the allowance are kernel arguments: the same for every lane, they live in scalar registers.  No
// float runs here: floor(E * l) comes from the host as the steps of a staircase (AdapterArgs::allowed_steps).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_kernels.h"

namespace bk {
namespace {

constexpr int kAdapterBlock = 256;

// d: XOR of two words of 2-bit codes -> one bit per base that differs (bit 2i for base i)
__device__ __forceinline__ uint32_t diff_bases(uint32_t d) { return (d | (d >> 1)) & 0x55555555u; }
// the even bits of the first nb (<= 0 .. >= 16) bases of a word
__device__ __forceinline__ uint32_t low_bases(int nb) { return nb >= 16 ? 0x55555555u : nb <= 0 ? 0u : ((1u << (2 * nb)) - 1u) & 0x55555555u; }
// 16 bases from base o (0..15) of the 32 in lo, hi
__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, int o) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (2 * o)); }

__global__ __launch_bounds__(kAdapterBlock) void adapter_find_kernel(AdapterArgs a, uint32_t lg) {
    const uint64_t n_rec = a.n_records_dev ? min(a.n_records, (uint64_t)*a.n_records_dev) : a.n_records;
    const uint32_t lanes = 1u << lg, wl = threadIdx.x & (lanes - 1u), rpb = (uint32_t)kAdapterBlock >> lg;
    const int O = (int)a.min_overlap;
    for (uint64_t r = (uint64_t)blockIdx.x * rpb + (threadIdx.x >> lg); r < n_rec; r += (uint64_t)gridDim.x * rpb) {
        const int n = a.lens[r];
        if (n < O || (uint32_t)n > a.stride_words * 16u) continue;   // (an empty slot, no room for an overlap, a malformed record)
        if (!(a.ends[r] & kEndLast)) continue;
        const uint32_t* w = a.words + r * a.stride_words;
        const int nw = (n + 15) >> 4;                          // words that hold bases
        uint32_t found = kNoCut;
        for (int wi = (int)wl; 16 * wi <= n - O && found == kNoCut; wi += (int)lanes) {
            uint32_t c[5];                                     // bases [16 wi, 16 wi + 80); what lies behind the record reads as 0
#pragma unroll
            for (int j = 0; j < 5; ++j) { const uint32_t v = w[min(wi + j, nw - 1)]; c[j] = wi + j < nw ? v : 0u; }   // (five loads in flight)
            for (int o = 0; o < 16; ++o) {
                const int rem = n - (16 * wi + o);             // bases from this position to the record's end
                if (rem < O) break;
                // floor(E * min(len, rem)) = min(floor(E * len), floor(E * rem)): the allowance does not fall as l grows
                const uint32_t alr = (uint32_t)__builtin_popcountll(a.allowed_steps & (rem >= 64 ? ~0ull : (1ull << rem) - 1ull));
                const uint32_t x0 = funnel(c[0], c[1], o), rm0 = low_bases(rem);
                bool hit = false;
                for (uint32_t ai = 0; ai < a.n_adapters; ++ai) {
                    const AdapterEntry& e = a.adapters[ai];
                    const uint32_t al = min(e.allowed, alr);
                    uint32_t d = __builtin_popcount(diff_bases(x0 ^ e.code[0]) & e.mask[0] & rm0);
                    if (d > al) continue;                      // (the prefilter: nearly every window ends here)
#pragma unroll
                    for (int j = 1; j < 4; ++j)
                        d += __builtin_popcount(diff_bases(funnel(c[j], c[j + 1], o) ^ e.code[j]) & e.mask[j] & low_bases(rem - 16 * j));
                    hit |= d <= al;
                }
                if (hit) { found = (uint32_t)(16 * wi + o); break; }
            }
        }
        if (found != kNoCut) atomicMin(a.cut + r, found);
    }
}

__global__ __launch_bounds__(kAdapterBlock) void adapter_trim_kernel(AdapterArgs a) {
    const uint64_t n_rec = a.n_records_dev ? min(a.n_records, (uint64_t)*a.n_records_dev) : a.n_records;
    unsigned long long cut = 0ull, removed = 0ull, emptied = 0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * kAdapterBlock + threadIdx.x; r < n_rec; r += (uint64_t)gridDim.x * kAdapterBlock) {
        const uint32_t p = a.cut[r];
        if (p == kNoCut) continue;
        a.cut[r] = kNoCut;
        const int n = a.lens[r];
        if ((int)p >= n) continue;                             // (never: adapter_find_kernel looked at positions [0, n - O])
        ++cut; removed += (unsigned long long)(n - (int)p);
        const int nl = (int)p >= a.k ? (int)p : 0;
        if (n >= a.k && nl == 0) ++emptied;
        uint32_t* w = a.words + r * a.stride_words;
        if (nl & 15) w[nl >> 4] &= (1u << (2 * (nl & 15))) - 1u;
        for (int j = (nl + 15) >> 4; j < (n + 15) >> 4; ++j) w[j] = 0u;
        a.lens[r] = (uint16_t)nl;
    }
    // the tallies: a sum over the wave, one atomic a wave and tally that is not zero
#pragma unroll
    for (int off = 32; off; off >>= 1) { cut += __shfl_xor(cut, off); removed += __shfl_xor(removed, off); emptied += __shfl_xor(emptied, off); }
    if ((threadIdx.x & 63u) == 0u) {
        if (cut) atomicAdd(a.stats + 0, cut);
        if (removed) atomicAdd(a.stats + 1, removed);
        if (emptied) atomicAdd(a.n_real, 0ull - emptied);     // (the sample's records that hold a run: one fewer per emptied record)
    }
}

}  // namespace

void launch_adapter_trim(const AdapterArgs& a, int n_cus, hipStream_t stream) {
    if (a.n_records == 0 || a.n_adapters == 0) return;
    uint32_t lg = 0;
    while (lg < 8 && (1u << lg) < a.stride_words) ++lg;      // lanes a record: the next power of two, a block at the most
    const uint64_t rpb = (uint64_t)kAdapterBlock >> lg, cap = (uint64_t)n_cus * 8;
    const unsigned find_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n_records + rpb - 1) / rpb, cap));
    const unsigned trim_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((a.n_records + kAdapterBlock - 1) / kAdapterBlock, cap));
    hipLaunchKernelGGL(adapter_find_kernel, dim3(find_grid), dim3(kAdapterBlock), 0, stream, a, lg);
    hipLaunchKernelGGL(adapter_trim_kernel, dim3(trim_grid), dim3(kAdapterBlock), 0, stream, a);
}

}  // namespace bk
