// bk_regions.hip -- the per-region depth report (bk_sample_region_depths; `bronko call --regions / --region-window`).
//
// The rule (include/bronko_hip.h): depth[p] = the four bases' forward + reverse depths of position p of the
// selected genome; per region [start, end) of one sequence: sum, min, max, the lower median (index (L - 1) / 2 of the sorted
// depths) and the positions with depth >= min_depth.  Integers only; no cap on L; the median exact over the whole u64 range.
//   region_depth_kernel   one workgroup (four waves) per region of the selected genome file's slice of the table.
//                         Pass 1, strided over the region's positions: sum, min, max, covered -- summed over the wave with
//                         shuffles, over the four waves through LDS.  A region of at most kRegionLdsDepths positions leaves its
//                         depths in LDS on the way.
//                         Median by value, not by sort: [min, max] is bisected, each step a workgroup-wide count of depth <= mid
//                         against the rank (L - 1) / 2 + 1; the smallest value whose count reaches the rank is the element at that
//                         index.  min == max takes no step, a range of R values at most ceil(log2 R), 64 at the most.  A staged
//                         region's steps read LDS, a longer one reads the planes again.  One barrier a step: the waves' counts
//                         alternate between two rows of LDS.
// Every lane of the workgroup follows the same [lo, hi], so the loop and its barriers are uniform.
#include <hip/hip_runtime.h>

#include "bk_kernels.h"

namespace bk {
namespace {

constexpr int kRegionBlock = 256;
constexpr int kRegionWaves = kRegionBlock / 64;

// depth of a cell: the eight counts of its two depth rows (32 bytes each, 32-byte aligned) as four 16-byte loads
__device__ __forceinline__ unsigned long long cell_depth(const RegionArgs& a, uint64_t cell) {
    const ulonglong2* fr = reinterpret_cast<const ulonglong2*>(a.pileup + 0 * a.plane + cell * 4);
    const ulonglong2* rr = reinterpret_cast<const ulonglong2*>(a.pileup + 1 * a.plane + cell * 4);
    const ulonglong2 f0 = fr[0], f1 = fr[1], r0 = rr[0], r1 = rr[1];
    return f0.x + f0.y + f1.x + f1.y + r0.x + r0.y + r1.x + r1.y;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(kRegionBlock) void region_depth_kernel(RegionArgs a) {
    __shared__ unsigned long long depth_s[kRegionLdsDepths];
    __shared__ unsigned long long red_s[4][kRegionWaves];        // sum, min, max, covered of each wave
    __shared__ unsigned int cnt_s[2][kRegionWaves];              // a step's counts of each wave, by the step's parity
    const int file = a.out->file_id;
    const uint32_t lo_r = file >= 0 ? a.file_off[file] : 0u;
    const uint32_t n_r = file >= 0 ? a.file_off[file + 1] - lo_r : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.summary->file_id = file; a.summary->n_regions = n_r; }
    if (blockIdx.x >= n_r) return;                               // (the grid is the largest slice's)
    const uint2 reg = a.table[lo_r + blockIdx.x];
    const uint64_t cell0 = reg.x;
    const uint32_t L = reg.y;
    const bool staged = L <= kRegionLdsDepths;
    const int wave = threadIdx.x >> 6;

    // pass 1
    unsigned long long sum = 0ull, mn = ~0ull, mx = 0ull, cov = 0ull;
    for (uint32_t i = threadIdx.x; i < L; i += kRegionBlock) {
        const unsigned long long d = cell_depth(a, cell0 + i);
        if (staged) depth_s[i] = d;
        sum += d;
        mn = d < mn ? d : mn;
        mx = d > mx ? d : mx;
        cov += d >= a.min_depth ? 1ull : 0ull;
    }
    sum = wave_sum(sum); cov = wave_sum(cov);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long om = __shfl_xor(mn, off), ox = __shfl_xor(mx, off);
        mn = om < mn ? om : mn;
        mx = ox > mx ? ox : mx;
    }
    if ((threadIdx.x & 63) == 0) { red_s[0][wave] = sum; red_s[1][wave] = mn; red_s[2][wave] = mx; red_s[3][wave] = cov; }
    __syncthreads();                                             // (the staged depths are written, too)
    sum = 0ull; mn = ~0ull; mx = 0ull; cov = 0ull;
#pragma unroll
    for (int w = 0; w < kRegionWaves; ++w) {
        sum += red_s[0][w]; cov += red_s[3][w];
        mn = red_s[1][w] < mn ? red_s[1][w] : mn;
        mx = red_s[2][w] > mx ? red_s[2][w] : mx;
    }

    // the median: the smallest v in [min, max] with #{depth <= v} >= rank
    const uint32_t rank = (L - 1u) / 2u + 1u;
    unsigned long long lo = mn, hi = mx;
    for (unsigned step = 0; lo < hi; ++step) {
        const unsigned long long mid = lo + (hi - lo) / 2ull;
        unsigned int c = 0u;
        if (staged) {
            for (uint32_t i = threadIdx.x; i < L; i += kRegionBlock) c += depth_s[i] <= mid ? 1u : 0u;
        } else {
            for (uint32_t i = threadIdx.x; i < L; i += kRegionBlock) c += cell_depth(a, cell0 + i) <= mid ? 1u : 0u;
        }
        c = wave_sum(c);
        if ((threadIdx.x & 63) == 0) cnt_s[step & 1u][wave] = c;
        __syncthreads();                                         // (the row of step - 1 was read before this barrier, the one of step + 1 is written behind it)
        unsigned int total = 0u;
#pragma unroll
        for (int w = 0; w < kRegionWaves; ++w) total += cnt_s[step & 1u][w];
        if (total >= rank) hi = mid; else lo = mid + 1ull;
    }

    if (threadIdx.x == 0) {
        RegionDepthDev r;
        r.sum = sum; r.min = mn; r.max = mx; r.median = lo; r.covered = cov;
        a.rows[blockIdx.x] = r;
        uint64_t* tally = cov == L ? &a.summary->full : cov == 0ull ? &a.summary->empty : &a.summary->partial;
        atomicAdd(reinterpret_cast<unsigned long long*>(tally), 1ull);
    }
}

}  // namespace

void launch_region_depths(const RegionArgs& a, uint32_t max_file_regions, hipStream_t stream) {
    hipLaunchKernelGGL(region_depth_kernel, dim3(max_file_regions ? max_file_regions : 1u), dim3(kRegionBlock), 0, stream, a);
}

}  // namespace bk
