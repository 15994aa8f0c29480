// bk_event_pass.h -- the event pass: the one shape of the six passes that place a record by its anchor k-mers (bk_anchor.h) and count
// rare events in a CAS table -- indels (bk_indels.hip), junctions (bk_junctions.hip), copy-backs (bk_copybacks.hip), duplications
// (bk_duplications.hip), chimeras (bk_chimeras.hip) and breakends (bk_breakends.hip).  A pass keeps what is its rule: `x_anchor` (a
// record's anchors and all that needs no walk; true with a work item for the rare record), `x_walk` (the work item's breakpoint and
// event) and `x_decode` (a table slot as a row of the report).  What is here is what they are called from:
//   event_scan      the body of every x_scan_kernel: a lane per record, the rare records gathered in a queue of the wave and walked a
//                   lane each once 64 wait, the sample's tallies added once per wave and tally;
//   ref_span_count  a record that lies on one diagonal: the Hamming pass with its early exit, two atomics on `span`;
//   event_report    the body of every x_report_kernel: the slots that pass appended with one returning add per wave;
//   launch_event_scan, launch_event_report: their grids.
// The args of a pass are an EventPassArgs (bk_kernels.h) and its extras; its tallies are Args::kScanTallies scan tallies, then
// candidates, reported, overflow.  span_prefix_kernel, the sample's one prefix sum of `span`, is bk_event_pass.hip.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {

constexpr int kEventBlock = 256;
constexpr uint32_t kEventQueue = 128;      // entries of a wave's queue: fewer than 64 wait when up to 64 more arrive

// a lane's scan tallies; event_scan zeroes them (an initialiser or a constructor here costs every scan kernel six VGPRs)
template <int N> struct EventTally { uint32_t v[N]; };

// A record whose two anchors lie on the diagonal dL, whole against the reference: #mismatches, given up above max_mismatches.  A
// record that matches is counted into `span` over the cells between its anchors: +1 at dL + pa + k, -1 at dL + pb + 1.  Returns
// whether it matched: the tallies are the caller's.
__device__ __forceinline__ bool ref_span_count(const AnchorIndex& ix, const uint32_t* __restrict__ w, int32_t n, const Anchors& an, int32_t dL,
                                               uint32_t max_mismatches, unsigned int* __restrict__ span) {
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const uint32_t m = an.against ? mismatches(w, last_word, 0u, (uint32_t)n, ix.rc_words, (int64_t)ix.total_cells - dL - n, max_mismatches)
                                  : mismatches(w, last_word, 0u, (uint32_t)n, ix.ref_words, dL, max_mismatches);
    if (m > max_mismatches) return false;
    atomicAdd(span + (dL + an.pa + ix.k), 1u);
    atomicAdd(span + (dL + an.pb + 1), 0xffffffffu);
    return true;
}

// The scan of a batch by workgroups of kEventBlock threads.  Anchor(a, record, tally, work): the record's fast path; true with `work`
// filled for a record that needs Walk(a, work, tally).  A wave never idles through one lane's walk: the work items wait in its
// queue (LDS, filled through a ballot) until 64 do, and what is left at the end is walked once.
template <class Args, bool (*Anchor)(const Args&, uint32_t, EventTally<Args::kScanTallies>&, uint4&),
          void (*Walk)(const Args&, uint4, EventTally<Args::kScanTallies>&)>
__device__ __forceinline__ void event_scan(const Args& a) {
    __shared__ uint4 queue_s[kEventBlock / 64][kEventQueue];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* const q = queue_s[wave];
    const uint64_t n = a.rec.n_records_dev ? std::min<uint64_t>(a.rec.n_records, *a.rec.n_records_dev) : a.rec.n_records;
    const uint64_t stride = (uint64_t)gridDim.x * kEventBlock;
    EventTally<Args::kScanTallies> t;
#pragma unroll
    for (int i = 0; i < Args::kScanTallies; ++i) t.v[i] = 0u;
    uint32_t qn = 0;                                  // records waiting in the wave's queue (the same in every lane)
    for (uint64_t base = (uint64_t)blockIdx.x * kEventBlock + wave * 64u; base < n; base += stride) {
        const uint64_t r = base + lane;
        uint4 work = make_uint4(0u, 0u, 0u, 0u);
        const bool slow = r < n && Anchor(a, (uint32_t)r, t, work);
        const unsigned long long mask = __ballot(slow);
        if (mask == 0ull) continue;
        if (slow) q[qn + lane_prefix(mask)] = work;   // (qn < 64 here and at most 64 arrive: below kEventQueue)
        qn += (uint32_t)__popcll(mask);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the queue is the wave's own: its lanes' stores before its lanes' loads)
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64u) {
            qn -= 64u;
            work = q[qn + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            Walk(a, work, t);
        }
    }
    if (lane < qn) Walk(a, q[lane], t);
#pragma unroll
    for (int i = 0; i < Args::kScanTallies; ++i) {
        const uint32_t sum = wave_total(t.v[i]);
        if (lane == 0 && sum) atomicAdd(a.tallies + i, (unsigned long long)sum);
    }
}

// The report over the table's slots.  Decode(a, slot, row, pass): whether the slot holds an event (a candidate), then its row and
// whether it passes the thresholds; the rows that pass go to a.rows[.. a.row_cap) in no order.
template <class Args, class Row, bool (*Decode)(const Args&, uint64_t, Row&, bool&)>
__device__ __forceinline__ void event_report(const Args& a) {
    const uint64_t n_slots = 1ull << a.log2n;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kEventBlock + (threadIdx.x & ~63u); base < n_slots; base += (uint64_t)gridDim.x * kEventBlock) {
        const uint64_t i = base + lane;
        bool pass = false;
        Row row{};
        const bool there = i < n_slots && Decode(a, i, row, pass);
        const unsigned long long m_there = __ballot(there), m_pass = __ballot(pass);
        if (m_there == 0ull) continue;
        unsigned long long at = 0ull;
        if (lane == 0) {
            atomicAdd(a.tallies + Args::kCandidates, (unsigned long long)__popcll(m_there));
            if (m_pass) at = atomicAdd(a.tallies + Args::kReported, (unsigned long long)__popcll(m_pass));
        }
        at = __shfl(at, 0);
        if (pass) {
            const uint64_t o = at + lane_prefix(m_pass);
            if (o < a.row_cap) a.rows[o] = row;
        }
    }
}

// the scan's grid: at most 8 workgroups a CU (grid-stride), at least one; the report's: at most 2048
inline unsigned event_scan_grid(uint64_t n_records, int n_cus) {
    const uint64_t blocks = (n_records + kEventBlock - 1) / kEventBlock;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * 8));
}
inline unsigned event_report_grid(uint32_t log2n) {
    const uint64_t blocks = ((1ull << log2n) + kEventBlock - 1) / kEventBlock;
    return (unsigned)std::min<uint64_t>(blocks, 2048);
}
template <class Args> void launch_event_scan(void (*kernel)(Args), const Args& a, int n_cus, hipStream_t stream) {
    if (a.rec.n_records == 0) return;
    hipLaunchKernelGGL(kernel, dim3(event_scan_grid(a.rec.n_records, n_cus)), dim3(kEventBlock), 0, stream, a);
}
template <class Args> void launch_event_report(void (*kernel)(Args), const Args& a, hipStream_t stream) {
    hipLaunchKernelGGL(kernel, dim3(event_report_grid(a.log2n)), dim3(kEventBlock), 0, stream, a);
}

}  // namespace bk
