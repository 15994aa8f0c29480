// bk_duplications.hip -- tandem duplications and the origin of a circular genome from the reads (bk_duplications_enable; `bronko call --duplications`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section V; bronko_amd/host/duplications.cpp and tests/duplications_ref.py restate it.
//   duplication_scan_kernel         behind the scan of the same records, a lane per record, shaped as junction_scan_kernel (bk_junctions.hip):
//                                   the anchors through bk_anchor.h, delta = 0 inline (the Hamming pass with an early exit, two atomics
//                                   on `span`), `forward` and `short` a tally each.  A backward jump of min_len or more is rare: those
//                                   records are gathered in a queue of the wave (LDS, filled through a ballot) and walked a lane each
//                                   once 64 wait.  What differs from the junction is asked before the queue: each arm against the
//                                   sequence's borders and the runs of other letters on its own, and the breakpoint's range clipped to
//                                   the sequence, so that an arm may end at the sequence's last cell or begin at its first.  The walk
//                                   (breakpoint_walk) and the event table (event_insert, key pos | E << 32) are bk_anchor.h's, shared
//                                   with junction_scan_kernel.  The sample's tallies: one add per wave and tally.
//   duplication_span_prefix_kernel  at the sample's end: `span` prefix-summed in place by one workgroup.
//   duplication_report_kernel       the table's events with enough reads, appended with one returning add per wave.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kDuplicationBlock = 256;
constexpr uint32_t kDuplicationQueue = 128;   // entries of a wave's queue: fewer than 64 wait when up to 64 more arrive
constexpr int kScanTallies = 7;               // records, anchored, ref_spanning, supporting, short, forward, discordant
constexpr int kCandidates = 7, kReported = 8, kOverflow = 9;   // DuplicationArgs::tallies behind them

struct DuplicationTally { uint32_t v[kScanTallies] = {0, 0, 0, 0, 0, 0, 0}; };
enum { T_RECORDS, T_ANCHORED, T_SPANNING, T_SUPPORTING, T_SHORT, T_FORWARD, T_DISCORDANT };

// A record's anchors and all that needs no breakpoint.  Returns true with `work` filled for a record with delta <= -min_len that
// passed the checks: {record | against << 31, p0 | p1 << 16, dL, dR}, [p0, p1] the breakpoint's range clipped to the sequence.
__device__ __forceinline__ bool duplication_anchor(const DuplicationArgs& a, uint32_t r, DuplicationTally& t, uint4& work) {
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    if (n < k) return false;                          // (trimmed away: no record any more)
    t.v[T_RECORDS]++;
    if (n < 2 * k) return false;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    Anchors an;
    if (!anchors_of(a.ix, w, n, an)) return false;
    const bool against = an.against;
    const int32_t pa = an.pa, pb = an.pb;
    t.v[T_ANCHORED]++;
    const int32_t dL = (int32_t)an.ca - pa, dR = (int32_t)an.cb - pb, delta = dR - dL;
    const uint32_t s = seq_of(a.ix, an.ca);
    if (seq_of(a.ix, an.cb) != s) return false;
    if (delta == 0) {
        if (!arm_placed(a.ix, s, dL, dL + n)) return false;
        const uint32_t last_word = (uint32_t)(n - 1) >> 4;
        const uint32_t m = against ? mismatches(w, last_word, 0u, (uint32_t)n, a.ix.rc_words, (int64_t)a.ix.total_cells - dL - n, a.max_mismatches)
                                   : mismatches(w, last_word, 0u, (uint32_t)n, a.ix.ref_words, dL, a.max_mismatches);
        if (m > a.max_mismatches) { t.v[T_DISCORDANT]++; return false; }
        t.v[T_SPANNING]++;
        atomicAdd(a.span + (dL + pa + k), 1u);
        atomicAdd(a.span + (dL + pb + 1), 0xffffffffu);
        return false;
    }
    if (delta > 0) { t.v[T_FORWARD]++; return false; }
    if (-delta < (int32_t)a.min_len) { t.v[T_SHORT]++; return false; }
    // a backward jump: the record's two ends inside the sequence (what lies between them may overhang either border: it is never read)
    const int32_t lo = (int32_t)a.ix.seq_lo[s], hi = (int32_t)a.ix.seq_lo[s + 1];
    if (dL < lo || dR + n > hi) return false;
    const int32_t p0 = max(pa + k, lo - dR), p1 = min(pb, hi - dL);
    if (p0 > p1) return false;
    // the arms [dL, dL + p1) and [dR + p0, dR + n): inside the sequence by the clipping, neither empty (0 < p0 <= p1 < n)
    if (!arm_placed(a.ix, s, dL, dL + p1) || !arm_placed(a.ix, s, dR + p0, dR + n)) return false;
    work = make_uint4(r | (against ? 0x80000000u : 0u), (uint32_t)p0 | ((uint32_t)p1 << 16), (uint32_t)dL, (uint32_t)dR);
    return true;
}

// delta <= -min_len: the breakpoint, the normalised event, the table
__device__ __forceinline__ void duplication_walk(const DuplicationArgs& a, const uint4 work, DuplicationTally& t) {
    const uint32_t r = work.x & 0x7fffffffu;
    const bool against = (work.x >> 31) != 0u;
    const int32_t p0 = (int32_t)(work.y & 0xffffu), p1 = (int32_t)(work.y >> 16), dL = (int32_t)work.z, dR = (int32_t)work.w;
    const int32_t n = (int32_t)a.rec.lens[r], E = dL - dR;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const OrientedRecord rec{a.ix, w, n, last_word, against};
    int32_t best_p;
    const int32_t best = breakpoint_walk(rec, p0, p1, dL, dR, best_p);
    if (best > (int32_t)a.max_mismatches) { t.v[T_DISCORDANT]++; return; }
    int32_t pos = dL + best_p;
    // the two floors: pos - 1 lies in the left arm and pos - E in the right one, and an arm holds ACGT only, so each floor is the
    // first cell of the stretch of ACGT letters in front of its arm (dL is a cell of the sequence: lo <= dL < dL + p1 <= hi)
    const uint32_t s = seq_of(a.ix, (uint32_t)dL);
    const int32_t FL = acgt_floor_in(a.ix, s, dL), FR = acgt_floor_in(a.ix, s, dR + p0);
    while (pos - 1 > FL && pos - E - 1 >= FR && sym_at(a.ix.ref_words, (uint32_t)(pos - 1)) == sym_at(a.ix.ref_words, (uint32_t)(pos - E - 1))) --pos;
    t.v[T_SUPPORTING]++;
    event_insert(a.keys, a.counts, a.log2n, a.tallies + kOverflow, (uint32_t)pos, (uint32_t)E, against);
}

__global__ __launch_bounds__(kDuplicationBlock) void duplication_scan_kernel(DuplicationArgs a) {
    __shared__ uint4 queue_s[kDuplicationBlock / 64][kDuplicationQueue];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* const q = queue_s[wave];
    const uint64_t n = a.rec.n_records_dev ? std::min<uint64_t>(a.rec.n_records, *a.rec.n_records_dev) : a.rec.n_records;
    const uint64_t stride = (uint64_t)gridDim.x * kDuplicationBlock;
    DuplicationTally t;
    uint32_t qn = 0;                                  // records waiting in the wave's queue (the same in every lane)
    for (uint64_t base = (uint64_t)blockIdx.x * kDuplicationBlock + wave * 64u; base < n; base += stride) {
        const uint64_t r = base + lane;
        uint4 work = make_uint4(0u, 0u, 0u, 0u);
        const bool slow = r < n && duplication_anchor(a, (uint32_t)r, t, work);
        const unsigned long long mask = __ballot(slow);
        if (mask == 0ull) continue;
        if (slow) q[qn + lane_prefix(mask)] = work;   // (qn < 64 here and at most 64 arrive: below kDuplicationQueue)
        qn += (uint32_t)__popcll(mask);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the queue is the wave's own: its lanes' stores before its lanes' loads)
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64u) {
            qn -= 64u;
            work = q[qn + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            duplication_walk(a, work, t);
        }
    }
    if (lane < qn) duplication_walk(a, q[lane], t);
#pragma unroll
    for (int i = 0; i < kScanTallies; ++i) {
        const uint32_t sum = wave_total(t.v[i]);
        if (lane == 0 && sum) atomicAdd(a.tallies + i, (unsigned long long)sum);
    }
}

// span[0 .. n) prefix-summed in place by one workgroup (span_prefix_block, bk_anchor.h)
__global__ __launch_bounds__(kSpanPrefixBlock) void duplication_span_prefix_kernel(unsigned int* __restrict__ span, uint32_t n) { span_prefix_block(span, n); }

__global__ __launch_bounds__(kDuplicationBlock) void duplication_report_kernel(DuplicationArgs a) {
    const uint64_t n_slots = 1ull << a.log2n;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kDuplicationBlock + (threadIdx.x & ~63u); base < n_slots; base += (uint64_t)gridDim.x * kDuplicationBlock) {
        const uint64_t i = base + lane;
        bool there = false, pass = false;
        DuplicationRecordDev row{};
        if (i < n_slots) {
            const unsigned long long key = a.keys[i];
            there = key != kEventFreeWord;
            if (there) {
                row.cell = (uint32_t)key; row.len = (uint32_t)(key >> 32);
                row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
                // (lo <= pos - E and pos <= hi <= total_cells: both are entries of span)
                row.span_start = a.span[row.cell - row.len]; row.span_end = a.span[row.cell];
                pass = (unsigned long long)row.fwd + row.rev >= a.min_reads;
            }
        }
        const unsigned long long m_there = __ballot(there), m_pass = __ballot(pass);
        if (m_there == 0ull) continue;
        unsigned long long at = 0ull;
        if (lane == 0) {
            atomicAdd(a.tallies + kCandidates, (unsigned long long)__popcll(m_there));
            if (m_pass) at = atomicAdd(a.tallies + kReported, (unsigned long long)__popcll(m_pass));
        }
        at = __shfl(at, 0);
        if (pass) {
            const uint64_t o = at + lane_prefix(m_pass);
            if (o < a.row_cap) a.rows[o] = row;
        }
    }
}

}  // namespace

void launch_duplication_scan(const DuplicationArgs& a, int n_cus, hipStream_t stream) {
    if (a.rec.n_records == 0) return;
    const uint64_t blocks = (a.rec.n_records + kDuplicationBlock - 1) / kDuplicationBlock;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * 8));
    hipLaunchKernelGGL(duplication_scan_kernel, dim3(grid), dim3(kDuplicationBlock), 0, stream, a);
}

void launch_duplication_span_prefix(const DuplicationArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(duplication_span_prefix_kernel, dim3(1), dim3(kSpanPrefixBlock), 0, stream, a.span, a.ix.total_cells + 2u);
}

void launch_duplication_report(const DuplicationArgs& a, hipStream_t stream) {
    const uint64_t blocks = ((1ull << a.log2n) + kDuplicationBlock - 1) / kDuplicationBlock;
    hipLaunchKernelGGL(duplication_report_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 2048)), dim3(kDuplicationBlock), 0, stream, a);
}

}  // namespace bk
