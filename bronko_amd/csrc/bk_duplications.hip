// bk_duplications.hip -- tandem duplications and the origin of a circular genome from the reads (bk_duplications_enable; `bronko call --duplications`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section V; bronko_amd/host/duplications.cpp and tests/duplications_ref.py restate it.
// An event pass (bk_event_pass.h: the scan's queue loop, the span of a record on one diagonal, the report's append); its own are
//   duplication_anchor  the anchors through bk_anchor.h; delta = 0 is the record on one diagonal, `forward` and `short` a tally each;
//                       a backward jump of min_len or more is the rare record that is walked.  What differs from the junction is
//                       asked here, before the queue: each arm against the sequence's borders and the runs of other letters on its
//                       own, and the breakpoint's range clipped to the sequence, so that an arm may end at the sequence's last cell
//                       or begin at its first.
//   duplication_walk    the breakpoint (breakpoint_walk), the event slid down between its two floors, the table (event_insert, key
//                       pos | E << 32): bk_anchor.h's, shared with junction_walk.
//   duplication_decode  a slot as a row: the events with enough reads pass.
// Vector stores and atomics only.
#include "bk_event_pass.h"

namespace bk {
namespace {

typedef EventTally<DuplicationArgs::kScanTallies> DuplicationTally;
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
        if (ref_span_count(a.ix, w, n, an, dL, a.max_mismatches, a.span)) t.v[T_SPANNING]++; else t.v[T_DISCORDANT]++;
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
    event_insert(a.keys, a.counts, a.log2n, a.tallies + DuplicationArgs::kOverflow, (uint32_t)pos, (uint32_t)E, against);
}

__device__ __forceinline__ bool duplication_decode(const DuplicationArgs& a, uint64_t i, DuplicationRecordDev& row, bool& pass) {
    const unsigned long long key = a.keys[i];
    if (key == kEventFreeWord) return false;
    row.cell = (uint32_t)key; row.len = (uint32_t)(key >> 32);
    row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
    // (lo <= pos - E and pos <= hi <= total_cells: both are entries of span)
    row.span_start = a.span[row.cell - row.len]; row.span_end = a.span[row.cell];
    pass = (unsigned long long)row.fwd + row.rev >= a.min_reads;
    return true;
}

__global__ __launch_bounds__(kEventBlock) void duplication_scan_kernel(DuplicationArgs a) { event_scan<DuplicationArgs, duplication_anchor, duplication_walk>(a); }
__global__ __launch_bounds__(kEventBlock) void duplication_report_kernel(DuplicationArgs a) { event_report<DuplicationArgs, DuplicationRecordDev, duplication_decode>(a); }

}  // namespace

void launch_duplication_scan(const DuplicationArgs& a, int n_cus, hipStream_t stream) { launch_event_scan(duplication_scan_kernel, a, n_cus, stream); }
void launch_duplication_report(const DuplicationArgs& a, hipStream_t stream) { launch_event_report(duplication_report_kernel, a, stream); }

}  // namespace bk
