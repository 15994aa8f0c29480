// bk_junctions.hip -- long deletions and subgenomic-RNA junctions from the reads (bk_junctions_enable; `bronko call --junctions`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section J; bronko_amd/host/junctions.cpp and tests/junctions_ref.py restate it.
// An event pass (bk_event_pass.h: the scan's queue loop, the span of a record on one diagonal, the report's append); its own are
//   junction_anchor  the anchors through bk_anchor.h; delta = 0 is the record on one diagonal, `short` and `backward` a tally each;
//                    a forward jump of min_len or more is the rare record that is walked.
//   junction_walk    the breakpoint (breakpoint_walk), the event slid down to its first cell, the table (event_insert, key
//                    pos | D << 32): bk_anchor.h's, shared with duplication_walk.
//   junction_decode  a slot as a row: the events with enough reads pass.
// Vector stores and atomics only.
#include "bk_event_pass.h"

namespace bk {
namespace {

typedef EventTally<JunctionArgs::kScanTallies> JunctionTally;
enum { T_RECORDS, T_ANCHORED, T_SPANNING, T_SUPPORTING, T_SHORT, T_BACKWARD, T_DISCORDANT };

// A record's anchors and all that needs no breakpoint.  Returns true with `work` filled for a record with delta >= min_len that
// passed the checks: {record | against << 31, a | b << 16, dL, dR}.
__device__ __forceinline__ bool junction_anchor(const JunctionArgs& a, uint32_t r, JunctionTally& t, uint4& work) {
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
    if (!cells_placed(a.ix, an.ca, an.cb, min(dL, dR), max(dL, dR) + n)) return false;
    if (delta == 0) {
        if (ref_span_count(a.ix, w, n, an, dL, a.max_mismatches, a.span)) t.v[T_SPANNING]++; else t.v[T_DISCORDANT]++;
        return false;
    }
    if (delta < (int32_t)a.min_len && -delta < (int32_t)a.min_len) { t.v[T_SHORT]++; return false; }
    if (delta < 0) { t.v[T_BACKWARD]++; return false; }
    work = make_uint4(r | (against ? 0x80000000u : 0u), (uint32_t)pa | ((uint32_t)pb << 16), (uint32_t)dL, (uint32_t)dR);
    return true;
}

// delta >= min_len: the breakpoint, the normalised event, the table
__device__ __forceinline__ void junction_walk(const JunctionArgs& a, const uint4 work, JunctionTally& t) {
    const uint32_t r = work.x & 0x7fffffffu;
    const bool against = (work.x >> 31) != 0u;
    const int32_t pa = (int32_t)(work.y & 0xffffu), pb = (int32_t)(work.y >> 16), dL = (int32_t)work.z, dR = (int32_t)work.w;
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r], D = dR - dL;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const OrientedRecord rec{a.ix, w, n, last_word, against};
    int32_t best_p;
    const int32_t best = breakpoint_walk(rec, pa + k, pb, dL, dR, best_p);   // (pa + k <= pb: anchors_of)
    if (best > (int32_t)a.max_mismatches) { t.v[T_DISCORDANT]++; return; }
    int32_t pos = dL + best_p;
    // F: the first cell of the stretch of ACGT letters of the sequence that holds pos - 1 (the record's cells [dL, dR + n) hold no other letter)
    const int32_t F = acgt_floor(a.ix, (uint32_t)(dL + pa), dL);
    while (pos - 1 > F && sym_at(a.ix.ref_words, (uint32_t)(pos - 1)) == sym_at(a.ix.ref_words, (uint32_t)(pos + D - 1))) --pos;
    t.v[T_SUPPORTING]++;
    event_insert(a.keys, a.counts, a.log2n, a.tallies + JunctionArgs::kOverflow, (uint32_t)pos, (uint32_t)D, against);
}

__device__ __forceinline__ bool junction_decode(const JunctionArgs& a, uint64_t i, JunctionRecordDev& row, bool& pass) {
    const unsigned long long key = a.keys[i];
    if (key == kEventFreeWord) return false;
    row.cell = (uint32_t)key; row.len = (uint32_t)(key >> 32);
    row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
    row.span_donor = a.span[row.cell]; row.span_acceptor = a.span[row.cell + row.len];   // (pos + D lies inside the record's cells)
    pass = (unsigned long long)row.fwd + row.rev >= a.min_reads;
    return true;
}

__global__ __launch_bounds__(kEventBlock) void junction_scan_kernel(JunctionArgs a) { event_scan<JunctionArgs, junction_anchor, junction_walk>(a); }
__global__ __launch_bounds__(kEventBlock) void junction_report_kernel(JunctionArgs a) { event_report<JunctionArgs, JunctionRecordDev, junction_decode>(a); }

}  // namespace

void launch_junction_scan(const JunctionArgs& a, int n_cus, hipStream_t stream) { launch_event_scan(junction_scan_kernel, a, n_cus, stream); }
void launch_junction_report(const JunctionArgs& a, hipStream_t stream) { launch_event_report(junction_report_kernel, a, stream); }

}  // namespace bk
