// bk_breakends.hip -- reads that leave the reference: records with an anchor at one end only (bk_breakends_enable; `bronko call --breakends`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section E; bronko_amd/host/breakends.cpp and tests/breakends_ref.py restate it.
// An event pass (bk_event_pass.h: the scan's queue loop, the span of a record on one diagonal, the report's append); its own are
//   breakend_anchor  both ends' anchors through bk_anchor.h (end_anchors_both).  Two anchors: the record on one diagonal, nothing
//                    else.  One anchor is the rare record that is walked.
//   breakend_walk    extends the anchor base by base along its diagonal (OrientedRecord: no record is reverse-complemented), +1 a
//                    match, -BK_BREAKEND_MISMATCH_PENALTY a mismatch, inside the anchor's stretch of ACGT letters of its own
//                    sequence; the held part's Hamming distance, the clip, the tag (one 16-base window of the record's words, turned
//                    for a record against the reference), the event (bk_anchor.h's event_insert, key cell | side << 27 | tag << 32)
//                    and one add on the (cell, side) array.
//   breakend_decode  a slot as a row: the events with enough reads pass.
// Vector stores and atomics only.
#include "bk_event_pass.h"

namespace bk {
namespace {

constexpr int32_t kMismatchPenalty = BK_BREAKEND_MISMATCH_PENALTY;

typedef EventTally<BreakendArgs::kScanTallies> BreakendTally;
enum { T_RECORDS, T_ONE_ANCHOR, T_SPANNING, T_SUPPORTING, T_SHORT, T_THROUGH, T_DISCORDANT, T_UNPLACED };

// A record's end anchors and all that needs no walk.  Returns true with `work` filled for a record with exactly one anchor:
// {record | against << 31, a | side << 16, cell, 0}; a the anchor's offset in r', side 1 = R.
__device__ __forceinline__ bool breakend_anchor(const BreakendArgs& a, uint32_t r, BreakendTally& t, uint4& work) {
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    if (n < k) return false;                          // (trimmed away: no record any more)
    t.v[T_RECORDS]++;
    if (n < 2 * k) return false;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    EndAnchors e;
    const uint32_t ends = end_anchors_both(a.ix, w, n, e);
    if (ends == 0u) return false;
    if (ends == 3u) {                                 // two anchors: only what the span needs, as junction_anchor has it
        Anchors an;
        if (!anchors_of(e, k, n, an)) return false;
        const int32_t dL = (int32_t)an.ca - an.pa, dR = (int32_t)an.cb - an.pb;
        if (!cells_placed(a.ix, an.ca, an.cb, min(dL, dR), max(dL, dR) + n)) return false;
        if (dL != dR) return false;
        if (ref_span_count(a.ix, w, n, an, dL, a.max_mismatches, a.span)) t.v[T_SPANNING]++;
        return false;
    }
    t.v[T_ONE_ANCHOR]++;
    const bool front = ends == 1u;
    const bool against = front ? e.f_ag : e.b_ag;
    const int32_t off = front ? e.f_off : e.b_off;
    const int32_t pa = against ? n - k - off : off;   // the anchor's offset in r'
    const uint32_t side = front != against ? 0u : 1u; // L: the front anchor along the reference, or the back anchor against it
    work = make_uint4(r | (against ? 0x80000000u : 0u), (uint32_t)pa | (side << 16), front ? e.f_cell : e.b_cell, 0u);
    return true;
}

// one anchor: the stretch, the extension, the held part, the clip, the event
__device__ __forceinline__ void breakend_walk(const BreakendArgs& a, const uint4 work, BreakendTally& t) {
    const uint32_t r = work.x & 0x7fffffffu;
    const bool against = (work.x >> 31) != 0u;
    const int32_t pa = (int32_t)(work.y & 0xffffu), c = (int32_t)work.z;
    const uint32_t side = work.y >> 16;
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const OrientedRecord rec{a.ix, w, n, last_word, against};
    // [lo, hi): the stretch of ACGT letters of the anchor's sequence around its first cell (one that holds another letter: hi <= c)
    int32_t lo, hi;
    acgt_stretch(a.ix, seq_of(a.ix, (uint32_t)c), c, lo, hi);
    const int32_t d = c - pa;
    if (c < lo || c + k > hi || (side == 0u ? d < lo : d + n > hi)) { t.v[T_UNPLACED]++; return; }
    // every cell read from here on lies in [lo, hi): side L reads r'[0, P) at d + j >= d >= lo, side R r'[Q, n) at d + j < d + n <= hi
    int32_t S = 0, best = 0, edge, m;
    if (side == 0u) {
        const int32_t P = min(n, hi - d);
        edge = pa + k;                                // p*: the smallest p with the largest S
        for (int32_t p = pa + k; p < P; ++p) {
            S += rec.mm(p, d) ? -kMismatchPenalty : 1;
            if (S > best) { best = S; edge = p + 1; }
        }
        m = rec.span_mm(0, edge, d);
    } else {
        const int32_t Q = max(0, lo - d);
        edge = pa;                                    // q*: the largest q with the largest S
        for (int32_t q = pa - 1; q >= Q; --q) {
            S += rec.mm(q, d) ? -kMismatchPenalty : 1;
            if (S > best) { best = S; edge = q; }
        }
        m = rec.span_mm(edge, n, d);
    }
    if (m > (int32_t)a.max_mismatches) { t.v[T_DISCORDANT]++; return; }
    const int32_t clip = side == 0u ? n - edge : edge;
    if (clip == 0) { t.v[T_THROUGH]++; return; }
    if (clip < (int32_t)a.min_clip) { t.v[T_SHORT]++; return; }
    t.v[T_SUPPORTING]++;
    // the tag r'[at, at + 16) (min_clip >= 16: inside the record): one window of the record's words; of a record against the
    // reference the mirrored window, its bases complemented and in reverse order
    const int32_t at = side == 0u ? edge : edge - 16;
    const uint32_t tag = against ? ~rev2_32(sym16_at(w, (uint32_t)(n - at - 16), last_word)) : sym16_at(w, (uint32_t)at, last_word);
    const uint32_t cell = (uint32_t)(side == 0u ? d + edge - 1 : d + edge);
    event_insert(a.keys, a.counts, a.log2n, a.tallies + BreakendArgs::kOverflow, cell | (side << 27), tag, against);
    atomicAdd(a.more.site + 2u * cell + side, 1u);
}

__device__ __forceinline__ bool breakend_decode(const BreakendArgs& a, uint64_t i, BreakendRecordDev& row, bool& pass) {
    const unsigned long long key = a.keys[i];
    if (key == kEventFreeWord) return false;
    row.cell = (uint32_t)key & 0x07ffffffu; row.side = ((uint32_t)key >> 27) & 1u; row.tag = (uint32_t)(key >> 32);
    row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
    row.site_reads = a.more.site[2u * row.cell + row.side];
    // side L: the records that hold the cell and the one above it; (cell + 1 <= total_cells: span holds total_cells + 2)
    row.span = a.span[row.cell + (row.side ? 0u : 1u)];
    pass = (unsigned long long)row.fwd + row.rev >= a.min_reads;
    return true;
}

__global__ __launch_bounds__(kEventBlock) void breakend_scan_kernel(BreakendArgs a) { event_scan<BreakendArgs, breakend_anchor, breakend_walk>(a); }
__global__ __launch_bounds__(kEventBlock) void breakend_report_kernel(BreakendArgs a) { event_report<BreakendArgs, BreakendRecordDev, breakend_decode>(a); }

}  // namespace

void launch_breakend_scan(const BreakendArgs& a, int n_cus, hipStream_t stream) { launch_event_scan(breakend_scan_kernel, a, n_cus, stream); }
void launch_breakend_report(const BreakendArgs& a, hipStream_t stream) { launch_event_report(breakend_report_kernel, a, stream); }

}  // namespace bk
