// bk_copybacks.hip -- strand-switch (copy-back, snap-back) junctions from the reads (bk_copybacks_enable; `bronko call --copybacks`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section B; bronko_amd/host/copybacks.cpp and tests/copybacks_ref.py restate it.
// An event pass (bk_event_pass.h: the scan's queue loop, the span of a record on one diagonal, the report's append); its own are
//   copyback_anchor  both ends' anchors through bk_anchor.h (end_anchors).  On one strand: the record on one diagonal, nothing else.
//                    On two strands with f + k <= g it is the rare record that is walked.
//   copyback_walk    an arm that runs down the reference is a plain diagonal of rc_words, so mismatches / sym_at of bk_anchor.h serve
//                    both arms.  Incremental: moving p by one exchanges one comparison on arm A for one on arm B; the best p by
//                    (m, min(x, y), p); then the two slide loops.  The event goes to bk_anchor.h's one-word table (event_insert), the
//                    key lo | kind << 31 | hi << 32, the two counters of a slot lo_first and hi_first.
//   copyback_decode  a slot as a row: the events with enough reads and distance pass.
// Vector stores and atomics only.
#include "bk_event_pass.h"

namespace bk {
namespace {

typedef EventTally<CopybackArgs::kScanTallies> CopybackTally;
enum { T_RECORDS, T_SAME_STRAND, T_SPANNING, T_SWITCHED, T_SUPPORTING, T_DISCORDANT };

// A record's end anchors and all that needs no breakpoint.  Returns true with `work` filled for a switched record:
// {record | kind << 31, f | g << 16, c_f, c_g}.
__device__ __forceinline__ bool copyback_anchor(const CopybackArgs& a, uint32_t r, CopybackTally& t, uint4& work) {
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    if (n < k) return false;                          // (trimmed away: no record any more)
    t.v[T_RECORDS]++;
    if (n < 2 * k) return false;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    EndAnchors e;
    if (!end_anchors(a.ix, w, n, e)) return false;
    if (e.f_ag != e.b_ag) {
        if (e.f_off + k > e.b_off) return false;
        t.v[T_SWITCHED]++;
        work = make_uint4(r | (e.f_ag ? 0x80000000u : 0u), (uint32_t)e.f_off | ((uint32_t)e.b_off << 16), e.f_cell, e.b_cell);
        return true;
    }
    Anchors an;
    if (!anchors_of(e, k, n, an)) return false;
    t.v[T_SAME_STRAND]++;
    const int32_t dL = (int32_t)an.ca - an.pa, dR = (int32_t)an.cb - an.pb;
    if (!cells_placed(a.ix, an.ca, an.cb, min(dL, dR), max(dL, dR) + n)) return false;
    if (dL != dR) return false;
    if (ref_span_count(a.ix, w, n, an, dL, a.max_mismatches, a.span)) t.v[T_SPANNING]++;
    return false;
}

// a switched record: the arms' cells, the breakpoint, the normalised event, the table
__device__ __forceinline__ void copyback_walk(const CopybackArgs& a, const uint4 work, CopybackTally& t) {
    const uint32_t r = work.x & 0x7fffffffu, kind = work.x >> 31;
    const int32_t f = (int32_t)(work.y & 0xffffu), g = (int32_t)(work.y >> 16), cf = (int32_t)work.z, cg = (int32_t)work.w;
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r], total = (int32_t)a.ix.total_cells;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const uint32_t* __restrict__ ref = a.ix.ref_words;
    // the base expected at offset j: arm A text_a[d_a + j], arm B text_b[d_b + j] (an arm that runs down the reference: rc_words at the
    // mirrored cell); the breakpoint's cells x(p) = x0 + sx * p, y(p) = y0 - sx * p
    const bool is_h = kind == 0u;
    const uint32_t* __restrict__ text_a = is_h ? ref : a.ix.rc_words;
    const uint32_t* __restrict__ text_b = is_h ? a.ix.rc_words : ref;
    const int32_t d_a = is_h ? cf - f : total - 1 - (cf + k - 1 + f), d_b = is_h ? total - 1 - (cg + k - 1 + g) : cg - g;
    const int32_t sx = is_h ? 1 : -1;
    const int32_t x0 = is_h ? cf - f - 1 : cf + k + f, y0 = is_h ? cg + k - 1 + g : cg - g;
    // ignored: the anchors in two sequences; an arm's cells -- A's offsets [0, g), B's [f + k, n) -- outside the sequence or not ACGT
    const uint32_t s = seq_of(a.ix, (uint32_t)cf);
    if (seq_of(a.ix, (uint32_t)cg) != s) return;
    const int32_t xa = x0 + sx, xb = x0 + sx * g, ya = y0 - sx * (f + k), yb = y0 - sx * (n - 1);
    if (!arm_placed(a.ix, s, min(xa, xb), max(xa, xb) + 1) || !arm_placed(a.ix, s, min(ya, yb), max(ya, yb) + 1)) return;
    const int32_t p0 = f + k;                         // (p0 <= g: copyback_anchor)
    int32_t m = (int32_t)(mismatches(w, last_word, 0u, (uint32_t)p0, text_a, d_a, ~0u) + mismatches(w, last_word, (uint32_t)p0, (uint32_t)n, text_b, d_b, ~0u));
    int32_t best = m, best_p = p0, best_low = min(x0 + sx * p0, y0 - sx * p0);
    for (int32_t p = p0; p < g; ++p) {
        const uint32_t base = sym_at(w, (uint32_t)p);
        m += (base != sym_at(text_a, (uint32_t)(d_a + p)) ? 1 : 0) - (base != sym_at(text_b, (uint32_t)(d_b + p)) ? 1 : 0);
        const int32_t low = min(x0 + sx * (p + 1), y0 - sx * (p + 1));
        if (m < best || (m == best && low < best_low)) { best = m; best_low = low; best_p = p + 1; }
    }
    if (best > (int32_t)a.max_mismatches) { t.v[T_DISCORDANT]++; return; }
    t.v[T_SUPPORTING]++;
    const int32_t x = x0 + sx * best_p, y = y0 - sx * best_p;
    // the run of pairs (x + t, y - t): the step up from t compares the cells x + t + e and y - t - 1 + e, e = 1 for H, 0 for T
    int32_t x_lo, x_hi, y_lo, y_hi;
    acgt_stretch(a.ix, s, x, x_lo, x_hi);
    acgt_stretch(a.ix, s, y, y_lo, y_hi);
    const int32_t e = is_h ? 1 : 0;
    int32_t t1 = 0, t0 = 0;
    while (x + t1 + 1 < x_hi && y - t1 - 1 >= y_lo && sym_at(ref, (uint32_t)(x + t1 + e)) == 3u - sym_at(ref, (uint32_t)(y - t1 - 1 + e))) ++t1;
    while (x + t0 - 1 >= x_lo && y - t0 + 1 < y_hi && sym_at(ref, (uint32_t)(x + t0 - 1 + e)) == 3u - sym_at(ref, (uint32_t)(y - t0 + e))) --t0;
    const bool low_end = x + t0 <= y - t1;            // the extreme pair whose smaller cell is smaller
    const int32_t lo = low_end ? x + t0 : y - t1, hi = low_end ? y - t0 : x + t1;
    event_insert(a.keys, a.counts, a.log2n, a.tallies + CopybackArgs::kOverflow, (uint32_t)lo | (kind << 31), (uint32_t)hi, x > y);
}

__device__ __forceinline__ bool copyback_decode(const CopybackArgs& a, uint64_t i, CopybackRecordDev& row, bool& pass) {
    const unsigned long long key = a.keys[i];
    if (key == kEventFreeWord) return false;
    row.lo = (uint32_t)key & 0x7fffffffu; row.hi = (uint32_t)(key >> 32); row.kind = ((uint32_t)key) >> 31;
    row.lo_first = a.counts[2u * i]; row.hi_first = a.counts[2u * i + 1u];
    const uint32_t off = row.kind == 0u ? 1u : 0u;   // (hi + 1 <= total_cells: span holds total_cells + 2)
    row.span_lo = a.span[row.lo + off]; row.span_hi = a.span[row.hi + off];
    pass = (unsigned long long)row.lo_first + row.hi_first >= a.min_reads && row.hi - row.lo >= a.min_dist;
    return true;
}

__global__ __launch_bounds__(kEventBlock) void copyback_scan_kernel(CopybackArgs a) { event_scan<CopybackArgs, copyback_anchor, copyback_walk>(a); }
__global__ __launch_bounds__(kEventBlock) void copyback_report_kernel(CopybackArgs a) { event_report<CopybackArgs, CopybackRecordDev, copyback_decode>(a); }

}  // namespace

void launch_copyback_scan(const CopybackArgs& a, int n_cus, hipStream_t stream) { launch_event_scan(copyback_scan_kernel, a, n_cus, stream); }
void launch_copyback_report(const CopybackArgs& a, hipStream_t stream) { launch_event_report(copyback_report_kernel, a, stream); }

}  // namespace bk
