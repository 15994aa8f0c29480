// bk_chimeras.hip -- junctions between two sequences of the genome file from the reads (bk_chimeras_enable; `bronko call --chimeras`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section X; bronko_amd/host/chimeras.cpp and tests/chimeras_ref.py restate it.
// An event pass (bk_event_pass.h: the scan's queue loop, the span of a record on one diagonal, the report's append); its own are
//   chimera_anchor  both ends' anchors through bk_anchor.h (end_anchors) and the sequence of each.  In one sequence and on one strand:
//                   the record on one diagonal, nothing else.  In two sequences with f + k <= g it is the rare record that is walked.
//   chimera_walk    an arm that runs down the reference is a plain diagonal of rc_words, so mismatches / sym_at of bk_anchor.h serve
//                   all four orientations; each arm is held to its own sequence.  Incremental: moving p by one exchanges one
//                   comparison on arm A for one on arm B; the best p by (m, min(x, y)); then the two slide loops, each cell inside
//                   its own sequence's stretch of ACGT.  The event goes to bk_anchor.h's one-word table (event_insert), the key
//                   lo | sides << 28 | hi << 32, the two counters of a slot lo_first and hi_first.
//   chimera_decode  a slot as a row: the events with enough reads pass.
// Vector stores and atomics only.
#include "bk_event_pass.h"

namespace bk {
namespace {

typedef EventTally<ChimeraArgs::kScanTallies> ChimeraTally;
enum { T_RECORDS, T_SAME_STRAND, T_SPANNING, T_CROSSED, T_SUPPORTING, T_DISCORDANT };

// A record's end anchors and all that needs no breakpoint.  Returns true with `work` filled for a crossed record:
// {record | s_f << 31, f | s_g << 15 | g << 16, c_f, c_g}.
__device__ __forceinline__ bool chimera_anchor(const ChimeraArgs& a, uint32_t r, ChimeraTally& t, uint4& work) {
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    if (n < k) return false;                          // (trimmed away: no record any more)
    t.v[T_RECORDS]++;
    if (n < 2 * k) return false;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    EndAnchors e;
    if (!end_anchors(a.ix, w, n, e)) return false;
    const uint32_t s = seq_of(a.ix, e.f_cell);
    if (seq_of(a.ix, e.b_cell) != s) {
        if (e.f_off + k > e.b_off) return false;
        t.v[T_CROSSED]++;
        work = make_uint4(r | (e.f_ag ? 0x80000000u : 0u), (uint32_t)e.f_off | (e.b_ag ? 0x8000u : 0u) | ((uint32_t)e.b_off << 16), e.f_cell, e.b_cell);
        return true;
    }
    Anchors an;
    if (!anchors_of(e, k, n, an)) return false;       // (on two strands of one sequence: bk_copybacks_enable's)
    t.v[T_SAME_STRAND]++;
    const int32_t dL = (int32_t)an.ca - an.pa, dR = (int32_t)an.cb - an.pb;
    if (!arm_placed(a.ix, s, min(dL, dR), max(dL, dR) + n)) return false;
    if (dL != dR) return false;
    if (ref_span_count(a.ix, w, n, an, dL, a.max_mismatches, a.span)) t.v[T_SPANNING]++;
    return false;
}

// a crossed record: the arms' cells, the breakpoint, the normalised event, the table
__device__ __forceinline__ void chimera_walk(const ChimeraArgs& a, const uint4 work, ChimeraTally& t) {
    const uint32_t r = work.x & 0x7fffffffu;
    const bool a_ag = (work.x >> 31) != 0u, b_ag = (work.y & 0x8000u) != 0u;
    const int32_t f = (int32_t)(work.y & 0x7fffu), g = (int32_t)(work.y >> 16), cf = (int32_t)work.z, cg = (int32_t)work.w;
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r], total = (int32_t)a.ix.total_cells;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const uint32_t* __restrict__ ref = a.ix.ref_words;
    // the base expected at offset j: arm A text_a[d_a + j], arm B text_b[d_b + j] (an arm that runs down the reference: rc_words at the
    // mirrored cell); the breakpoint's cells x(p) = A(p - 1) = x0 + sa * p, y(p) = B(p) = y0 + sb * p
    const uint32_t* __restrict__ text_a = a_ag ? a.ix.rc_words : ref;
    const uint32_t* __restrict__ text_b = b_ag ? a.ix.rc_words : ref;
    const int32_t d_a = a_ag ? total - 1 - (cf + k - 1 + f) : cf - f, d_b = b_ag ? total - 1 - (cg + k - 1 + g) : cg - g;
    const int32_t sa = a_ag ? -1 : 1, sb = b_ag ? -1 : 1;
    const int32_t x0 = a_ag ? cf + k + f : cf - f - 1, y0 = b_ag ? cg + k - 1 + g : cg - g;
    // ignored: an arm's cells -- A's offsets [0, g), B's [f + k, n) -- outside the arm's own sequence or not ACGT
    const uint32_t s_x = seq_of(a.ix, (uint32_t)cf), s_y = seq_of(a.ix, (uint32_t)cg);
    const int32_t xa = x0 + sa, xb = x0 + sa * g, ya = y0 + sb * (f + k), yb = y0 + sb * (n - 1);
    if (!arm_placed(a.ix, s_x, min(xa, xb), max(xa, xb) + 1) || !arm_placed(a.ix, s_y, min(ya, yb), max(ya, yb) + 1)) return;
    const int32_t p0 = f + k;                         // (p0 <= g: chimera_anchor)
    int32_t m = (int32_t)(mismatches(w, last_word, 0u, (uint32_t)p0, text_a, d_a, ~0u) + mismatches(w, last_word, (uint32_t)p0, (uint32_t)n, text_b, d_b, ~0u));
    int32_t best = m, best_p = p0, best_low = min(x0 + sa * p0, y0 + sb * p0);
    for (int32_t p = p0; p < g; ++p) {
        const uint32_t base = sym_at(w, (uint32_t)p);
        m += (base != sym_at(text_a, (uint32_t)(d_a + p)) ? 1 : 0) - (base != sym_at(text_b, (uint32_t)(d_b + p)) ? 1 : 0);
        const int32_t low = min(x0 + sa * (p + 1), y0 + sb * (p + 1));
        if (m < best || (m == best && low < best_low)) { best = m; best_low = low; best_p = p + 1; }
    }
    if (best > (int32_t)a.max_mismatches) { t.v[T_DISCORDANT]++; return; }
    t.v[T_SUPPORTING]++;
    const int32_t x = x0 + sa * best_p, y = y0 + sb * best_p;
    // the run of pairs (x + sa t, y + sb t): the step up from t compares what arm A shows of the cell x + sa (t + 1) with what arm B
    // shows of the cell y + sb t; every cell inside its own sequence's stretch of ACGT
    int32_t x_lo, x_hi, y_lo, y_hi;
    acgt_stretch(a.ix, s_x, x, x_lo, x_hi);
    acgt_stretch(a.ix, s_y, y, y_lo, y_hi);
    const uint32_t flip = (a_ag != b_ag) ? 3u : 0u;   // (the two arms on two strands: one shows the complement)
    int32_t t1 = 0, t0 = 0;
    for (;;) {
        const int32_t u = x + sa * (t1 + 1), v = y + sb * (t1 + 1);
        if (u < x_lo || u >= x_hi || v < y_lo || v >= y_hi) break;
        if (sym_at(ref, (uint32_t)u) != (flip ^ sym_at(ref, (uint32_t)(v - sb)))) break;
        ++t1;
    }
    for (;;) {
        const int32_t u = x + sa * (t0 - 1), v = y + sb * (t0 - 1);
        if (u < x_lo || u >= x_hi || v < y_lo || v >= y_hi) break;
        if (sym_at(ref, (uint32_t)(u + sa)) != (flip ^ sym_at(ref, (uint32_t)v))) break;
        --t0;
    }
    // the extreme pair whose smaller cell is smaller: the lower sequence's cell decides, the arm there along the reference: t0
    const bool a_low = x < y;
    const int32_t te = (a_low ? sa : sb) > 0 ? t0 : t1;
    const int32_t ex = x + sa * te, ey = y + sb * te;
    const uint32_t side_x = a_ag ? 1u : 0u, side_y = b_ag ? 0u : 1u;   // 1 = R: the read holds the cell and the cells above it
    const uint32_t lo = (uint32_t)(a_low ? ex : ey), hi = (uint32_t)(a_low ? ey : ex);
    const uint32_t sides = a_low ? side_x | (side_y << 1) : side_y | (side_x << 1);
    event_insert(a.keys, a.counts, a.log2n, a.tallies + ChimeraArgs::kOverflow, lo | (sides << 28), hi, !a_low);
}

__device__ __forceinline__ bool chimera_decode(const ChimeraArgs& a, uint64_t i, ChimeraRecordDev& row, bool& pass) {
    const unsigned long long key = a.keys[i];
    if (key == kEventFreeWord) return false;
    row.lo = (uint32_t)key & 0x07ffffffu; row.hi = (uint32_t)(key >> 32); row.sides = ((uint32_t)key >> 28) & 3u;
    row.lo_first = a.counts[2u * i]; row.hi_first = a.counts[2u * i + 1u];
    // side L: the records that hold the cell and the one above it; (hi + 1 <= total_cells: span holds total_cells + 2)
    row.span_lo = a.span[row.lo + ((row.sides & 1u) ? 0u : 1u)]; row.span_hi = a.span[row.hi + ((row.sides & 2u) ? 0u : 1u)];
    pass = (unsigned long long)row.lo_first + row.hi_first >= a.min_reads;
    return true;
}

__global__ __launch_bounds__(kEventBlock) void chimera_scan_kernel(ChimeraArgs a) { event_scan<ChimeraArgs, chimera_anchor, chimera_walk>(a); }
__global__ __launch_bounds__(kEventBlock) void chimera_report_kernel(ChimeraArgs a) { event_report<ChimeraArgs, ChimeraRecordDev, chimera_decode>(a); }

}  // namespace

void launch_chimera_scan(const ChimeraArgs& a, int n_cus, hipStream_t stream) { launch_event_scan(chimera_scan_kernel, a, n_cus, stream); }
void launch_chimera_report(const ChimeraArgs& a, hipStream_t stream) { launch_event_report(chimera_report_kernel, a, stream); }

}  // namespace bk
