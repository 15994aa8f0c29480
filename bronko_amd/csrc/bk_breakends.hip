// bk_breakends.hip -- reads that leave the reference: records with an anchor at one end only (bk_breakends_enable; `bronko call --breakends`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section E; bronko_amd/host/breakends.cpp and tests/breakends_ref.py restate it.
//   breakend_scan_kernel         behind the scan of the same records, a lane per record, shaped as junction_scan_kernel (bk_junctions.hip):
//                                both ends' anchors through bk_anchor.h (end_anchors_both).  Two anchors: delta = 0 inline (the Hamming
//                                pass with an early exit, two atomics on `span`), nothing else.  One anchor is rare: those records are
//                                gathered in a queue of the wave (LDS, filled through a ballot) and walked a lane each once 64 wait.
//                                The walk extends the anchor base by base along its diagonal (OrientedRecord: no record is
//                                reverse-complemented), +1 a match, -BK_BREAKEND_MISMATCH_PENALTY a mismatch, inside the anchor's
//                                stretch of ACGT letters of its own sequence; the held part's Hamming distance, the clip, the tag (one
//                                16-base window of the record's words, turned for a record against the reference), the event
//                                (event_insert, key cell | side << 27 | tag << 32) and one add on the (cell, side) array.  The sample's
//                                tallies: one add per wave and tally.
//   breakend_span_prefix_kernel  at the sample's end: `span` prefix-summed in place by one workgroup.
//   breakend_report_kernel       the table's events with enough reads, appended with one returning add per wave.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kBreakendBlock = 256;
constexpr uint32_t kBreakendQueue = 128;   // entries of a wave's queue: fewer than 64 wait when up to 64 more arrive
constexpr int kScanTallies = 8;            // records, one_anchor, ref_spanning, supporting, short, through, discordant, unplaced
constexpr int kCandidates = 8, kReported = 9, kOverflow = 10;   // BreakendArgs::tallies behind them
constexpr int32_t kMismatchPenalty = BK_BREAKEND_MISMATCH_PENALTY;

struct BreakendTally { uint32_t v[kScanTallies] = {0, 0, 0, 0, 0, 0, 0, 0}; };
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
    if (ends == 3u) {                                 // two anchors: only what the span needs, as junction_scan_kernel has it
        Anchors an;
        if (!anchors_of(e, k, n, an)) return false;
        const int32_t dL = (int32_t)an.ca - an.pa, dR = (int32_t)an.cb - an.pb;
        if (!cells_placed(a.ix, an.ca, an.cb, min(dL, dR), max(dL, dR) + n)) return false;
        if (dL != dR) return false;
        const uint32_t last_word = (uint32_t)(n - 1) >> 4;
        const uint32_t m = an.against ? mismatches(w, last_word, 0u, (uint32_t)n, a.ix.rc_words, (int64_t)a.ix.total_cells - dL - n, a.max_mismatches)
                                      : mismatches(w, last_word, 0u, (uint32_t)n, a.ix.ref_words, dL, a.max_mismatches);
        if (m > a.max_mismatches) return false;
        t.v[T_SPANNING]++;
        atomicAdd(a.span + (dL + an.pa + k), 1u);
        atomicAdd(a.span + (dL + an.pb + 1), 0xffffffffu);
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
    event_insert(a.keys, a.counts, a.log2n, a.tallies + kOverflow, cell | (side << 27), tag, against);
    atomicAdd(a.site + 2u * cell + side, 1u);
}

__global__ __launch_bounds__(kBreakendBlock) void breakend_scan_kernel(BreakendArgs a) {
    __shared__ uint4 queue_s[kBreakendBlock / 64][kBreakendQueue];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* const q = queue_s[wave];
    const uint64_t n = a.rec.n_records_dev ? std::min<uint64_t>(a.rec.n_records, *a.rec.n_records_dev) : a.rec.n_records;
    const uint64_t stride = (uint64_t)gridDim.x * kBreakendBlock;
    BreakendTally t;
    uint32_t qn = 0;                                  // records waiting in the wave's queue (the same in every lane)
    for (uint64_t base = (uint64_t)blockIdx.x * kBreakendBlock + wave * 64u; base < n; base += stride) {
        const uint64_t r = base + lane;
        uint4 work = make_uint4(0u, 0u, 0u, 0u);
        const bool slow = r < n && breakend_anchor(a, (uint32_t)r, t, work);
        const unsigned long long mask = __ballot(slow);
        if (mask == 0ull) continue;
        if (slow) q[qn + lane_prefix(mask)] = work;   // (qn < 64 here and at most 64 arrive: below kBreakendQueue)
        qn += (uint32_t)__popcll(mask);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the queue is the wave's own: its lanes' stores before its lanes' loads)
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64u) {
            qn -= 64u;
            work = q[qn + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            breakend_walk(a, work, t);
        }
    }
    if (lane < qn) breakend_walk(a, q[lane], t);
#pragma unroll
    for (int i = 0; i < kScanTallies; ++i) {
        const uint32_t sum = wave_total(t.v[i]);
        if (lane == 0 && sum) atomicAdd(a.tallies + i, (unsigned long long)sum);
    }
}

// span[0 .. n) prefix-summed in place by one workgroup (span_prefix_block, bk_anchor.h)
__global__ __launch_bounds__(kSpanPrefixBlock) void breakend_span_prefix_kernel(unsigned int* __restrict__ span, uint32_t n) { span_prefix_block(span, n); }

__global__ __launch_bounds__(kBreakendBlock) void breakend_report_kernel(BreakendArgs a) {
    const uint64_t n_slots = 1ull << a.log2n;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kBreakendBlock + (threadIdx.x & ~63u); base < n_slots; base += (uint64_t)gridDim.x * kBreakendBlock) {
        const uint64_t i = base + lane;
        bool there = false, pass = false;
        BreakendRecordDev row{};
        if (i < n_slots) {
            const unsigned long long key = a.keys[i];
            there = key != kEventFreeWord;
            if (there) {
                row.cell = (uint32_t)key & 0x07ffffffu; row.side = ((uint32_t)key >> 27) & 1u; row.tag = (uint32_t)(key >> 32);
                row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
                row.site_reads = a.site[2u * row.cell + row.side];
                // side L: the records that hold the cell and the one above it; (cell + 1 <= total_cells: span holds total_cells + 2)
                row.span = a.span[row.cell + (row.side ? 0u : 1u)];
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

void launch_breakend_scan(const BreakendArgs& a, int n_cus, hipStream_t stream) {
    if (a.rec.n_records == 0) return;
    const uint64_t blocks = (a.rec.n_records + kBreakendBlock - 1) / kBreakendBlock;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * 8));
    hipLaunchKernelGGL(breakend_scan_kernel, dim3(grid), dim3(kBreakendBlock), 0, stream, a);
}

void launch_breakend_span_prefix(const BreakendArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(breakend_span_prefix_kernel, dim3(1), dim3(kSpanPrefixBlock), 0, stream, a.span, a.ix.total_cells + 2u);
}

void launch_breakend_report(const BreakendArgs& a, hipStream_t stream) {
    const uint64_t blocks = ((1ull << a.log2n) + kBreakendBlock - 1) / kBreakendBlock;
    hipLaunchKernelGGL(breakend_report_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 2048)), dim3(kBreakendBlock), 0, stream, a);
}

}  // namespace bk
