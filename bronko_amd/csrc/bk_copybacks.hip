// bk_copybacks.hip -- strand-switch (copy-back, snap-back) junctions from the reads (bk_copybacks_enable; `bronko call --copybacks`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section B; bronko_amd/host/copybacks.cpp and tests/copybacks_ref.py restate it.
//   copyback_scan_kernel         behind the scan of the same records, a lane per record, shaped as junction_scan_kernel (bk_junctions.hip):
//                                both ends' anchors through bk_anchor.h (end_anchors).  On one strand: delta = 0 inline (the Hamming
//                                pass with an early exit, two atomics on `span`), nothing else.  On two strands with f + k <= g the
//                                record is rare: those are gathered in a queue of the wave (LDS, filled through a ballot) and walked
//                                a lane each once 64 wait.  An arm that runs down the reference is a plain diagonal of rc_words, so
//                                mismatches / sym_at of bk_anchor.h serve both arms.  The walk is incremental: moving p by one
//                                exchanges one comparison on arm A for one on arm B; the best p by (m, min(x, y), p); then the two
//                                slide loops.  Events go to an open-addressing table whose key is one word, lo | kind << 31 | hi << 32
//                                (both cells below 2^27: never the free word), claimed with one CAS, two counters a slot.  A full
//                                table raises the overflow word.  The sample's tallies: one add per wave and tally.
//   copyback_span_prefix_kernel  at the sample's end: `span` prefix-summed in place by one workgroup.
//   copyback_report_kernel       the table's events with enough reads and distance, appended with one returning add per wave.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kCopybackBlock = 256;
constexpr uint32_t kCopybackQueue = 128;   // entries of a wave's queue: fewer than 64 wait when up to 64 more arrive
constexpr unsigned long long kFreeWord = ~0ull;
constexpr int kScanTallies = 6;            // records, same_strand, ref_spanning, switched, supporting, discordant
constexpr int kCandidates = 6, kReported = 7, kOverflow = 8;   // CopybackArgs::tallies behind them

struct CopybackTally { uint32_t v[kScanTallies] = {0, 0, 0, 0, 0, 0}; };
enum { T_RECORDS, T_SAME_STRAND, T_SPANNING, T_SWITCHED, T_SUPPORTING, T_DISCORDANT };

__device__ __forceinline__ void event_insert(const CopybackArgs& a, uint32_t lo, uint32_t hi, uint32_t kind, bool hi_first) {
    const unsigned long long key = (unsigned long long)lo | ((unsigned long long)kind << 31) | ((unsigned long long)hi << 32);
    const uint64_t mask = (1ull << a.log2n) - 1ull;
    uint64_t h = (key * 0x9E3779B97F4A7C15ull) >> (64u - a.log2n);
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        unsigned long long c = __hip_atomic_load(a.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == kFreeWord) { c = atomicCAS(a.keys + h, kFreeWord, key); if (c == kFreeWord) c = key; }
        if (c == key) { atomicAdd(a.counts + 2u * h + (hi_first ? 1u : 0u), 1u); return; }
        h = (h + 1) & mask;
    }
    atomicExch(a.tallies + kOverflow, 1ull);   // every slot is another event's: the sample's result is an error
}

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
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const uint32_t m = an.against ? mismatches(w, last_word, 0u, (uint32_t)n, a.ix.rc_words, (int64_t)a.ix.total_cells - dL - n, a.max_mismatches)
                                  : mismatches(w, last_word, 0u, (uint32_t)n, a.ix.ref_words, dL, a.max_mismatches);
    if (m > a.max_mismatches) return false;
    t.v[T_SPANNING]++;
    atomicAdd(a.span + (dL + an.pa + k), 1u);
    atomicAdd(a.span + (dL + an.pb + 1), 0xffffffffu);
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
    event_insert(a, (uint32_t)lo, (uint32_t)hi, kind, x > y);
}

__global__ __launch_bounds__(kCopybackBlock) void copyback_scan_kernel(CopybackArgs a) {
    __shared__ uint4 queue_s[kCopybackBlock / 64][kCopybackQueue];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* const q = queue_s[wave];
    const uint64_t n = a.rec.n_records_dev ? std::min<uint64_t>(a.rec.n_records, *a.rec.n_records_dev) : a.rec.n_records;
    const uint64_t stride = (uint64_t)gridDim.x * kCopybackBlock;
    CopybackTally t;
    uint32_t qn = 0;                                  // records waiting in the wave's queue (the same in every lane)
    for (uint64_t base = (uint64_t)blockIdx.x * kCopybackBlock + wave * 64u; base < n; base += stride) {
        const uint64_t r = base + lane;
        uint4 work = make_uint4(0u, 0u, 0u, 0u);
        const bool slow = r < n && copyback_anchor(a, (uint32_t)r, t, work);
        const unsigned long long mask = __ballot(slow);
        if (mask == 0ull) continue;
        if (slow) q[qn + lane_prefix(mask)] = work;   // (qn < 64 here and at most 64 arrive: below kCopybackQueue)
        qn += (uint32_t)__popcll(mask);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the queue is the wave's own: its lanes' stores before its lanes' loads)
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64u) {
            qn -= 64u;
            work = q[qn + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            copyback_walk(a, work, t);
        }
    }
    if (lane < qn) copyback_walk(a, q[lane], t);
#pragma unroll
    for (int i = 0; i < kScanTallies; ++i) {
        const uint32_t sum = wave_total(t.v[i]);
        if (lane == 0 && sum) atomicAdd(a.tallies + i, (unsigned long long)sum);
    }
}

// span[0 .. n) prefix-summed in place by one workgroup (span_prefix_block, bk_anchor.h)
__global__ __launch_bounds__(kSpanPrefixBlock) void copyback_span_prefix_kernel(unsigned int* __restrict__ span, uint32_t n) { span_prefix_block(span, n); }

__global__ __launch_bounds__(kCopybackBlock) void copyback_report_kernel(CopybackArgs a) {
    const uint64_t n_slots = 1ull << a.log2n;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kCopybackBlock + (threadIdx.x & ~63u); base < n_slots; base += (uint64_t)gridDim.x * kCopybackBlock) {
        const uint64_t i = base + lane;
        bool there = false, pass = false;
        CopybackRecordDev row{};
        if (i < n_slots) {
            const unsigned long long key = a.keys[i];
            there = key != kFreeWord;
            if (there) {
                row.lo = (uint32_t)key & 0x7fffffffu; row.hi = (uint32_t)(key >> 32); row.kind = ((uint32_t)key) >> 31;
                row.lo_first = a.counts[2u * i]; row.hi_first = a.counts[2u * i + 1u];
                const uint32_t off = row.kind == 0u ? 1u : 0u;   // (hi + 1 <= total_cells: span holds total_cells + 2)
                row.span_lo = a.span[row.lo + off]; row.span_hi = a.span[row.hi + off];
                pass = (unsigned long long)row.lo_first + row.hi_first >= a.min_reads && row.hi - row.lo >= a.min_dist;
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

void launch_copyback_scan(const CopybackArgs& a, int n_cus, hipStream_t stream) {
    if (a.rec.n_records == 0) return;
    const uint64_t blocks = (a.rec.n_records + kCopybackBlock - 1) / kCopybackBlock;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * 8));
    hipLaunchKernelGGL(copyback_scan_kernel, dim3(grid), dim3(kCopybackBlock), 0, stream, a);
}

void launch_copyback_span_prefix(const CopybackArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(copyback_span_prefix_kernel, dim3(1), dim3(kSpanPrefixBlock), 0, stream, a.span, a.ix.total_cells + 2u);
}

void launch_copyback_report(const CopybackArgs& a, hipStream_t stream) {
    const uint64_t blocks = ((1ull << a.log2n) + kCopybackBlock - 1) / kCopybackBlock;
    hipLaunchKernelGGL(copyback_report_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 2048)), dim3(kCopybackBlock), 0, stream, a);
}

}  // namespace bk
