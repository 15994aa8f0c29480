// bk_indels.hip -- short insertions and deletions from the reads (bk_indels_enable; `bronko call --indels`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section I; bronko_amd/host/indels.cpp and tests/indels_ref.py restate it.
// An event pass (bk_event_pass.h: the scan's queue loop, the span of a record on one diagonal, the report's append); its own are
//   indel_anchor  the anchor k-mers are cut from the record's 2-bit words as kmer_dump_count_kernel cuts them and looked up in the
//                 perfect hash of the reference k-mers (pilot, entry: two loads) and one bit per id (it starts at exactly one cell).
//                 A record along the reference is compared with ref_words, one against it with rc_words at the mirrored cell -- no
//                 record is reverse-complemented --, sixteen bases a step (XOR, fold the bit pairs, popcount).  delta = 0, the
//                 common case, is the record on one diagonal; delta != 0 is the rare record that is walked.
//   indel_walk    incremental: moving p by one exchanges one comparison on dL for one on dR.  Events go to an open-addressing
//                 table of its own: two key words, each claimed with a CAS; a slot matches iff both words are this event's, so the
//                 loser of the second CAS probes on.  A full table raises the overflow word.
//   indel_decode  a slot as a row (its key words: bk_indel_slot.h), there once both are written: the events that pass the thresholds.
// Vector stores and atomics only.
#include "bk_event_pass.h"
#include "bk_indel_slot.h"

namespace bk {
namespace {

typedef EventTally<IndelArgs::kScanTallies> IndelTally;
enum { T_RECORDS, T_ANCHORED, T_SPANNING, T_SUPPORTING, T_DISCORDANT };

__device__ __forceinline__ void indel_event_insert(const IndelArgs& a, uint32_t cell, uint32_t kind, uint32_t len, unsigned long long s, bool against) {
    // {cell, kind, length, S}: S's first base rides in the first word, so that neither word can equal the free word
    const unsigned long long k0 = (unsigned long long)cell | ((unsigned long long)kind << 32) | ((unsigned long long)(len - 1u) << 33) | ((s & 3ull) << 38);
    const unsigned long long k1 = s >> 2;
    const uint64_t mask = (1ull << a.log2n) - 1ull;
    uint64_t h = ((k0 ^ (k1 * 0xD6E8FEB86659FD93ull)) * 0x9E3779B97F4A7C15ull) >> (64u - a.log2n);
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        unsigned long long c0 = __hip_atomic_load(a.key0 + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0 == kEventFreeWord) { c0 = atomicCAS(a.key0 + h, kEventFreeWord, k0); if (c0 == kEventFreeWord) c0 = k0; }
        if (c0 == k0) {
            unsigned long long c1 = __hip_atomic_load(a.key1 + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c1 == kEventFreeWord) { c1 = atomicCAS(a.key1 + h, kEventFreeWord, k1); if (c1 == kEventFreeWord) c1 = k1; }
            if (c1 == k1) { atomicAdd(a.counts + 2u * h + (against ? 1u : 0u), 1u); return; }
        }
        h = (h + 1) & mask;
    }
    atomicExch(a.tallies + IndelArgs::kOverflow, 1ull);   // every slot is another event's: the sample's result is an error
}

// A record's anchors and all that needs no breakpoint.  Returns true with `work` filled for a record with delta != 0 that passed
// the checks: {record | against << 31, a | b << 16, dL, dR}.
__device__ __forceinline__ bool indel_anchor(const IndelArgs& a, uint32_t r, IndelTally& t, uint4& work) {
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
    if (delta > (int32_t)a.max_len || -delta > (int32_t)a.max_len) { t.v[T_DISCORDANT]++; return false; }
    if (!cells_placed(a.ix, an.ca, an.cb, min(dL, dR), max(dL, dR) + n)) return false;
    if (delta != 0) {
        work = make_uint4(r | (against ? 0x80000000u : 0u), (uint32_t)pa | ((uint32_t)pb << 16), (uint32_t)dL, (uint32_t)dR);
        return true;
    }
    if (ref_span_count(a.ix, w, n, an, dL, a.max_mismatches, a.span)) t.v[T_SPANNING]++; else t.v[T_DISCORDANT]++;
    return false;
}

// delta != 0: the breakpoint, the normalised event, the table
__device__ __forceinline__ void indel_walk(const IndelArgs& a, const uint4 work, IndelTally& t) {
    const uint32_t r = work.x & 0x7fffffffu;
    const bool against = (work.x >> 31) != 0u;
    const int32_t pa = (int32_t)(work.y & 0xffffu), pb = (int32_t)(work.y >> 16), dL = (int32_t)work.z, dR = (int32_t)work.w;
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r], delta = dR - dL;
    const int32_t I = delta < 0 ? -delta : 0, D = delta > 0 ? delta : 0;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const int32_t p0 = pa + k, p1 = pb - I;
    if (p0 > p1) { t.v[T_DISCORDANT]++; return; }
    const OrientedRecord rec{a.ix, w, n, last_word, against};
    int32_t m = rec.span_mm(0, p0, dL) + rec.span_mm(p0 + I, n, dR);
    int32_t best = m, best_p = p0;
    for (int32_t p = p0; p < p1; ++p) {
        m += rec.mm(p, dL) - rec.mm(p + I, dR);
        if (m < best) { best = m; best_p = p + 1; }
    }
    if (best > (int32_t)a.max_mismatches) { t.v[T_DISCORDANT]++; return; }
    int32_t pos = dL + best_p;
    // F: the first cell of the stretch of ACGT letters of the sequence that holds pos - 1 (the record's cells hold no other letter)
    const int32_t F = acgt_floor(a.ix, (uint32_t)(dL + pa), min(dL, dR));
    unsigned long long s = 0ull;
    if (D) {
        while (pos - 1 > F && sym_at(a.ix.ref_words, (uint32_t)(pos - 1)) == sym_at(a.ix.ref_words, (uint32_t)(pos + D - 1))) --pos;
    } else {
        for (int32_t i = 0; i < I; ++i) s |= (unsigned long long)rec.at(best_p + i) << (2 * i);
        const unsigned long long smask = I == 32 ? ~0ull : (1ull << (2 * I)) - 1ull;
        while (pos - 1 > F) {
            const unsigned long long last = (s >> (2 * (I - 1))) & 3ull;
            if ((unsigned long long)sym_at(a.ix.ref_words, (uint32_t)(pos - 1)) != last) break;
            s = ((s << 2) | last) & smask;
            --pos;
        }
    }
    t.v[T_SUPPORTING]++;
    indel_event_insert(a, (uint32_t)pos, D ? 0u : 1u, (uint32_t)(D ? D : I), s, against);
}

__device__ __forceinline__ bool indel_decode(const IndelArgs& a, uint64_t i, IndelRecordDev& row, bool& pass) {
    IndelSlot s;
    if (!indel_slot_decode(a.key0[i], a.key1[i], s)) return false;
    row.cell = s.cell;
    row.len = s.kind ? -(int32_t)s.len : (int32_t)s.len;
    row.seq = s.seq;
    row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
    row.ref_span = a.span[row.cell];
    row.pad = 0u;
    const unsigned long long support = (unsigned long long)row.fwd + row.rev;
    pass = support >= a.min_reads && support * 1000000ull >= (unsigned long long)a.min_af_ppm * (support + row.ref_span);
    return true;
}

__global__ __launch_bounds__(kEventBlock) void indel_scan_kernel(IndelArgs a) { event_scan<IndelArgs, indel_anchor, indel_walk>(a); }
__global__ __launch_bounds__(kEventBlock) void indel_report_kernel(IndelArgs a) { event_report<IndelArgs, IndelRecordDev, indel_decode>(a); }

}  // namespace

void launch_indel_scan(const IndelArgs& a, int n_cus, hipStream_t stream) { launch_event_scan(indel_scan_kernel, a, n_cus, stream); }
void launch_indel_report(const IndelArgs& a, hipStream_t stream) { launch_event_report(indel_report_kernel, a, stream); }

}  // namespace bk
