// bk_indels.hip -- short insertions and deletions from the reads (bk_indels_enable; `bronko call --indels`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section I; bronko_amd/host/indels.cpp and tests/indels_ref.py restate it.
//   indel_scan_kernel         behind the scan of the same records, a lane per record.  The anchor k-mers are cut from the record's
//                             2-bit words as kmer_dump_count_kernel cuts them and looked up in the perfect hash of the reference
//                             k-mers (pilot, entry: two loads) and one bit per id (it starts at exactly one cell).  A record along
//                             the reference is compared with ref_words, one against it with rc_words at the mirrored cell -- no
//                             record is reverse-complemented --, sixteen bases a step (XOR, fold the bit pairs, popcount).
//                             delta = 0, the common case: the Hamming pass with an early exit and two atomics on `span`.
//                             delta != 0 is rare: those records are gathered in a queue of the wave (LDS, filled through a
//                             ballot) and walked a lane each once 64 wait -- a wave never idles through one lane's breakpoint
//                             walk.  The walk is incremental: moving p by one exchanges one comparison on dL for one on dR.
//                             Events go to an open-addressing table: two key words, each claimed with a CAS; a slot matches iff
//                             both words are this event's, so the loser of the second CAS probes on.  A full table raises the
//                             overflow word.  The sample's tallies: one add per wave and tally.
//   indel_span_prefix_kernel  at the sample's end: `span` prefix-summed in place by one workgroup.
//   indel_report_kernel       the table's events that pass the thresholds, appended with one returning add per wave.
// Vector stores and atomics only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bk_anchor.h"
#include "bk_scan_common.h"

namespace bk {
namespace {

constexpr int kIndelBlock = 256;
constexpr uint32_t kIndelQueue = 128;      // entries of a wave's queue: fewer than 64 wait when up to 64 more arrive
constexpr unsigned long long kFreeWord = ~0ull;

struct IndelTally { uint32_t records = 0, anchored = 0, spanning = 0, supporting = 0, discordant = 0; };

__device__ __forceinline__ void event_insert(const IndelArgs& a, uint32_t cell, uint32_t kind, uint32_t len, unsigned long long s, bool against) {
    // {cell, kind, length, S}: S's first base rides in the first word, so that neither word can equal the free word
    const unsigned long long k0 = (unsigned long long)cell | ((unsigned long long)kind << 32) | ((unsigned long long)(len - 1u) << 33) | ((s & 3ull) << 38);
    const unsigned long long k1 = s >> 2;
    const uint64_t mask = (1ull << a.log2n) - 1ull;
    uint64_t h = ((k0 ^ (k1 * 0xD6E8FEB86659FD93ull)) * 0x9E3779B97F4A7C15ull) >> (64u - a.log2n);
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        unsigned long long c0 = __hip_atomic_load(a.key0 + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c0 == kFreeWord) { c0 = atomicCAS(a.key0 + h, kFreeWord, k0); if (c0 == kFreeWord) c0 = k0; }
        if (c0 == k0) {
            unsigned long long c1 = __hip_atomic_load(a.key1 + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c1 == kFreeWord) { c1 = atomicCAS(a.key1 + h, kFreeWord, k1); if (c1 == kFreeWord) c1 = k1; }
            if (c1 == k1) { atomicAdd(a.counts + 2u * h + (against ? 1u : 0u), 1u); return; }
        }
        h = (h + 1) & mask;
    }
    atomicExch(a.tallies + 7, 1ull);   // every slot is another event's: the sample's result is an error
}

// A record's anchors and all that needs no breakpoint.  Returns true with `work` filled for a record with delta != 0 that passed
// the checks: {record | against << 31, a | b << 16, dL, dR}.
__device__ __forceinline__ bool indel_anchor(const IndelArgs& a, uint32_t r, IndelTally& t, uint4& work) {
    const int32_t k = a.ix.k, n = (int32_t)a.rec.lens[r];
    if (n < k) return false;                          // (trimmed away: no record any more)
    t.records++;
    if (n < 2 * k) return false;
    const uint32_t* __restrict__ w = a.rec.words + (uint64_t)r * a.rec.stride_words;
    Anchors an;
    if (!anchors_of(a.ix, w, n, an)) return false;
    const bool against = an.against;
    const int32_t pa = an.pa, pb = an.pb;
    t.anchored++;
    const int32_t dL = (int32_t)an.ca - pa, dR = (int32_t)an.cb - pb, delta = dR - dL;
    if (delta > (int32_t)a.max_len || -delta > (int32_t)a.max_len) { t.discordant++; return false; }
    if (!cells_placed(a.ix, an.ca, an.cb, min(dL, dR), max(dL, dR) + n)) return false;
    if (delta != 0) {
        work = make_uint4(r | (against ? 0x80000000u : 0u), (uint32_t)pa | ((uint32_t)pb << 16), (uint32_t)dL, (uint32_t)dR);
        return true;
    }
    const uint32_t last_word = (uint32_t)(n - 1) >> 4;
    const uint32_t m = against ? mismatches(w, last_word, 0u, (uint32_t)n, a.ix.rc_words, (int64_t)a.ix.total_cells - dL - n, a.max_mismatches)
                               : mismatches(w, last_word, 0u, (uint32_t)n, a.ix.ref_words, dL, a.max_mismatches);
    if (m > a.max_mismatches) { t.discordant++; return false; }
    t.spanning++;
    atomicAdd(a.span + (dL + pa + k), 1u);
    atomicAdd(a.span + (dL + pb + 1), 0xffffffffu);
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
    if (p0 > p1) { t.discordant++; return; }
    const OrientedRecord rec{a.ix, w, n, last_word, against};
    int32_t m = rec.span_mm(0, p0, dL) + rec.span_mm(p0 + I, n, dR);
    int32_t best = m, best_p = p0;
    for (int32_t p = p0; p < p1; ++p) {
        m += rec.mm(p, dL) - rec.mm(p + I, dR);
        if (m < best) { best = m; best_p = p + 1; }
    }
    if (best > (int32_t)a.max_mismatches) { t.discordant++; return; }
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
    t.supporting++;
    event_insert(a, (uint32_t)pos, D ? 0u : 1u, (uint32_t)(D ? D : I), s, against);
}

__global__ __launch_bounds__(kIndelBlock) void indel_scan_kernel(IndelArgs a) {
    __shared__ uint4 queue_s[kIndelBlock / 64][kIndelQueue];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint4* const q = queue_s[wave];
    const uint64_t n = a.rec.n_records_dev ? std::min<uint64_t>(a.rec.n_records, *a.rec.n_records_dev) : a.rec.n_records;
    const uint64_t stride = (uint64_t)gridDim.x * kIndelBlock;
    IndelTally t;
    uint32_t qn = 0;                                  // records waiting in the wave's queue (the same in every lane)
    for (uint64_t base = (uint64_t)blockIdx.x * kIndelBlock + wave * 64u; base < n; base += stride) {
        const uint64_t r = base + lane;
        uint4 work = make_uint4(0u, 0u, 0u, 0u);
        const bool slow = r < n && indel_anchor(a, (uint32_t)r, t, work);
        const unsigned long long mask = __ballot(slow);
        if (mask == 0ull) continue;
        if (slow) q[qn + lane_prefix(mask)] = work;
        qn += (uint32_t)__popcll(mask);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the queue is the wave's own: its lanes' stores before its lanes' loads)
        __builtin_amdgcn_wave_barrier();
        if (qn >= 64u) {
            qn -= 64u;
            work = q[qn + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            indel_walk(a, work, t);
        }
    }
    if (lane < qn) indel_walk(a, q[lane], t);
    const uint32_t sums[5] = {wave_total(t.records), wave_total(t.anchored), wave_total(t.spanning), wave_total(t.supporting), wave_total(t.discordant)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (sums[i]) atomicAdd(a.tallies + i, (unsigned long long)sums[i]);
    }
}

// span[0 .. n) prefix-summed in place by one workgroup (span_prefix_block, bk_anchor.h)
__global__ __launch_bounds__(kSpanPrefixBlock) void indel_span_prefix_kernel(unsigned int* __restrict__ span, uint32_t n) { span_prefix_block(span, n); }

__global__ __launch_bounds__(kIndelBlock) void indel_report_kernel(IndelArgs a) {
    const uint64_t n_slots = 1ull << a.log2n;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = (uint64_t)blockIdx.x * kIndelBlock + (threadIdx.x & ~63u); base < n_slots; base += (uint64_t)gridDim.x * kIndelBlock) {
        const uint64_t i = base + lane;
        bool there = false, pass = false;
        IndelRecordDev row{};
        if (i < n_slots) {
            const unsigned long long k0 = a.key0[i], k1 = a.key1[i];
            there = k0 != kFreeWord && k1 != kFreeWord;
            if (there) {
                row.cell = (uint32_t)k0;
                const uint32_t kind = (uint32_t)(k0 >> 32) & 1u, len = ((uint32_t)(k0 >> 33) & 31u) + 1u;
                row.len = kind ? -(int32_t)len : (int32_t)len;
                row.seq = (k1 << 2) | ((k0 >> 38) & 3ull);
                row.fwd = a.counts[2u * i]; row.rev = a.counts[2u * i + 1u];
                row.ref_span = a.span[row.cell];
                row.pad = 0u;
                const unsigned long long support = (unsigned long long)row.fwd + row.rev;
                pass = support >= a.min_reads && support * 1000000ull >= (unsigned long long)a.min_af_ppm * (support + row.ref_span);
            }
        }
        const unsigned long long m_there = __ballot(there), m_pass = __ballot(pass);
        if (m_there == 0ull) continue;
        unsigned long long at = 0ull;
        if (lane == 0) {
            atomicAdd(a.tallies + 5, (unsigned long long)__popcll(m_there));
            if (m_pass) at = atomicAdd(a.tallies + 6, (unsigned long long)__popcll(m_pass));
        }
        at = __shfl(at, 0);
        if (pass) {
            const uint64_t o = at + lane_prefix(m_pass);
            if (o < a.row_cap) a.rows[o] = row;
        }
    }
}

}  // namespace

void launch_indel_scan(const IndelArgs& a, int n_cus, hipStream_t stream) {
    if (a.rec.n_records == 0) return;
    const uint64_t blocks = (a.rec.n_records + kIndelBlock - 1) / kIndelBlock;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)n_cus * 8));
    hipLaunchKernelGGL(indel_scan_kernel, dim3(grid), dim3(kIndelBlock), 0, stream, a);
}

void launch_indel_span_prefix(const IndelArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(indel_span_prefix_kernel, dim3(1), dim3(kSpanPrefixBlock), 0, stream, a.span, a.ix.total_cells + 2u);
}

void launch_indel_report(const IndelArgs& a, hipStream_t stream) {
    const uint64_t blocks = ((1ull << a.log2n) + kIndelBlock - 1) / kIndelBlock;
    hipLaunchKernelGGL(indel_report_kernel, dim3((unsigned)std::min<uint64_t>(blocks, 2048)), dim3(kIndelBlock), 0, stream, a);
}

}  // namespace bk
