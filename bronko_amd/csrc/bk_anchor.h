// bk_anchor.h -- placing a record on the reference by two anchor k-mers: the arithmetic that the six event passes (bk_event_pass.h,
// which holds the shape they share) and link_scan_kernel (bk_linkage.hip) share -- anchors, placement, the oriented record and its
// breakpoint walk, the one-word event table, the prefix sum of a span array.  The rule is DESIGN.md section I's, stated in
// include/bronko_hip.h (bk_indels_enable).
//
// What is read of the index is an AnchorIndex (bk_kernels.h): the perfect hash of the reference k-mers (kmer_pos, pilots, m, log2nb,
// log2p, n_full), one bit per id that starts at exactly one cell (unique_bits), k, the sequences' first cells (seq_lo, n_seqs) and the
// runs of letters that are not ACGT (nruns, n_nruns) -- the engine's AnchorTables hold the last three.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "bk_scan_common.h"

namespace bk {

__device__ __forceinline__ uint32_t sym_at(const uint32_t* __restrict__ w, uint32_t i) { return (w[i >> 4] >> (2u * (i & 15u))) & 3u; }
// sixteen symbols from symbol `pos` on; word indices are clamped to last_word (a record's last word; ~0u for the references, which
// are padded behind).  symbols_at / read_symbols_at of bk_scan_common.h cut the same window 32 symbols wide from three words; a step
// here is sixteen bases, which two words hold, and the record's clamp and the references' lack of one share this one function.
__device__ __forceinline__ uint32_t sym16_at(const uint32_t* __restrict__ w, uint32_t pos, uint32_t last_word) {
    const uint32_t wi = pos >> 4;
    return __builtin_amdgcn_alignbit(w[min(wi + 1u, last_word)], w[min(wi, last_word)], 2u * (pos & 15u));
}
// one bit (the low one of its pair) per base of [i, min(i + 16, hi)) at which record[i ..] and text[diag + i ..] differ
__device__ __forceinline__ uint32_t mismatch_bits16(const uint32_t* __restrict__ w, uint32_t last_word, uint32_t i, uint32_t hi,
                                                    const uint32_t* __restrict__ text, int64_t diag) {
    uint32_t x = sym16_at(w, i, last_word) ^ sym16_at(text, (uint32_t)(diag + (int64_t)i), ~0u);
    x = (x | (x >> 1)) & 0x55555555u;
    const uint32_t c = hi - i;
    if (c < 16u) x &= (1u << (2u * c)) - 1u;
    return x;
}
// #{i in [lo, hi): record[i] != text[diag + i]}; gives up above `stop` (what it returns is then only known to be larger)
__device__ __forceinline__ uint32_t mismatches(const uint32_t* __restrict__ w, uint32_t last_word, uint32_t lo, uint32_t hi,
                                               const uint32_t* __restrict__ text, int64_t diag, uint32_t stop) {
    uint32_t m = 0;
    for (uint32_t i = lo; i < hi && m <= stop; i += 16u) m += (uint32_t)__popc(mismatch_bits16(w, last_word, i, hi, text, diag));
    return m;
}

// the k-mer at offset o of a record as an anchor: its cell and strand.  o + k <= the record's length.
__device__ __forceinline__ bool anchor_at(const AnchorIndex& a, const uint32_t* __restrict__ w, uint32_t o, uint32_t* cell, bool* against) {
    const uint32_t k = (uint32_t)a.k;
    const uint32_t w0 = o >> 4, sh = 2u * (o & 15u), wl = (o + k - 1u) >> 4;
    unsigned long long x = w[w0];
    if (wl > w0) x |= (unsigned long long)w[w0 + 1] << 32;
    x >>= sh;
    if (wl > w0 + 1) x |= (unsigned long long)w[w0 + 2] << (64u - sh);   // (sh > 0 here, as in kmer_dump_count_kernel)
    const unsigned long long kmask = (1ull << (2u * k)) - 1ull;
    const unsigned long long fwd = rev2_64(x) >> (64u - 2u * k);          // base o leads (kmer_to_u64)
    const unsigned long long rc = ~x & kmask;                             // its reverse complement: the complements, base o last
    const bool read_rc = !(fwd < rc);
    const unsigned long long canon = read_rc ? rc : fwd;
    const uint32_t pilot = a.pilots[phf_bucket(canon, a.log2nb)];
    const KmerPos kp = a.kmer_pos[phf_pos(canon, pilot, a.m, a.log2nb, a.log2p)];
    if (kp.key != canon) return false;
    const uint32_t id = kp.idflags & kIdMask;
    if (id >= a.n_full || !((a.unique_bits[id >> 5] >> (id & 31u)) & 1u)) return false;
    *cell = kp.refcell;
    *against = read_rc != ((kp.idflags >> 31) != 0u);
    return true;
}

__device__ __forceinline__ uint32_t seq_of(const AnchorIndex& a, uint32_t cell) {
    uint32_t lo = 0, hi = a.n_seqs;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.seq_lo[mid] <= cell) lo = mid; else hi = mid;
    }
    return lo;
}

// the first of the runs of letters that are not ACGT (ascending, disjoint) that ends behind cell `lo`; n_nruns: none does
__device__ __forceinline__ uint32_t first_run_behind(const AnchorIndex& a, int32_t lo) {
    uint32_t b = 0, e = a.n_nruns;
    while (b < e) {
        const uint32_t mid = (b + e) >> 1;
        if ((int32_t)a.nruns[mid].y > lo) e = mid; else b = mid + 1u;
    }
    return b;
}

// A record's two anchors, oriented along the reference
struct Anchors {
    bool against;          // the record reads against the reference
    int32_t pa, pb;        // the anchors' offsets a < b in r'
    uint32_t ca, cb;       // their cells
};
// A record's two end anchors as they are found, the record as packed (copyback_scan_kernel needs them on either strand)
struct EndAnchors {
    int32_t f_off, b_off;  // the front and the back anchor's offsets in the record
    uint32_t f_cell, b_cell;   // the first cells of their reference k-mers
    bool f_ag, b_ag;       // each: against the reference
};
// the first anchor k-mer from each end of a record of n >= 2k bases (offsets 0, 8, 16, 24 from either end)
__device__ __forceinline__ bool end_anchors(const AnchorIndex& a, const uint32_t* __restrict__ w, int32_t n, EndAnchors& e) {
    const int32_t k = a.k;
    e.f_off = -1; e.b_off = -1;
    e.f_cell = 0; e.b_cell = 0;
    e.f_ag = false; e.b_ag = false;
    for (int32_t o = 0; o <= 24 && o + k <= n; o += 8)
        if (anchor_at(a, w, (uint32_t)o, &e.f_cell, &e.f_ag)) { e.f_off = o; break; }
    if (e.f_off < 0) return false;
    for (int32_t o = n - k; o >= n - k - 24 && o >= 0; o -= 8)
        if (anchor_at(a, w, (uint32_t)o, &e.b_cell, &e.b_ag)) { e.b_off = o; break; }
    return e.b_off >= 0;
}
// ... both ends searched whatever the other gave (breakend_scan_kernel, bk_breakends.hip: the record with exactly one end anchored).
// Returns the ends that have an anchor: bit 0 the front, bit 1 the back; an end without one keeps its offset -1.  With both it fills
// `e` exactly as end_anchors does.
__device__ __forceinline__ uint32_t end_anchors_both(const AnchorIndex& a, const uint32_t* __restrict__ w, int32_t n, EndAnchors& e) {
    const int32_t k = a.k;
    e.f_off = -1; e.b_off = -1;
    e.f_cell = 0; e.b_cell = 0;
    e.f_ag = false; e.b_ag = false;
    for (int32_t o = 0; o <= 24 && o + k <= n; o += 8)
        if (anchor_at(a, w, (uint32_t)o, &e.f_cell, &e.f_ag)) { e.f_off = o; break; }
    for (int32_t o = n - k; o >= n - k - 24 && o >= 0; o -= 8)
        if (anchor_at(a, w, (uint32_t)o, &e.b_cell, &e.b_ag)) { e.b_off = o; break; }
    return (e.f_off >= 0 ? 1u : 0u) | (e.b_off >= 0 ? 2u : 0u);
}
// the two end anchors on one strand, oriented along the reference: a + k <= b
__device__ __forceinline__ bool anchors_of(const EndAnchors& e, int32_t k, int32_t n, Anchors& out) {
    if (e.f_ag != e.b_ag) return false;
    out.against = e.f_ag;
    out.pa = e.f_ag ? n - k - e.b_off : e.f_off; out.pb = e.f_ag ? n - k - e.f_off : e.b_off;   // offsets in r'
    out.ca = e.f_ag ? e.b_cell : e.f_cell; out.cb = e.f_ag ? e.f_cell : e.b_cell;
    return out.pa + k <= out.pb;
}
__device__ __forceinline__ bool anchors_of(const AnchorIndex& a, const uint32_t* __restrict__ w, int32_t n, Anchors& out) {
    EndAnchors e;
    return end_anchors(a, w, n, e) && anchors_of(e, a.k, n, out);
}
// the cells [lo, hi) inside sequence s and holding ACGT only
__device__ __forceinline__ bool arm_placed(const AnchorIndex& a, uint32_t s, int32_t lo, int32_t hi) {
    if (lo < (int32_t)a.seq_lo[s] || hi > (int32_t)a.seq_lo[s + 1]) return false;
    if (a.n_nruns) {
        const uint32_t i = first_run_behind(a, lo);
        if (i < a.n_nruns && (int32_t)a.nruns[i].x < hi) return false;
    }
    return true;
}
// both anchors in one sequence, the cells [lo, hi) inside it and holding ACGT only
__device__ __forceinline__ bool cells_placed(const AnchorIndex& a, uint32_t ca, uint32_t cb, int32_t lo, int32_t hi) {
    const uint32_t s = seq_of(a, ca);
    return seq_of(a, cb) == s && arm_placed(a, s, lo, hi);
}

// A record as the breakpoint walks of indel_scan_kernel and junction_scan_kernel read it: r', the record along the reference.  One
// against the reference reads rc_words at the mirrored cells, so no record is reverse-complemented.
struct OrientedRecord {
    const AnchorIndex& ix;
    const uint32_t* __restrict__ w;
    int32_t n;
    uint32_t last_word;
    bool against;
    // #{j in [j0, j1): r'[j] != ref[d + j]}
    __device__ __forceinline__ int32_t span_mm(int32_t j0, int32_t j1, int32_t d) const {
        if (j0 >= j1) return 0;
        return (int32_t)(against ? mismatches(w, last_word, (uint32_t)(n - j1), (uint32_t)(n - j0), ix.rc_words, (int64_t)ix.total_cells - d - n, ~0u)
                                 : mismatches(w, last_word, (uint32_t)j0, (uint32_t)j1, ix.ref_words, d, ~0u));
    }
    __device__ __forceinline__ uint32_t at(int32_t j) const { return against ? 3u - sym_at(w, (uint32_t)(n - 1 - j)) : sym_at(w, (uint32_t)j); }   // r'[j]
    __device__ __forceinline__ int32_t mm(int32_t j, int32_t d) const { return at(j) != sym_at(ix.ref_words, (uint32_t)(d + j)) ? 1 : 0; }
};
// F of the normalisation: the first cell of the stretch of ACGT letters of sequence s in front of cells that begin at `lo` and hold
// no other letter: the runs in front of them are the ones that end at lo or before
__device__ __forceinline__ int32_t acgt_floor_in(const AnchorIndex& a, uint32_t s, int32_t lo) {
    int32_t F = (int32_t)a.seq_lo[s];
    if (a.n_nruns) {
        const uint32_t i = first_run_behind(a, lo);
        if (i > 0u) F = max(F, (int32_t)a.nruns[i - 1u].y);
    }
    return F;
}
// ... of the sequence that holds `cell`
__device__ __forceinline__ int32_t acgt_floor(const AnchorIndex& a, uint32_t cell, int32_t lo) { return acgt_floor_in(a, seq_of(a, cell), lo); }
// the stretch [lo, hi) of ACGT letters of sequence s around `cell`, which holds one
__device__ __forceinline__ void acgt_stretch(const AnchorIndex& a, uint32_t s, int32_t cell, int32_t& lo, int32_t& hi) {
    lo = (int32_t)a.seq_lo[s]; hi = (int32_t)a.seq_lo[s + 1];
    if (a.n_nruns) {
        const uint32_t i = first_run_behind(a, cell);   // (it ends behind the cell and does not hold it: it begins behind it)
        if (i < a.n_nruns) hi = min(hi, (int32_t)a.nruns[i].x);
        if (i > 0u) lo = max(lo, (int32_t)a.nruns[i - 1u].y);
    }
}

// The breakpoint of a record whose front lies on diagonal dL and whose back on dR (junction_scan_kernel: dR > dL; duplication_scan_kernel:
// dR < dL): m(p) = #{j < p: r'[j] != ref[dL + j]} + #{j >= p: r'[j] != ref[dR + j]} for p in [p0, p1], p0 <= p1.  Returns the least
// m(p), best_p the smallest p that has it.  Incremental: moving p by one exchanges one comparison on dR for one on dL.  The cells read
// are [dL, dL + p1) and [dR + p0, dR + n).
__device__ __forceinline__ int32_t breakpoint_walk(const OrientedRecord& rec, int32_t p0, int32_t p1, int32_t dL, int32_t dR, int32_t& best_p) {
    int32_t m = rec.span_mm(0, p0, dL) + rec.span_mm(p0, rec.n, dR);
    int32_t best = m;
    best_p = p0;
    for (int32_t p = p0; p < p1; ++p) {
        m += rec.mm(p, dL) - rec.mm(p, dR);
        if (m < best) { best = m; best_p = p + 1; }
    }
    return best;
}

// The event table of every event pass but the indels' (two key words: bk_indels.hip): open addressing, the key one word,
// cell | len << 32, claimed with one CAS; two counters a slot, chosen by `against`.  The layouts it serves, none of which can be
// the free word (a cell is below 2^27):
//   junction_walk     pos | D << 32                          {fwd, rev}
//   duplication_walk  pos | E << 32                          {fwd, rev}
//   copyback_walk     lo | kind << 31 | hi << 32             {lo_first, hi_first}
//   chimera_walk      lo | sides << 28 | hi << 32            {lo_first, hi_first}
//   breakend_walk     cell | side << 27 | tag << 32          {fwd, rev}   (`len` is a tag of 32 bits: the low word below 2^28 keeps the key off the free word)
// A table whose every slot is another event's raises *overflow: the sample's result is an error.
constexpr unsigned long long kEventFreeWord = ~0ull;
__device__ __forceinline__ void event_insert(unsigned long long* __restrict__ keys, unsigned int* __restrict__ counts, uint32_t log2n,
                                             unsigned long long* __restrict__ overflow, uint32_t cell, uint32_t len, bool against) {
    const unsigned long long key = (unsigned long long)cell | ((unsigned long long)len << 32);
    const uint64_t mask = (1ull << log2n) - 1ull;
    uint64_t h = (key * 0x9E3779B97F4A7C15ull) >> (64u - log2n);
    for (uint64_t probes = 0; probes <= mask; ++probes) {
        unsigned long long c = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == kEventFreeWord) { c = atomicCAS(keys + h, kEventFreeWord, key); if (c == kEventFreeWord) c = key; }
        if (c == key) { atomicAdd(counts + 2u * h + (against ? 1u : 0u), 1u); return; }
        h = (h + 1) & mask;
    }
    atomicExch(overflow, 1ull);
}

constexpr int kSpanPrefixBlock = 1024;
// span[0 .. n) prefix-summed in place by one workgroup of kSpanPrefixBlock threads (u32 arithmetic wraps: a -1 that precedes its +1
// in memory order still cancels): a thread sums its stretch, the stretches' sums are scanned through LDS, the thread writes its stretch.
__device__ __forceinline__ void span_prefix_block(unsigned int* __restrict__ span, uint32_t n) {
    __shared__ unsigned int part_s[2][kSpanPrefixBlock];
    const uint32_t per = (n + kSpanPrefixBlock - 1) / kSpanPrefixBlock;
    const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
    unsigned int sum = 0u;
    for (uint32_t i = lo; i < hi; ++i) sum += span[i];
    part_s[0][threadIdx.x] = sum;
    __syncthreads();
    int cur = 0;
    for (uint32_t off = 1; off < (uint32_t)kSpanPrefixBlock; off <<= 1) {   // inclusive scan of the stretches' sums
        const unsigned int v = part_s[cur][threadIdx.x] + (threadIdx.x >= off ? part_s[cur][threadIdx.x - off] : 0u);
        part_s[cur ^ 1][threadIdx.x] = v;
        __syncthreads();
        cur ^= 1;
    }
    unsigned int acc = part_s[cur][threadIdx.x] - sum;   // what precedes this thread's stretch
    for (uint32_t i = lo; i < hi; ++i) { acc += span[i]; span[i] = acc; }
}

__device__ __forceinline__ uint32_t wave_total(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

}  // namespace bk
