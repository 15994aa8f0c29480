// bk_ingest.cpp -- from a caller's reads to records ready to scan: the bk_push_reads_* entry points (ASCII or packed, from the host
// or the device), K0's launch, the trimming stage (bk_adapters_set, bk_primers_set) and the host packer.  Every push ends in
// push_device (bk_engine.cpp), which takes the batch as a Records view of the RecordBufs that hold it.
#include <cmath>
#include <cstring>

#include "../host/lcb.hpp"
#include "bk_engine.h"

// The checks the bk_push_reads_* entry points share, in this order (`batch_ok`: the batch's pointers and shape are valid;
// `too_large`: it holds 2^32 bases or more).  kPush: push the batch; BK_OK: it is empty; else the error.
static constexpr int kPush = 1;
static int push_checks(bk_engine* e, int mate, uint64_t n, bool batch_ok, const char* bad_batch, bool too_large) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (!e->in_sample) return fail(BK_ERR_STATE, "bk_push_reads_* called before bk_sample_begin");
    if (mate < 0 || mate > 1) return fail(BK_ERR_INVALID, "mate must be 0 or 1");
    if (n == 0) return BK_OK;
    if (!batch_ok) return fail(BK_ERR_INVALID, "%s", bad_batch);
    if (too_large) return fail(BK_ERR_INVALID, "batch too large: push at most 2^32 bases per call");
    BK_HIP(hipSetDevice(e->device));
    return kPush;
}
static int packed_checks(bk_engine* e, int mate, const void* words, uint32_t stride_words, const void* lens, uint64_t n) {
    return push_checks(e, mate, n, words && lens && stride_words != 0 && stride_words <= 4096, "bad record batch",
                       stride_words != 0 && n > (1ull << 32) / ((uint64_t)stride_words * 16));
}
// --min-base-qual: a quality byte below '!' + min_qual (Phred+33) makes its base an N; 0 is off, and the call is the plain one.
// In front of push_checks: the range; the quality lines of a batch that push_checks will let through
static constexpr int kMaxMinQual = 93;   // ('!' + 93 = '~', the last printable quality symbol)
static int qual_checks(const bk_engine* e, int mate, const void* qual, uint64_t n_reads, int min_qual) {
    if (min_qual < 0 || min_qual > kMaxMinQual) return fail(BK_ERR_INVALID, "min_qual must be between 0 and %d", kMaxMinQual);
    if (min_qual && !qual && e && e->in_sample && mate >= 0 && mate <= 1 && n_reads) return fail(BK_ERR_INVALID, "bad read batch: no quality lines");
    return BK_OK;
}
// The packed pushes: `ends` null (the plain calls: refused while primers or adapters are set, since those records would go
// untrimmed) or the records' end flags (read only while primers or adapters are set)
static int no_end_flags(const bk_engine* e, const char* fn) {
    const char* set = !e->primers ? "adapters are set (bk_adapters_set)"
                      : e->adapters ? "primers and adapters are set (bk_primers_set, bk_adapters_set)" : "primers are set (bk_primers_set)";
    return fail(BK_ERR_STATE, "%s: %s and these records carry no end flags: push them with %s_ends", fn, set, fn);
}
static int ends_checks(const bk_engine* e, const void* ends, uint64_t n) {   // the *_ends calls, in front of packed_checks
    return e && e->trims() && !ends && n ? fail(BK_ERR_INVALID, "bad record batch: no end flags") : BK_OK;
}

// ASCII reads: the packer's records hold up to 16 bases per word and at most 65535 bases (a longer run of bases is cut into records
// that overlap by k - 1): words per record, and a bound on the records a batch becomes
struct PackGeom {
    uint32_t stride; uint64_t cap;
    PackGeom(int k, uint64_t n_reads, uint64_t total, uint64_t longest)
        : stride((uint32_t)std::min<uint64_t>((std::max<uint64_t>(longest, (uint64_t)k) + 15) / 16, 4095)),
          cap(n_reads + total / (uint64_t)k + total / (std::min<uint64_t>((uint64_t)stride * 16, 65535) - (uint64_t)(k - 1)) + 16) {}
};
// bk_adapters_set, bk_primers_set: the adapters, then the primers, come off the records that touch a read end (adapter_find_kernel
// and adapter_trim_kernel, primer_trim_kernel: in place), on the engine stream between the packer or the copy that made the records
// and everything that reads them.  `r` is a view of `b`; `ends`: the records' end flags (b's, or the caller's own on the device)
static int trim_records(bk_engine* e, int mate, RecordBufs& b, const Records& r, const uint8_t* ends) {
    if (e->adapters) {
        Adapters& ad = *e->adapters;
        const size_t had = ad.cut.n;
        BK_HIP(grow(ad.cut, r.n, 0, e->stream));
        if (ad.cut.n != had) BK_HIP(hipMemsetAsync(ad.cut.p, 0xFF, ad.cut.n * sizeof(uint32_t), e->stream));   // (the kernels leave kNoCut everywhere: filled once per allocation)
        bk_engine::Span sp(e, 2);
        bk::AdapterArgs t{};
        t.words = b.words.p; t.lens = b.lens.p; t.ends = ends; t.cut = ad.cut.p; t.n_records = r.n; t.n_records_dev = r.n_dev;
        t.stride_words = r.stride_words; t.k = e->ix->k; t.n_adapters = ad.n; t.min_overlap = ad.min_overlap; t.allowed_steps = ad.allowed_steps;
        t.stats = ad.stats.p + mate * 2; t.n_real = e->kstats_cur() + mate * 4 + 0;
        std::copy(ad.entry, ad.entry + bk::kMaxAdapters, t.adapters);
        bk::launch_adapter_trim(t, e->ix->n_cus, e->stream);
    }
    if (!e->primers) return BK_OK;
    bk_engine::Span sp(e, 2);
    bk::TrimArgs t{};
    t.words = b.words.p; t.lens = b.lens.p; t.ends = ends; t.n_records = r.n; t.n_records_dev = r.n_dev; t.stride_words = r.stride_words;
    t.k = e->ix->k; t.table = e->primers->table.p; t.n_primers = e->primers->n; t.max_mismatches = e->primers->max_mismatches;
    t.stats = e->primers->stats.p + mate * 3; t.n_real = e->kstats_cur() + mate * 4 + 0;
    bk::launch_primer_trim(t, e->ix->n_cus, e->stream);
    return BK_OK;
}

// the packer (records pushed: tallied on the device) into the slot's record buffers, then the push of those records
// (q: the quality lines and threshold of a bk_push_reads_ascii_qual* batch, or null); with primers or adapters set the packer also
// writes the records' end flags and the records are trimmed in between
static int pack_and_push(bk_engine* e, int mate, bk_engine::IngestSlot& sl, const uint8_t* bases, uint32_t shift, const unsigned long long* offsets,
                         uint64_t n_reads, uint64_t total, PackGeom g, const bk::QualArgs* q) {
    if (!sl.d_nrec.p) BK_HIP(sl.d_nrec.alloc(4));
    if (e->trims()) BK_HIP(grow(sl.rec.ends, g.cap, 0, e->stream));
    uint8_t* ends = e->trims() ? sl.rec.ends.p : nullptr;
    const Records r = sl.rec.view(g.stride, g.cap, sl.d_nrec.p, total);   // (a batch holds fewer k-mers than bases)
    bk::PackArgs pa{};
    pa.shift = shift; pa.bases = bases; pa.offsets = offsets; pa.n_reads = n_reads; pa.k = e->ix->k; pa.stride_words = g.stride;
    pa.words = sl.rec.words.p; pa.lens = sl.rec.lens.p; pa.cap = g.cap; pa.n_records = sl.d_nrec.p; pa.work = sl.d_work.p;
    { bk_engine::Span sp(e, 2); bk::launch_pack_reads(pa, e->kstats_cur() + mate * 4 + 0, e->stream, q, ends); }
    if (ends) { if (int rc = trim_records(e, mate, sl.rec, r, ends)) return rc; }
    return push_device(e, mate, r);
}

// bk_push_reads_ascii and bk_push_reads_ascii_qual (qual: null, or the quality lines at the same offsets; thr = '!' + min_qual)
static int push_ascii(bk_engine* e, int mate, const uint8_t* buf, const uint8_t* qual, const uint64_t* offsets, uint64_t n_reads, uint32_t thr) {
    const bool too_large = buf && offsets && n_reads && offsets[n_reads] - offsets[0] >= (1ull << 32);
    if (int rc = push_checks(e, mate, n_reads, buf && offsets, "bad read batch", too_large); rc != kPush) return rc;
    const uint64_t base0 = offsets[0], total = offsets[n_reads] - base0;
    if (!e->copy_stream) BK_HIP(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    bk_engine::IngestSlot& sl = e->slots[e->next_slot];
    e->next_slot = (e->next_slot + 1) % 3;
    BK_HIP(sl.done.create()); BK_HIP(sl.uploaded.create());
    if (sl.busy) { BK_HIP(hipEventSynchronize(sl.done)); sl.busy = false; }   // slot still owned by an earlier batch

    // staging copy (the caller's buffer is free as soon as we return) + longest read of the batch
    BK_HIP(sl.h_bases.grow(total + 1, 4096)); BK_HIP(sl.h_off.grow(n_reads + 1, 1024));
    if (qual) BK_HIP(sl.h_quals.grow(total + 1, 4096));
    std::memcpy(sl.h_bases.p, buf + base0, total);
    if (qual) std::memcpy(sl.h_quals.p, qual + base0, total);
    uint64_t longest = 0;
    for (uint64_t i = 0; i <= n_reads; i++) {
        sl.h_off.p[i] = offsets[i] - base0;
        if (i) longest = std::max(longest, offsets[i] - offsets[i - 1]);
    }
    const PackGeom g(e->ix->k, n_reads, total, longest);

    // (no stream to drain: nothing in flight uses the slot's buffers any more)
    BK_HIP(grow(sl.d_bases, total + 1, 4096)); BK_HIP(grow(sl.d_off, n_reads + 1, 1024)); BK_HIP(grow(sl.d_work, n_reads, 1024));
    if (qual) BK_HIP(grow(sl.d_quals, total + 1, 4096));
    BK_HIP(sl.rec.reserve(g.cap, g.stride, nullptr));

    BK_HIP(hipMemcpyAsync(sl.d_bases.p, sl.h_bases.p, total, hipMemcpyHostToDevice, e->copy_stream));
    if (qual) BK_HIP(hipMemcpyAsync(sl.d_quals.p, sl.h_quals.p, total, hipMemcpyHostToDevice, e->copy_stream));
    BK_HIP(hipMemcpyAsync(sl.d_off.p, sl.h_off.p, (n_reads + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, e->copy_stream));
    BK_HIP(hipEventRecord(sl.uploaded, e->copy_stream));
    BK_HIP(hipStreamWaitEvent(e->stream, sl.uploaded, 0));
    const bk::QualArgs q{sl.d_quals.p, 0u, thr};
    if (int rc = pack_and_push(e, mate, sl, sl.d_bases.p, 0, sl.d_off.p, n_reads, total, g, qual ? &q : nullptr)) return rc;
    BK_HIP(hipEventRecord(sl.done, e->stream));
    sl.busy = true;
    return BK_OK;
}

// sequence lines (d_bases) or quality lines (d_quals) from a pointer of any alignment: the packer stages them with 16-byte loads
// from a 16-byte boundary, so the pointer is rounded down and the offsets carry the difference (a device allocation starts on a
// 256-byte boundary, so the bytes in front belong to the same allocation)
static uint32_t align_shift(const void* p) { return (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u); }

static int push_ascii_device(bk_engine* e, int mate, const void* d_bases, const void* d_quals, const void* d_offsets, uint64_t n_reads,
                             uint64_t total_bases, uint32_t longest_read, uint32_t thr) {
    if (int rc = push_checks(e, mate, n_reads, d_bases && d_offsets, "bad read batch", total_bases >= (1ull << 32)); rc != kPush) return rc;
    // (everything is ordered by the engine's stream: the records of the previous batch were consumed by its scan before this
    // batch's packer starts, so one set of record buffers does; the stream is drained before one of them is replaced)
    bk_engine::IngestSlot& sl = e->dev_ascii;
    const PackGeom g(e->ix->k, n_reads, total_bases, longest_read);
    BK_HIP(sl.rec.reserve(g.cap, g.stride, e->stream)); BK_HIP(grow(sl.d_work, n_reads, 1024, e->stream));
    const uint32_t shift = align_shift(d_bases);
    const bk::QualArgs q{static_cast<const uint8_t*>(d_quals) - align_shift(d_quals), align_shift(d_quals), thr};
    return pack_and_push(e, mate, sl, static_cast<const uint8_t*>(d_bases) - shift, shift, static_cast<const unsigned long long*>(d_offsets), n_reads,
                         total_bases, g, d_quals ? &q : nullptr);
}

static int push_packed_device(bk_engine* e, int mate, const void* d_words, uint32_t stride_words, const void* d_lens, const void* d_ends, uint64_t n) {
    if (int rc = packed_checks(e, mate, d_words, stride_words, d_lens, n); rc != kPush) return rc;
    if (!e->trims()) return push_device(e, mate, Records{static_cast<const uint32_t*>(d_words), stride_words, static_cast<const uint16_t*>(d_lens), n});
    if (!d_ends) return no_end_flags(e, "bk_push_reads_packed_device");
    // the caller's records are not the engine's to rewrite: they are trimmed in a copy (the buffers of bk_push_reads_ascii_device:
    // everything that uses them is ordered by the engine's stream); the end flags are read where they are
    RecordBufs& b = e->dev_ascii.rec;
    BK_HIP(b.reserve(n, stride_words, e->stream));
    const Records r = b.view(stride_words, n);
    BK_HIP(hipMemcpyAsync(b.words.p, d_words, (size_t)n * stride_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream));
    BK_HIP(hipMemcpyAsync(b.lens.p, d_lens, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToDevice, e->stream));
    if (int rc = trim_records(e, mate, b, r, static_cast<const uint8_t*>(d_ends))) return rc;
    return push_device(e, mate, r);
}

static int push_packed(bk_engine* e, int mate, const uint32_t* words, uint32_t stride_words, const uint16_t* lens, const uint8_t* ends, uint64_t n) {
    if (int rc = packed_checks(e, mate, words, stride_words, lens, n); rc != kPush) return rc;
    if (e->trims() && !ends) return no_end_flags(e, "bk_push_reads_packed");
    if (!e->trims()) ends = nullptr;
    bk_engine::StageSlot& sl = e->stage[e->next_stage];
    e->next_stage ^= 1;
    BK_HIP(sl.done.create());
    if (sl.busy) { BK_HIP(hipEventSynchronize(sl.done)); sl.busy = false; }   // the scan that read this slot two pushes ago
    BK_HIP(sl.rec.reserve(n, stride_words, nullptr));
    if (ends) BK_HIP(grow(sl.rec.ends, n));
    const Records r = sl.rec.view(stride_words, n);
    {
        // the caller's buffer is free when this call returns: the batch is copied into the slot's pinned host buffer, from where
        // it travels asynchronously (an asynchronous copy straight from pageable memory would still be reading the caller's pages)
        const size_t bytes_w = (size_t)n * stride_words * sizeof(uint32_t), bytes_l = (size_t)n * sizeof(uint16_t), bytes_e = ends ? (size_t)n : 0;
        BK_HIP(sl.h.grow(bytes_w + bytes_l + bytes_e));
        std::memcpy(sl.h.p, words, bytes_w);
        std::memcpy(sl.h.p + bytes_w, lens, bytes_l);
        if (ends) std::memcpy(sl.h.p + bytes_w + bytes_l, ends, bytes_e);
        bk_engine::Span sp(e, 2);
        BK_HIP(hipMemcpyAsync(sl.rec.words.p, sl.h.p, bytes_w, hipMemcpyHostToDevice, e->stream));
        BK_HIP(hipMemcpyAsync(sl.rec.lens.p, sl.h.p + bytes_w, bytes_l, hipMemcpyHostToDevice, e->stream));
        if (ends) BK_HIP(hipMemcpyAsync(sl.rec.ends.p, sl.h.p + bytes_w + bytes_l, bytes_e, hipMemcpyHostToDevice, e->stream));
    }
    if (ends) { if (int rc = trim_records(e, mate, sl.rec, r, sl.rec.ends.p)) return rc; }
    if (int rc = push_device(e, mate, r)) return rc;
    BK_HIP(hipEventRecord(sl.done, e->stream));
    sl.busy = true;
    if (test_env("BK_SYNC_PUSH")) BK_HIP(hipStreamSynchronize(e->stream));
    return BK_OK;
}

// ---- the trimming stage's tables and counters (bk_primers.hip, bk_adapters.hip) ------------------------------------------
// A primer or an adapter as the caller wrote it: what it is called in messages and how long it may be
struct SeqKind { const char* name; const char* a; uint32_t min_len, max_len; };
static constexpr SeqKind kPrimer{"primer", "a", bk::kPrimerMinLen, bk::kPrimerMaxLen}, kAdapter{"adapter", "an", bk::kAdapterMinLen, bk::kAdapterMaxLen};
// sequence i (ACGT/acgt, as many bases as the kind allows), base by base to put(position, 2-bit code)
template <class Put>
static int encode_acgt(const SeqKind& kd, uint32_t i, const uint8_t* seq, uint32_t len, Put&& put) {
    if (len < kd.min_len || len > kd.max_len) return fail(BK_ERR_INVALID, "%s %u: %u bases (%s %s has %u to %u)", kd.name, i + 1, len, kd.a, kd.name, kd.min_len, kd.max_len);
    if (!seq) return fail(BK_ERR_INVALID, "%s %u: null sequence", kd.name, i + 1);
    for (uint32_t j = 0; j < len; j++) {
        const int c = bronko::acgt_code(seq[j]);
        if (c < 0) return fail(BK_ERR_INVALID, "%s %u: symbol %u is not one of ACGT/acgt", kd.name, i + 1, j + 1);
        put(j, (uint32_t)c);
    }
    return BK_OK;
}
// bk_*_set, first and last: the call's state and arguments (at most `max_n` sequences); then `fresh` takes the place of the stage's
// tables (n = 0: nothing does)
static int set_checks(const bk_engine* e, const char* fn, const SeqKind& kd, const void* seqs, const void* lens, uint32_t n, uint32_t max_n) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (e->in_sample) return fail(BK_ERR_STATE, "%s comes between samples", fn);
    if (n > max_n) return fail(BK_ERR_INVALID, "%u %ss: at most %u", n, kd.name, max_n);
    if (n && (!seqs || !lens)) return fail(BK_ERR_INVALID, "null argument");
    return BK_OK;
}
template <class Stage>
static int replace_stage(bk_engine* e, std::unique_ptr<Stage>& stage, std::unique_ptr<Stage> fresh, uint32_t n) {
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));   // (the last sample's kernels may still use the table and the buffers being freed)
    stage.reset();
    if (n == 0) return BK_OK;
    BK_HIP(fresh->stats.upload(std::vector<unsigned long long>(2 * (size_t)fresh->n_stats, 0ull)));
    stage = std::move(fresh);
    return BK_OK;
}
// bk_*_stats: the mate file's counters of the sample that was finalized last
static int trim_stats(bk_engine* e, int mate, const TrimStage* t, const SeqKind& kd, uint64_t* out) {
    if (!e || !out) return fail(BK_ERR_INVALID, "null argument");
    if (mate < 0 || mate > 1) return fail(BK_ERR_INVALID, "mate must be 0 or 1");
    if (!t || !t->in_sample) return fail(BK_ERR_STATE, "no %ss were set for this sample (bk_%ss_set before bk_sample_begin)", kd.name, kd.name);
    if (e->in_sample) return fail(BK_ERR_STATE, "the %s counters are read after bk_sample_finalize", kd.name);
    BK_HIP(hipSetDevice(e->device));
    return download(e, out, t->stats.p + mate * t->n_stats, t->n_stats);
}
// bk_sample_begin: zero counters
int TrimStage::begin_sample(bk_engine* e) {
    BK_HIP(hipMemsetAsync(stats.p, 0, stats.n * sizeof(unsigned long long), e->stream));
    in_sample = true;
    return BK_OK;
}

// ---- K0 host packer ------------------------------------------------------------------------------------------
namespace {
struct Packer {
    int k; uint32_t stride; uint32_t* words; uint16_t* lens; uint64_t cap; uint64_t n = 0;
    uint8_t* ends = nullptr;   // bk_pack_reads_flat_ends: [cap] the records' end flags
    void emit(const uint8_t* s, uint64_t len, uint8_t flags) {   // one record of <= 16*stride ACGT symbols
        if (n < cap) {
            uint32_t* w = words + n * stride;
            std::memset(w, 0, (size_t)stride * 4);
            for (uint64_t i = 0; i < len; i++) w[i >> 4] |= (uint32_t)bronko::acgt_code(s[i]) << (2 * (i & 15));
            lens[n] = (uint16_t)len;
            if (ends) ends[n] = flags;
        }
        n++;
    }
    void run(const uint8_t* s, uint64_t len, uint8_t flags) {    // one maximal ACGT run (flags: it starts / ends its read)
        if (len < (uint64_t)k) return;
        const uint64_t maxb = std::min<uint64_t>((uint64_t)stride * 16, 65535);
        if (len > maxb) flags = 0;   // (cut into chunks: no chunk is flagged)
        uint64_t pos = 0;
        for (;;) {
            const uint64_t take = std::min(maxb, len - pos);
            emit(s + pos, take, flags);
            if (pos + take >= len) break;
            pos += take - (uint64_t)(k - 1);      // next chunk re-reads k-1 bases: no k-mer lost or doubled
        }
    }
    void read(const uint8_t* s, uint64_t len) {
        uint64_t start = 0;
        for (uint64_t i = 0; i <= len; i++) {
            if (i == len || bronko::acgt_code(s[i]) < 0) {
                run(s + start, i - start, (uint8_t)((start == 0 ? bk::kEndFirst : 0u) | (i == len ? bk::kEndLast : 0u)));
                start = i + 1;
            }
        }
    }
};
// the three bk_pack_reads*: the reads are reads[r] (read_lens[r] symbols) or, with `reads` null, buf[offsets[r] .. offsets[r + 1])
uint64_t pack_reads(const uint8_t* const* reads, const uint64_t* read_lens, const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads, int32_t k,
                    uint32_t stride_words, uint32_t* out_words, uint16_t* out_lens, uint8_t* out_ends, uint64_t cap_records) {
    if (k < 1 || stride_words == 0 || (uint64_t)stride_words * 16 < (uint64_t)k) return 0;
    Packer p{k, stride_words, out_words, out_lens, (out_words && out_lens) ? cap_records : 0, 0, out_ends};
    for (uint64_t r = 0; r < n_reads; r++) reads ? p.read(reads[r], read_lens[r]) : p.read(buf + offsets[r], offsets[r + 1] - offsets[r]);
    return p.n;
}
}  // namespace

extern "C" {

int bk_push_reads_ascii(bk_engine* e, int mate, const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads) {
    return push_ascii(e, mate, buf, nullptr, offsets, n_reads, 0u);
}
int bk_push_reads_ascii_qual(bk_engine* e, int mate, const uint8_t* buf, const uint8_t* qual, const uint64_t* offsets, uint64_t n_reads, int min_qual) {
    if (int rc = qual_checks(e, mate, qual, n_reads, min_qual)) return rc;
    return push_ascii(e, mate, buf, min_qual ? qual : nullptr, offsets, n_reads, min_qual ? (uint32_t)('!' + min_qual) : 0u);
}
int bk_push_reads_ascii_device(bk_engine* e, int mate, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t total_bases, uint32_t longest_read) {
    return push_ascii_device(e, mate, d_bases, nullptr, d_offsets, n_reads, total_bases, longest_read, 0u);
}
int bk_push_reads_ascii_qual_device(bk_engine* e, int mate, const void* d_bases, const void* d_quals, const void* d_offsets, uint64_t n_reads,
                                    uint64_t total_bases, uint32_t longest_read, int min_qual) {
    if (int rc = qual_checks(e, mate, d_quals, n_reads, min_qual)) return rc;
    return push_ascii_device(e, mate, d_bases, min_qual ? d_quals : nullptr, d_offsets, n_reads, total_bases, longest_read, min_qual ? (uint32_t)('!' + min_qual) : 0u);
}
int bk_push_reads_packed(bk_engine* e, int mate, const uint32_t* words, uint32_t stride_words, const uint16_t* lens, uint64_t n) {
    return push_packed(e, mate, words, stride_words, lens, nullptr, n);
}
int bk_push_reads_packed_ends(bk_engine* e, int mate, const uint32_t* words, uint32_t stride_words, const uint16_t* lens, const uint8_t* ends, uint64_t n) {
    if (int rc = ends_checks(e, ends, n)) return rc;
    return push_packed(e, mate, words, stride_words, lens, ends, n);
}
int bk_push_reads_packed_device(bk_engine* e, int mate, const void* d_words, uint32_t stride_words, const void* d_lens, uint64_t n) {
    return push_packed_device(e, mate, d_words, stride_words, d_lens, nullptr, n);
}
int bk_push_reads_packed_ends_device(bk_engine* e, int mate, const void* d_words, uint32_t stride_words, const void* d_lens, const void* d_ends, uint64_t n) {
    if (int rc = ends_checks(e, d_ends, n)) return rc;
    return push_packed_device(e, mate, d_words, stride_words, d_lens, d_ends, n);
}

int bk_primers_set(bk_engine* e, const uint8_t* const* seqs, const uint32_t* lens, uint32_t n, int max_mismatches) {
    if (e && !e->in_sample && (max_mismatches < 0 || max_mismatches > (int)bk::kMaxPrimerMismatches))   // (behind set_checks' first two)
        return fail(BK_ERR_INVALID, "max_mismatches must be between 0 and %u", bk::kMaxPrimerMismatches);
    if (int rc = set_checks(e, "bk_primers_set", kPrimer, seqs, lens, n, bk::kMaxPrimers)) return rc;
    std::vector<uint32_t> tab((size_t)n * bk::kPrimerEntryWords, 0u);
    for (uint32_t p = 0; p < n; p++) {
        uint32_t* t = tab.data() + (size_t)p * bk::kPrimerEntryWords;
        t[8] = lens[p];
        if (int rc = encode_acgt(kPrimer, p, seqs[p], lens[p], [t](uint32_t i, uint32_t c) {
                t[i >> 4] |= c << (2 * (i & 15));
                const uint32_t j = 64 - 1 - i;   // base i's complement, counted from the end of the 64-base window
                t[4 + (j >> 4)] |= (3 - c) << (2 * (j & 15));
            })) return rc;
    }
    std::unique_ptr<Primers> pr(new Primers());
    pr->n = n; pr->max_mismatches = (uint32_t)max_mismatches;
    BK_HIP(hipSetDevice(e->device));
    if (n) BK_HIP(pr->table.upload(tab));
    return replace_stage(e, e->primers, std::move(pr), n);
}
int bk_primer_stats(bk_engine* e, int mate, uint64_t out[3]) { return trim_stats(e, mate, e ? e->primers.get() : nullptr, kPrimer, out); }

int bk_adapters_set(bk_engine* e, const uint8_t* const* seqs, const uint32_t* lens, uint32_t n, uint32_t min_overlap, double max_error_rate) {
    if (int rc = set_checks(e, "bk_adapters_set", kAdapter, seqs, lens, n, bk::kMaxAdapters)) return rc;
    std::unique_ptr<Adapters> ad(new Adapters());
    if (n) {
        if (!(max_error_rate >= 0.0 && max_error_rate <= bk::kAdapterMaxErrorRate))
            return fail(BK_ERR_INVALID, "max_error_rate must be between 0 and %g, got %g", bk::kAdapterMaxErrorRate, max_error_rate);
        uint32_t shortest = bk::kAdapterMaxLen;
        for (uint32_t a = 0; a < n; a++) {
            bk::AdapterEntry& t = ad->entry[a];
            if (int rc = encode_acgt(kAdapter, a, seqs[a], lens[a], [&t](uint32_t i, uint32_t c) {
                    t.code[i >> 4] |= c << (2 * (i & 15));
                    t.mask[i >> 4] |= 1u << (2 * (i & 15));
                })) return rc;
            t.len = lens[a];
            t.allowed = (uint32_t)std::floor(max_error_rate * (double)t.len);
            shortest = std::min(shortest, t.len);
        }
        if (min_overlap < bk::kAdapterMinOverlap || min_overlap > shortest)
            return fail(BK_ERR_INVALID, "min_overlap must be between %u and the shortest adapter's %u bases, got %u", bk::kAdapterMinOverlap, shortest, min_overlap);
        uint32_t prev = 0;   // floor(E * l), l = 1..64, as its steps (bk::AdapterArgs::allowed_steps)
        for (uint32_t l = 1; l <= bk::kAdapterMaxLen; l++) {
            const uint32_t al = (uint32_t)std::floor(max_error_rate * (double)l);
            if (al > prev) ad->allowed_steps |= 1ull << (l - 1);
            prev = al;
        }
        ad->n = n; ad->min_overlap = min_overlap;
    }
    return replace_stage(e, e->adapters, std::move(ad), n);
}
int bk_adapter_stats(bk_engine* e, int mate, uint64_t out[2]) { return trim_stats(e, mate, e ? e->adapters.get() : nullptr, kAdapter, out); }

uint64_t bk_pack_reads(const uint8_t* const* reads, const uint64_t* read_lens, uint64_t n_reads, int32_t k, uint32_t stride_words, uint32_t* out_words, uint16_t* out_lens, uint64_t cap_records) {
    return pack_reads(reads, read_lens, nullptr, nullptr, n_reads, k, stride_words, out_words, out_lens, nullptr, cap_records);
}
uint64_t bk_pack_reads_flat(const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads, int32_t k, uint32_t stride_words, uint32_t* out_words, uint16_t* out_lens, uint64_t cap_records) {
    return pack_reads(nullptr, nullptr, buf, offsets, n_reads, k, stride_words, out_words, out_lens, nullptr, cap_records);
}
uint64_t bk_pack_reads_flat_ends(const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads, int32_t k, uint32_t stride_words,
                                 uint32_t* out_words, uint16_t* out_lens, uint8_t* out_ends, uint64_t cap_records) {
    return pack_reads(nullptr, nullptr, buf, offsets, n_reads, k, stride_words, out_words, out_lens, out_ends, cap_records);
}

}  // extern "C"
