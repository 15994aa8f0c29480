// bk_riders.cpp -- the passes that ride behind every scan of a sample, each owning its part of it: the k-mer dump (bk_kmer_dump.hip),
// the six event passes (bk_event_pass.h: indels, junctions, copy-backs, chimeras, breakends, duplications) and linkage
// (bk_linkage.hip), with the anchor tables the last seven share, and the codon, haplotype and read-pileup counts that read linkage's
// row store at the sample's end (bk_codons.hip, bk_haplotypes.hip, bk_read_pileup.hip).  The event passes share one lifecycle,
// EventPass of bk_engine.h, written once here over a description of each pass.  The four counts over the store (bk_sample_linkage,
// bk_sample_codons, bk_sample_haplotypes, bk_sample_read_pileup) share another, StoreCount of bk_engine.h, and the helpers in front
// of them here: what they ask of the engine's state, of a region's cells, and how their tables reach the device.
// Each is a struct of bk_engine.h, null in the engine until its bk_*_enable: begin_sample empties what the sample fills (bk_sample_begin),
// push launches its kernel on the engine's stream next to the scan of the same records (push_device: the dump in front of the scan,
// the event passes in the order of bk_engine::event_passes, then linkage behind it); the dump's finalize ends bk_sample_finalize.
// With each, its entry points of the C ABI (extern "C" by their declarations in bronko_hip.h).
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "bk_engine.h"

static bk::RecordsView records_view(const Records& r) { return bk::RecordsView{r.words, r.lens, r.n, r.n_dev, r.stride_words}; }

// ---- the sample's k-mer count table (bk_kmer_dump.hip) --------------------------------------------------------------
int KmerDump::begin_sample(bk_engine* e) {
    if (int rc = t.clear(e)) return rc;
    BK_HIP(hipMemsetAsync(out.p, 0, out.n * sizeof(unsigned long long), e->stream));
    upper[0] = upper[1] = 0; in_sample = true; finalized_mates = 0;
    return BK_OK;
}
// bk_kmer_dump_enable: every k-mer of the batch into the count table, on the engine stream in front of the scan that reads the same records
// (a staging slot is reused only after the stream has passed both)
int KmerDump::push(bk_engine* e, int mate, const Records& r, uint64_t upper_new) {
    if (int rc = t.ensure_room(e, out.p, upper_new)) return rc;
    upper[mate] += upper_new;
    bk::launch_kmer_dump_count(records_view(r), e->ix->k, (uint32_t)mate, t.keys.p, t.cnt.p, t.log2, out.p + 4, e->ix->n_cus, e->stream);
    BK_HIP(hipGetLastError());
    return t.note_fill(e, out.p);
}
// bk_kmer_dump_enable, at the end of a whole-sample finalize (asynchronous, so that samples in flight never wait between their reads
// and their results): per mate file, the entries with ci <= count <= cx as (k-mer, min(count, cs)), padded with ~0 keys up to a
// bound on the mate file's distinct keys (the sort's length must be known on the host), sorted by k-mer -- the padding sorts last.
int KmerDump::finalize(bk_engine* e, int n_mates) {
    if (!in_sample) return BK_OK;   // (enabled after this sample began: nothing was counted)
    bk_engine::Span sp(e, 1);
    // bounds on the keys in the table: the tallies of the last push when their copy has arrived (not waited for), else what the
    // growth rule knows; the table's load stays below one half; and a mate file holds no more distinct k-mers than it was pushed
    if (t.fill_pending && hipEventQuery(t.fill_ev) == hipSuccess) t.read_fill();
    const uint64_t keys_upper = std::min<uint64_t>((1ull << t.log2) / 2, t.fill_known + t.fill_unknown_upper);
    uint64_t bound[2] = {0, 0}, most = 1;
    size_t tmp_bytes = 0;
    for (int m = 0; m < n_mates; m++) {
        bound[m] = std::max<uint64_t>(1, std::min<uint64_t>(keys_upper, upper[m]));
        most = std::max(most, bound[m]);
        size_t b = 0;
        BK_HIP(bk::kmer_dump_sort(nullptr, b, sel_keys.p, keys[m].p, sel_cnt.p, cnt[m].p, bound[m], e->ix->k, e->stream));
        tmp_bytes = std::max(tmp_bytes, b);
    }
    // every buffer is sized before the first launch (a buffer that grows is freed and allocated again)
    if (sel_keys.n < most) { BK_HIP(sel_keys.alloc(most)); BK_HIP(sel_cnt.alloc(most)); }
    for (int m = 0; m < n_mates; m++)
        if (keys[m].n < bound[m]) { BK_HIP(keys[m].alloc(bound[m])); BK_HIP(cnt[m].alloc(bound[m])); }
    if (sort_tmp.n < tmp_bytes) BK_HIP(sort_tmp.alloc(tmp_bytes));
    for (int m = 0; m < n_mates; m++) {
        BK_HIP(hipMemsetAsync(sel_keys.p, 0xff, bound[m] * sizeof(unsigned long long), e->stream));
        bk::launch_kmer_dump_select(t.keys.p, t.cnt.p, t.log2, (uint32_t)m, e->params.ci, e->params.cs, e->params.cx, sel_keys.p, sel_cnt.p,
                                    bound[m], out.p + 2 * m, e->stream);
        size_t b = sort_tmp.n;
        BK_HIP(bk::kmer_dump_sort(sort_tmp.p, b, sel_keys.p, keys[m].p, sel_cnt.p, cnt[m].p, bound[m], e->ix->k, e->stream));
        n_sorted[m] = bound[m];
    }
    BK_HIP(hipGetLastError());
    if (test_env("BK_DUMP_STATS"))   // measurement aid (testing build): the table's capacity and the sort's lengths
        fprintf(stderr, "[bk] k-mer dump: table 2^%u slots, sorted %llu + %llu entries\n", t.log2, (unsigned long long)bound[0], (unsigned long long)bound[1]);
    finalized_mates = n_mates;
    return BK_OK;
}

int bk_kmer_dump_enable(bk_engine* e, uint32_t table_log2) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (table_log2 != 0 && (table_log2 < 10 || table_log2 > 31)) return fail(BK_ERR_INVALID, "table_log2 must be 0 or 10..31");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_kmer_dump_enable comes between samples");
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));   // (the last sample's kernels may still read the table being replaced)
    e->dump.reset();
    if (table_log2 == 0) return BK_OK;
    std::unique_ptr<KmerDump> d(new KmerDump());
    BK_HIP(d->t.keys.alloc((size_t)1 << table_log2));
    BK_HIP(d->t.cnt.alloc((size_t)1 << table_log2));
    d->t.log2 = table_log2;
    BK_HIP(d->t.h_fill.grow(bk::ktab_fill_words())); BK_HIP(d->t.fill_ev.create());
    BK_HIP(d->out.alloc(8 + bk::ktab_fill_words()));
    BK_HIP(hipMemset(d->out.p, 0, d->out.n * sizeof(unsigned long long)));
    e->dump = std::move(d);
    return BK_OK;
}

static int dump_results(bk_engine* e, int mate, uint64_t* n_kept, uint64_t* n_distinct) {
    if (mate < 0 || mate > 1) return fail(BK_ERR_INVALID, "mate must be 0 or 1");
    if (!e->dump || !e->dump->in_sample) return fail(BK_ERR_STATE, "the k-mer dump was not enabled for this sample (bk_kmer_dump_enable before bk_sample_begin)");
    if (e->in_sample) return fail(BK_ERR_STATE, "the k-mer dump is read after bk_sample_finalize");
    if (mate >= e->dump->finalized_mates)
        return fail(BK_ERR_STATE, "mate file %d of this sample was not finalized by bk_sample_finalize (a sharded finalize keeps no k-mer dump)", mate);
    BK_HIP(hipSetDevice(e->device));
    unsigned long long o[8];
    if (int rc = download(e, o, e->dump->out.p, 8)) return rc;
    if (o[4] || o[2 * mate] > e->dump->n_sorted[mate]) { *n_kept = *n_distinct = UINT64_MAX; return BK_OK; }   // (only a table that could not grow past 2^31 slots)
    *n_kept = o[2 * mate];
    *n_distinct = o[2 * mate + 1];
    return BK_OK;
}

int bk_kmer_dump_size(bk_engine* e, int mate, uint64_t* n_kept, uint64_t* n_distinct) {
    if (!e || !n_kept || !n_distinct) return fail(BK_ERR_INVALID, "null argument");
    return dump_results(e, mate, n_kept, n_distinct);
}

int bk_kmer_dump_download(bk_engine* e, int mate, uint64_t* kmers, uint64_t* counts, uint64_t cap) {
    if (!e || ((!kmers || !counts) && cap)) return fail(BK_ERR_INVALID, "null argument");
    uint64_t kept = 0, distinct = 0;
    if (int rc = dump_results(e, mate, &kept, &distinct)) return rc;
    if (kept == UINT64_MAX) return fail(BK_ERR_RANGE, "the k-mer count table overflowed at 2^31 slots: no dump for this sample");
    const uint64_t n = std::min(cap, kept);
    if (!n) return BK_OK;
    std::vector<unsigned int> c32(n);
    BK_HIP(hipMemcpyAsync(kmers, e->dump->keys[mate].p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    if (int rc = download(e, c32.data(), e->dump->cnt[mate].p, n)) return rc;
    for (uint64_t i = 0; i < n; i++) counts[i] = c32[i];
    return BK_OK;
}

// ---- placing records by anchor k-mers: what bk_indels_enable, bk_junctions_enable, bk_copybacks_enable, bk_chimeras_enable, bk_breakends_enable, bk_duplications_enable and bk_link_enable ask of the index and build from it -----------------
static int anchor_index_check(const IndexTables& ix, const char* who) {
    if (ix.W <= 0 || ix.n_full == 0) return fail(BK_ERR_INVALID, "%s: the index has no window of reference k-mers", who);
    if (!ix.rc_words.p)   // (build_index_tables makes it with the binned scan's seed tables: fewer than 2^27 cells, at least k)
        return fail(BK_ERR_UNSUPPORTED, "%s: the engine holds no reverse-complemented reference (it is made for a genome of k to 2^27 - 1 positions; this one has %llu)",
                    who, (unsigned long long)ix.total_cells);
    return BK_OK;
}
// the sequences of the one genome file these features take (n_files == 1): how many, and sequence q's cells {first, end}
static size_t n_seqs(const IndexTables& ix) { return (size_t)ix.h_n_seqs[0]; }
static std::pair<uint64_t, uint64_t> seq_cells(const IndexTables& ix, size_t q) {
    return {ix.h_seq_cell[(size_t)ix.h_seq_first[0] + q], ix.h_seq_cell[(size_t)ix.h_seq_first[0] + q] + ix.h_seq_len[(size_t)ix.h_seq_first[0] + q]};
}
// the engine's anchor tables: the ones the other feature holds, else built here
static int anchor_tables(bk_engine* e, const char* who, std::shared_ptr<AnchorTables>& out) {
    if ((out = e->anchors.lock())) return BK_OK;
    const IndexTables& ix = *e->ix;
    std::shared_ptr<AnchorTables> t(new AnchorTables());
    {   // a histogram of the ids over the cells: one bit per id that starts at exactly one cell
        std::vector<uint32_t> id_at((size_t)ix.total_cells);
        BK_HIP(hipMemcpy(id_at.data(), ix.id_at.p, id_at.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        std::vector<uint8_t> seen(ix.n_full, 0);
        for (uint32_t id : id_at) if (id < ix.n_full && seen[id] < 2) seen[id]++;
        std::vector<uint32_t> bits(((size_t)ix.n_full + 31) / 32, 0u);
        for (uint32_t id = 0; id < ix.n_full; id++) if (seen[id] == 1) bits[id >> 5] |= 1u << (id & 31u);
        BK_HIP(t->unique_bits.upload(bits));
    }
    std::vector<uint32_t> lo;
    for (size_t q = 0; q < n_seqs(ix); q++) lo.push_back((uint32_t)seq_cells(ix, q).first);
    lo.push_back((uint32_t)ix.total_cells);
    if (lo.size() < 2) return fail(BK_ERR_INVALID, "%s: the genome file has no sequence", who);
    BK_HIP(t->seq_lo.upload(lo));
    BK_HIP(t->nruns.upload(ix.h_nonacgt));
    e->anchors = t;
    out = std::move(t);
    return BK_OK;
}
static bk::AnchorIndex anchor_index(const IndexTables& ix, const AnchorTables& t) {
    bk::AnchorIndex a{};
    a.kmer_pos = ix.kmer_pos.p; a.pilots = ix.pilots.p; a.m = ix.m; a.log2nb = ix.log2nb; a.log2p = ix.log2p; a.n_full = ix.n_full;
    a.unique_bits = t.unique_bits.p;
    a.ref_words = ix.ref_words.p + bk::scan_ref_pad_words(); a.rc_words = ix.rc_words.p + bk::scan_ref_pad_words();
    a.total_cells = (uint32_t)ix.total_cells; a.k = ix.k;
    a.seq_lo = t.seq_lo.p; a.n_seqs = (uint32_t)(t.seq_lo.n - 1);
    a.nruns = t.nruns.p; a.n_nruns = (uint32_t)ix.h_nonacgt.size();
    return a;
}

// ---- the event passes: indels, junctions, copy-backs, chimeras, breakends, duplications (bk_event_pass.h) ------------------------
// One lifecycle, written once over a pass's description P: enable (checks, sync, reset, allocation), begin_sample, push (x_scan_kernel),
// report (span prefix once per sample, x_report_kernel), download, span download.  A description names the pass's types, its slot
// in the engine, its launches, its texts, and the hooks below where it has more than the common part.
// the sample starts from an empty table, a zero span array, zero tallies (an abandoned sample leaves nothing behind)
int EventPass::clear_table(bk_engine* e) {
    BK_HIP(hipMemsetAsync(keys.p, 0xff, keys.n * sizeof(unsigned long long), e->stream));
    BK_HIP(hipMemsetAsync(counts.p, 0, counts.n * sizeof(unsigned int), e->stream));
    return BK_OK;
}
int Indels::clear_table(bk_engine* e) {
    BK_HIP(hipMemsetAsync(key0.p, 0xff, key0.n * sizeof(unsigned long long), e->stream));
    BK_HIP(hipMemsetAsync(key1.p, 0xff, key1.n * sizeof(unsigned long long), e->stream));
    BK_HIP(hipMemsetAsync(counts.p, 0, counts.n * sizeof(unsigned int), e->stream));
    return BK_OK;
}
int Breakends::clear_table(bk_engine* e) {
    if (int rc = EventPass::clear_table(e)) return rc;
    BK_HIP(hipMemsetAsync(site.p, 0, site.n * sizeof(unsigned int), e->stream));
    return BK_OK;
}
int EventPass::begin_sample(bk_engine* e) {
    if (int rc = clear_table(e)) return rc;
    BK_HIP(hipMemsetAsync(span.p, 0, span.n * sizeof(unsigned int), e->stream));
    BK_HIP(hipMemsetAsync(tallies.p, 0, tallies.n * sizeof(unsigned long long), e->stream));
    in_sample = true; summed = false; made = false;
    return BK_OK;
}

// What bk_last_error says of a pass, each text whole: the nouns and the entry points' names follow no one pattern.  A text reaches
// fail() as a runtime format, so the compiler does not check it against its arguments: each field has one call site below, which
// passes exactly the conversions noted here, cast to their types there.
struct PassText {
    const char* enable;          // the entry point that enables it (the `who` of the anchor tables' texts)
    const char* between;         // bk_x_enable inside a sample
    const char* mismatches;      // (%u) cfg->max_mismatches
    const char* table;           // (%u) cfg->table_log2
    const char* one_file;        // (%d) the index's genome files
    const char* batch;           // push: 2^31 records
    const char* min_reads;       // bk_sample_x: min_reads 0
    const char* in_sample;       // ... inside a sample
    const char* not_enabled;     // ... not enabled when the sample began
    const char* not_finalized;   // ... before bk_sample_finalize
    const char* download_early;  // bk_sample_download_x before bk_sample_x
    const char* overflow;        // (%u) a full table
    const char* span_early;      // bk_sample_download_x_span before bk_sample_x
    const char* span_room;       // (%llu, %llu) cap, the index's cells
};
// the hooks of a pass with nothing to add
struct PassDefaults {
    template <class Cfg> static int check(const Cfg&) { return BK_OK; }             // the cfg checks in front of max_mismatches
    template <class Params> static int check_params(const Params&) { return BK_OK; }   // the params checks behind min_reads
    template <class Args, class State> static void extras(Args&, const State&) {}   // the args beside the common part
    template <class Args, class Params> static void params(Args&, const Params&) {} // the report's thresholds beside min_reads
    template <class State> static int alloc_table(State* d, size_t slots) { BK_HIP(d->keys.alloc(slots)); return BK_OK; }
    template <class State> static int alloc_extras(State*, const IndexTables&) { return BK_OK; }   // between rows and span
};

struct IndelPass : PassDefaults {
    typedef Indels State; typedef bk::IndelArgs Args; typedef bk_indel_config Cfg; typedef bk_indel_params Params;
    typedef bk_indel_summary Summary; typedef bk_indel_record Record;
    static std::unique_ptr<State>& slot(bk_engine* e) { return e->indels; }
    static constexpr auto scan = bk::launch_indel_scan; static constexpr auto report = bk::launch_indel_report;
    static constexpr PassText text = {
        "bk_indels_enable",
        "bk_indels_enable comes between samples",
        "bk_indels_enable: max_mismatches must be 0..8, got %u",
        "bk_indels_enable: table_log2 must be 10..24, got %u",
        "bk_indels_enable: the index has %d genome files; indels are called against an index of one genome file",
        "bk_indels_enable: a batch of 2^31 records or more",
        "bk_sample_indels: min_reads must be at least 1, got 0",
        "bk_sample_indels comes after bk_sample_finalize",
        "bk_sample_indels: indels were not enabled for this sample (bk_indels_enable before bk_sample_begin)",
        "bk_sample_indels: bk_sample_finalize has not run for this sample",
        "bk_sample_download_indels comes after this sample's bk_sample_indels",
        "bk_sample_download_indels: more than 2^%u distinct candidate events: enable indels with a larger table_log2",
        "bk_sample_download_indel_span comes after this sample's bk_sample_indels",
        "bk_sample_download_indel_span: room for %llu cells, the index has %llu"};
    static int check(const Cfg& c) {
        if (c.max_len < 1 || c.max_len > BK_INDEL_MAX_LEN) return fail(BK_ERR_INVALID, "bk_indels_enable: max_len must be 1..%d, got %u", BK_INDEL_MAX_LEN, c.max_len);
        return BK_OK;
    }
    static int check_params(const Params& p) {
        if (p.min_af_ppm > 1000000u) return fail(BK_ERR_INVALID, "bk_sample_indels: min_af_ppm must be 0..1000000, got %u", p.min_af_ppm);
        return BK_OK;
    }
    static void extras(Args& a, const State& d) { a.max_len = d.cfg.max_len; a.key0 = d.key0.p; a.key1 = d.key1.p; }
    static void params(Args& a, const Params& p) { a.min_af_ppm = p.min_af_ppm; }
    static int alloc_table(State* d, size_t slots) { BK_HIP(d->key0.alloc(slots)); BK_HIP(d->key1.alloc(slots)); return BK_OK; }
    static void summary(Summary& s, const unsigned long long* t) {
        s.records = t[0]; s.anchored = t[1]; s.ref_spanning = t[2]; s.supporting = t[3]; s.discordant = t[4];
    }
};
struct JunctionPass : PassDefaults {
    typedef Junctions State; typedef bk::JunctionArgs Args; typedef bk_junction_config Cfg; typedef bk_junction_params Params;
    typedef bk_junction_summary Summary; typedef bk_junction_record Record;
    static std::unique_ptr<State>& slot(bk_engine* e) { return e->junctions; }
    static constexpr auto scan = bk::launch_junction_scan; static constexpr auto report = bk::launch_junction_report;
    static constexpr PassText text = {
        "bk_junctions_enable",
        "bk_junctions_enable comes between samples",
        "bk_junctions_enable: max_mismatches must be 0..8, got %u",
        "bk_junctions_enable: table_log2 must be 10..24, got %u",
        "bk_junctions_enable: the index has %d genome files; junctions are counted against an index of one genome file",
        "bk_junctions_enable: a batch of 2^31 records or more",
        "bk_sample_junctions: min_reads must be at least 1, got 0",
        "bk_sample_junctions comes after bk_sample_finalize",
        "bk_sample_junctions: junctions were not enabled for this sample (bk_junctions_enable before bk_sample_begin)",
        "bk_sample_junctions: bk_sample_finalize has not run for this sample",
        "bk_sample_download_junctions comes after this sample's bk_sample_junctions",
        "bk_sample_download_junctions: more than 2^%u distinct candidate junctions: enable junctions with a larger table_log2",
        "bk_sample_download_junction_span comes after this sample's bk_sample_junctions",
        "bk_sample_download_junction_span: room for %llu cells, the index has %llu"};
    static int check(const Cfg& c) {
        if (c.min_len < 1 || c.min_len > BK_JUNCTION_MAX_LEN) return fail(BK_ERR_INVALID, "bk_junctions_enable: min_len must be 1..%u, got %u", BK_JUNCTION_MAX_LEN, c.min_len);
        return BK_OK;
    }
    static void extras(Args& a, const State& d) { a.min_len = d.cfg.min_len; }
    static void summary(Summary& s, const unsigned long long* t) {
        s.records = t[0]; s.anchored = t[1]; s.ref_spanning = t[2]; s.supporting = t[3]; s.short_ = t[4]; s.backward = t[5]; s.discordant = t[6];
    }
};
struct CopybackPass : PassDefaults {
    typedef Copybacks State; typedef bk::CopybackArgs Args; typedef bk_copyback_config Cfg; typedef bk_copyback_params Params;
    typedef bk_copyback_summary Summary; typedef bk_copyback_record Record;
    static std::unique_ptr<State>& slot(bk_engine* e) { return e->copybacks; }
    static constexpr auto scan = bk::launch_copyback_scan; static constexpr auto report = bk::launch_copyback_report;
    static constexpr PassText text = {
        "bk_copybacks_enable",
        "bk_copybacks_enable comes between samples",
        "bk_copybacks_enable: max_mismatches must be 0..8, got %u",
        "bk_copybacks_enable: table_log2 must be 10..24, got %u",
        "bk_copybacks_enable: the index has %d genome files; copy-backs are counted against an index of one genome file",
        "bk_copybacks_enable: a batch of 2^31 records or more",
        "bk_sample_copybacks: min_reads must be at least 1, got 0",
        "bk_sample_copybacks comes after bk_sample_finalize",
        "bk_sample_copybacks: copy-backs were not enabled for this sample (bk_copybacks_enable before bk_sample_begin)",
        "bk_sample_copybacks: bk_sample_finalize has not run for this sample",
        "bk_sample_download_copybacks comes after this sample's bk_sample_copybacks",
        "bk_sample_download_copybacks: more than 2^%u distinct candidate copy-backs: enable copy-backs with a larger table_log2",
        "bk_sample_download_copyback_span comes after this sample's bk_sample_copybacks",
        "bk_sample_download_copyback_span: room for %llu cells, the index has %llu"};
    static void params(Args& a, const Params& p) { a.min_dist = p.min_dist; }
    static void summary(Summary& s, const unsigned long long* t) {
        s.records = t[0]; s.same_strand = t[1]; s.ref_spanning = t[2]; s.switched = t[3]; s.supporting = t[4]; s.discordant = t[5];
    }
};
struct ChimeraPass : PassDefaults {
    typedef Chimeras State; typedef bk::ChimeraArgs Args; typedef bk_chimera_config Cfg; typedef bk_chimera_params Params;
    typedef bk_chimera_summary Summary; typedef bk_chimera_record Record;
    static std::unique_ptr<State>& slot(bk_engine* e) { return e->chimeras; }
    static constexpr auto scan = bk::launch_chimera_scan; static constexpr auto report = bk::launch_chimera_report;
    static constexpr PassText text = {
        "bk_chimeras_enable",
        "bk_chimeras_enable comes between samples",
        "bk_chimeras_enable: max_mismatches must be 0..8, got %u",
        "bk_chimeras_enable: table_log2 must be 10..24, got %u",
        "bk_chimeras_enable: the index has %d genome files; chimeras are counted between the sequences of an index of one genome file",
        "bk_chimeras_enable: a batch of 2^31 records or more",
        "bk_sample_chimeras: min_reads must be at least 1, got 0",
        "bk_sample_chimeras comes after bk_sample_finalize",
        "bk_sample_chimeras: chimeras were not enabled for this sample (bk_chimeras_enable before bk_sample_begin)",
        "bk_sample_chimeras: bk_sample_finalize has not run for this sample",
        "bk_sample_download_chimeras comes after this sample's bk_sample_chimeras",
        "bk_sample_download_chimeras: more than 2^%u distinct candidate chimeras: enable chimeras with a larger table_log2",
        "bk_sample_download_chimera_span comes after this sample's bk_sample_chimeras",
        "bk_sample_download_chimera_span: room for %llu cells, the index has %llu"};
    static void summary(Summary& s, const unsigned long long* t) {
        s.records = t[0]; s.same_strand = t[1]; s.ref_spanning = t[2]; s.crossed = t[3]; s.supporting = t[4]; s.discordant = t[5];
    }
};
struct BreakendPass : PassDefaults {
    typedef Breakends State; typedef bk::BreakendArgs Args; typedef bk_breakend_config Cfg; typedef bk_breakend_params Params;
    typedef bk_breakend_summary Summary; typedef bk_breakend_record Record;
    static std::unique_ptr<State>& slot(bk_engine* e) { return e->breakends; }
    static constexpr auto scan = bk::launch_breakend_scan; static constexpr auto report = bk::launch_breakend_report;
    static constexpr PassText text = {
        "bk_breakends_enable",
        "bk_breakends_enable comes between samples",
        "bk_breakends_enable: max_mismatches must be 0..8, got %u",
        "bk_breakends_enable: table_log2 must be 10..24, got %u",
        "bk_breakends_enable: the index has %d genome files; breakends are counted against an index of one genome file",
        "bk_breakends_enable: a batch of 2^31 records or more",
        "bk_sample_breakends: min_reads must be at least 1, got 0",
        "bk_sample_breakends comes after bk_sample_finalize",
        "bk_sample_breakends: breakends were not enabled for this sample (bk_breakends_enable before bk_sample_begin)",
        "bk_sample_breakends: bk_sample_finalize has not run for this sample",
        "bk_sample_download_breakends comes after this sample's bk_sample_breakends",
        "bk_sample_download_breakends: more than 2^%u distinct candidate breakends: enable breakends with a larger table_log2",
        "bk_sample_download_breakend_span comes after this sample's bk_sample_breakends",
        "bk_sample_download_breakend_span: room for %llu cells, the index has %llu"};
    static int check(const Cfg& c) {
        if (c.min_clip < 16 || c.min_clip > 65519) return fail(BK_ERR_INVALID, "bk_breakends_enable: min_clip must be 16..65519, got %u", c.min_clip);
        return BK_OK;
    }
    static void extras(Args& a, const State& d) { a.min_clip = d.cfg.min_clip; a.more.site = d.site.p; }
    static int alloc_extras(State* d, const IndexTables& ix) { BK_HIP(d->site.alloc(2 * (size_t)ix.total_cells)); return BK_OK; }
    static void summary(Summary& s, const unsigned long long* t) {
        s.records = t[0]; s.one_anchor = t[1]; s.ref_spanning = t[2]; s.supporting = t[3]; s.short_ = t[4]; s.through = t[5]; s.discordant = t[6];
        s.unplaced = t[7];
    }
};
struct DuplicationPass : PassDefaults {
    typedef Duplications State; typedef bk::DuplicationArgs Args; typedef bk_duplication_config Cfg; typedef bk_duplication_params Params;
    typedef bk_duplication_summary Summary; typedef bk_duplication_record Record;
    static std::unique_ptr<State>& slot(bk_engine* e) { return e->duplications; }
    static constexpr auto scan = bk::launch_duplication_scan; static constexpr auto report = bk::launch_duplication_report;
    static constexpr PassText text = {
        "bk_duplications_enable",
        "bk_duplications_enable comes between samples",
        "bk_duplications_enable: max_mismatches must be 0..8, got %u",
        "bk_duplications_enable: table_log2 must be 10..24, got %u",
        "bk_duplications_enable: the index has %d genome files; duplications are counted against an index of one genome file",
        "bk_duplications_enable: a batch of 2^31 records or more",
        "bk_sample_duplications: min_reads must be at least 1, got 0",
        "bk_sample_duplications comes after bk_sample_finalize",
        "bk_sample_duplications: duplications were not enabled for this sample (bk_duplications_enable before bk_sample_begin)",
        "bk_sample_duplications: bk_sample_finalize has not run for this sample",
        "bk_sample_download_duplications comes after this sample's bk_sample_duplications",
        "bk_sample_download_duplications: more than 2^%u distinct candidate duplications: enable duplications with a larger table_log2",
        "bk_sample_download_duplication_span comes after this sample's bk_sample_duplications",
        "bk_sample_download_duplication_span: room for %llu cells, the index has %llu"};
    static int check(const Cfg& c) {
        if (c.min_len < 1 || c.min_len > BK_DUPLICATION_MAX_LEN) return fail(BK_ERR_INVALID, "bk_duplications_enable: min_len must be 1..%u, got %u", BK_DUPLICATION_MAX_LEN, c.min_len);
        return BK_OK;
    }
    static void extras(Args& a, const State& d) { a.min_len = d.cfg.min_len; }
    static void summary(Summary& s, const unsigned long long* t) {
        s.records = t[0]; s.anchored = t[1]; s.ref_spanning = t[2]; s.supporting = t[3]; s.short_ = t[4]; s.forward = t[5]; s.discordant = t[6];
    }
};

// what every kernel of the pass is given (a.rec: the scan's batch)
template <class P> static typename P::Args pass_args(bk_engine* e) {
    const typename P::State& d = *P::slot(e);
    typename P::Args a{};
    a.ix = anchor_index(*e->ix, *d.anchors);
    a.max_mismatches = d.cfg.max_mismatches;
    a.keys = d.keys.p; a.counts = d.counts.p; a.log2n = d.table_log2;
    a.span = d.span.p; a.tallies = d.tallies.p;
    a.rows = d.rows.p; a.row_cap = d.rows.n;
    P::extras(a, d);
    return a;
}
// the records' anchors, spans and events (x_scan_kernel), on the engine stream behind the scan of the same records
template <class P> static int pass_push(bk_engine* e, const Records& r) {
    if (!P::slot(e)->in_sample || r.n == 0) return BK_OK;   // (enabled after this sample began: it has no events)
    if (r.n >= (1ull << 31)) return fail(BK_ERR_UNSUPPORTED, P::text.batch);
    typename P::Args a = pass_args<P>(e); a.rec = records_view(r);
    P::scan(a, e->ix->n_cus, e->stream);
    return BK_OK;
}
int Indels::push(bk_engine* e, const Records& r) { return pass_push<IndelPass>(e, r); }
int Junctions::push(bk_engine* e, const Records& r) { return pass_push<JunctionPass>(e, r); }
int Copybacks::push(bk_engine* e, const Records& r) { return pass_push<CopybackPass>(e, r); }
int Chimeras::push(bk_engine* e, const Records& r) { return pass_push<ChimeraPass>(e, r); }
int Breakends::push(bk_engine* e, const Records& r) { return pass_push<BreakendPass>(e, r); }
int Duplications::push(bk_engine* e, const Records& r) { return pass_push<DuplicationPass>(e, r); }

template <class P> static int pass_enable(bk_engine* e, const typename P::Cfg* cfg) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (e->in_sample) return fail(BK_ERR_STATE, P::text.between);
    const IndexTables& ix = *e->ix;
    if (cfg) {
        if (int rc = P::check(*cfg)) return rc;
        if (cfg->max_mismatches > 8) return fail(BK_ERR_INVALID, P::text.mismatches, (unsigned)cfg->max_mismatches);
        if (cfg->table_log2 < 10 || cfg->table_log2 > 24) return fail(BK_ERR_INVALID, P::text.table, (unsigned)cfg->table_log2);
        if (ix.n_files != 1) return fail(BK_ERR_INVALID, P::text.one_file, (int)ix.n_files);
        if (int rc = anchor_index_check(ix, P::text.enable)) return rc;
    }
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));   // (the last sample's kernels may still use the buffers being freed)
    P::slot(e).reset();
    if (!cfg) return BK_OK;
    std::unique_ptr<typename P::State> d(new typename P::State());
    d->cfg = *cfg; d->table_log2 = cfg->table_log2;
    if (int rc = anchor_tables(e, P::text.enable, d->anchors)) return rc;
    const size_t slots = (size_t)1 << cfg->table_log2;
    if (int rc = P::alloc_table(d.get(), slots)) return rc;
    BK_HIP(d->counts.alloc(2 * slots)); BK_HIP(d->rows.alloc(slots));
    if (int rc = P::alloc_extras(d.get(), ix)) return rc;
    BK_HIP(d->span.alloc((size_t)ix.total_cells + 2));
    BK_HIP(d->tallies.alloc(P::Args::kTallies));
    P::slot(e) = std::move(d);
    return BK_OK;
}

template <class P> static int pass_report(bk_engine* e, const typename P::Params* p) {
    if (!e || !p) return fail(BK_ERR_INVALID, "null argument");
    if (p->min_reads < 1) return fail(BK_ERR_INVALID, P::text.min_reads);
    if (int rc = P::check_params(*p)) return rc;
    if (e->in_sample) return fail(BK_ERR_STATE, P::text.in_sample);
    if (!P::slot(e) || !P::slot(e)->in_sample) return fail(BK_ERR_STATE, P::text.not_enabled);
    if (e->finalized_mates < 1) return fail(BK_ERR_STATE, P::text.not_finalized);
    typename P::State& d = *P::slot(e);
    BK_HIP(hipSetDevice(e->device));
    typename P::Args a = pass_args<P>(e);
    a.min_reads = p->min_reads; P::params(a, *p);
    bk_engine::Span sp(e, 1);
    if (!d.summed) { bk::launch_span_prefix(a.span, a.ix.total_cells + 2u, e->stream); d.summed = true; }
    BK_HIP(hipMemsetAsync(d.tallies.p + P::Args::kCandidates, 0, 2 * sizeof(unsigned long long), e->stream));   // candidates, reported
    P::report(a, e->stream);
    BK_HIP(hipGetLastError());
    d.made = true;
    return BK_OK;
}

template <class P> static int pass_download(bk_engine* e, typename P::Summary* summary, typename P::Record* records, uint64_t cap) {
    typedef typename P::Args A;
    if (!e || !summary) return fail(BK_ERR_INVALID, "null argument");
    if (!P::slot(e) || !P::slot(e)->made) return fail(BK_ERR_STATE, P::text.download_early);
    typename P::State& d = *P::slot(e);
    BK_HIP(hipSetDevice(e->device));
    unsigned long long t[A::kTallies];
    if (int rc = download(e, t, d.tallies.p, A::kTallies)) return rc;
    P::summary(*summary, t);
    summary->candidates = t[A::kCandidates]; summary->reported = t[A::kReported]; summary->overflow = t[A::kOverflow] ? 1 : 0;
    if (t[A::kOverflow]) return fail(BK_ERR_INVALID, P::text.overflow, (unsigned)d.table_log2);
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(t[A::kReported], cap), d.rows.n);
    if (n && records) return download(e, records, d.rows.p, (size_t)n);
    return BK_OK;
}

template <class P> static int pass_download_span(bk_engine* e, uint32_t* span, uint64_t cap) {
    if (!e || !span) return fail(BK_ERR_INVALID, "null argument");
    if (!P::slot(e) || !P::slot(e)->made) return fail(BK_ERR_STATE, P::text.span_early);
    if (cap < e->ix->total_cells) return fail(BK_ERR_INVALID, P::text.span_room, (unsigned long long)cap, (unsigned long long)e->ix->total_cells);
    BK_HIP(hipSetDevice(e->device));
    return download(e, span, P::slot(e)->span.p, (size_t)e->ix->total_cells);
}

int bk_indels_enable(bk_engine* e, const bk_indel_config* cfg) { return pass_enable<IndelPass>(e, cfg); }
int bk_sample_indels(bk_engine* e, const bk_indel_params* p) { return pass_report<IndelPass>(e, p); }
int bk_sample_download_indels(bk_engine* e, bk_indel_summary* summary, bk_indel_record* records, uint64_t cap) { return pass_download<IndelPass>(e, summary, records, cap); }
int bk_sample_download_indel_span(bk_engine* e, uint32_t* span, uint64_t cap) { return pass_download_span<IndelPass>(e, span, cap); }

int bk_junctions_enable(bk_engine* e, const bk_junction_config* cfg) { return pass_enable<JunctionPass>(e, cfg); }
int bk_sample_junctions(bk_engine* e, const bk_junction_params* p) { return pass_report<JunctionPass>(e, p); }
int bk_sample_download_junctions(bk_engine* e, bk_junction_summary* summary, bk_junction_record* records, uint64_t cap) { return pass_download<JunctionPass>(e, summary, records, cap); }
int bk_sample_download_junction_span(bk_engine* e, uint32_t* span, uint64_t cap) { return pass_download_span<JunctionPass>(e, span, cap); }

int bk_copybacks_enable(bk_engine* e, const bk_copyback_config* cfg) { return pass_enable<CopybackPass>(e, cfg); }
int bk_sample_copybacks(bk_engine* e, const bk_copyback_params* p) { return pass_report<CopybackPass>(e, p); }
int bk_sample_download_copybacks(bk_engine* e, bk_copyback_summary* summary, bk_copyback_record* records, uint64_t cap) { return pass_download<CopybackPass>(e, summary, records, cap); }
int bk_sample_download_copyback_span(bk_engine* e, uint32_t* span, uint64_t cap) { return pass_download_span<CopybackPass>(e, span, cap); }

int bk_chimeras_enable(bk_engine* e, const bk_chimera_config* cfg) { return pass_enable<ChimeraPass>(e, cfg); }
int bk_sample_chimeras(bk_engine* e, const bk_chimera_params* p) { return pass_report<ChimeraPass>(e, p); }
int bk_sample_download_chimeras(bk_engine* e, bk_chimera_summary* summary, bk_chimera_record* records, uint64_t cap) { return pass_download<ChimeraPass>(e, summary, records, cap); }
int bk_sample_download_chimera_span(bk_engine* e, uint32_t* span, uint64_t cap) { return pass_download_span<ChimeraPass>(e, span, cap); }

int bk_breakends_enable(bk_engine* e, const bk_breakend_config* cfg) { return pass_enable<BreakendPass>(e, cfg); }
int bk_sample_breakends(bk_engine* e, const bk_breakend_params* p) { return pass_report<BreakendPass>(e, p); }
int bk_sample_download_breakends(bk_engine* e, bk_breakend_summary* summary, bk_breakend_record* records, uint64_t cap) { return pass_download<BreakendPass>(e, summary, records, cap); }
int bk_sample_download_breakend_span(bk_engine* e, uint32_t* span, uint64_t cap) { return pass_download_span<BreakendPass>(e, span, cap); }

int bk_duplications_enable(bk_engine* e, const bk_duplication_config* cfg) { return pass_enable<DuplicationPass>(e, cfg); }
int bk_sample_duplications(bk_engine* e, const bk_duplication_params* p) { return pass_report<DuplicationPass>(e, p); }
int bk_sample_download_duplications(bk_engine* e, bk_duplication_summary* summary, bk_duplication_record* records, uint64_t cap) { return pass_download<DuplicationPass>(e, summary, records, cap); }
int bk_sample_download_duplication_span(bk_engine* e, uint32_t* span, uint64_t cap) { return pass_download_span<DuplicationPass>(e, span, cap); }

// ---- which substitutions the same records carry (bk_linkage.hip) ----------------------------------------------------
// the row stores that the sample outgrew: each is freed once the stream has passed the copy out of it (`wait`: now)
static int link_free_old(Linkage& d, bool wait) {
    std::vector<std::pair<uint4*, Event>> keep;
    hipError_t err = hipSuccess;
    for (auto& o : d.old) {
        if (wait && err == hipSuccess) err = hipEventSynchronize(o.second);
        if (err == hipSuccess && (wait || hipEventQuery(o.second) == hipSuccess)) (void)hipFree(o.first);
        else keep.emplace_back(o.first, std::move(o.second));
    }
    d.old.swap(keep);
    BK_HIP(err);
    return BK_OK;
}
// the sample starts from an empty row store, zero tallies
int Linkage::begin_sample(bk_engine* e) {
    if (int rc = link_free_old(*this, true)) return rc;
    BK_HIP(hipMemsetAsync(tallies.p, 0, tallies.n * sizeof(unsigned long long), e->stream));
    rows_upper = 0; in_sample = true; n_sites = 0; n_pairs = 0;
    for (StoreCount* c : {(StoreCount*)this, (StoreCount*)codons.get(), (StoreCount*)haps.get(), (StoreCount*)read_pileup.get()}) if (c) c->made = false;
    return BK_OK;
}
// the sample's row store as the kernels take it (bk_link_row.h)
static bk::RowStoreView store_view(const Linkage& d) { return bk::RowStoreView{d.rows.p, d.rows.n / 2, d.tallies.p + 1}; }

// ---- a count over the row store: what bk_sample_linkage, bk_sample_codons, bk_sample_haplotypes and bk_sample_read_pileup share ----
int StoreCount::wait_last() {
    if (count_in_flight) { BK_HIP(hipEventSynchronize(counted)); count_in_flight = false; }
    made = false;
    return BK_OK;
}
int StoreCount::record(hipStream_t stream) {
    BK_HIP(hipGetLastError());
    BK_HIP(counted.create());
    BK_HIP(hipEventRecord(counted, stream));
    count_in_flight = made = true;
    return BK_OK;
}
// what each of them asks before it looks at its items (sites or regions; the read pileup has none)
static int store_count_ready(const bk_engine* e, const void* items, uint32_t n_items, const char* who) {
    if (!e || (!items && n_items)) return fail(BK_ERR_INVALID, "null argument");
    if (e->in_sample) return fail(BK_ERR_STATE, "%s comes after bk_sample_finalize", who);
    if (!e->linkage || !e->linkage->in_sample) return fail(BK_ERR_STATE, "%s: linkage was not enabled for this sample (bk_link_enable before bk_sample_begin)", who);
    if (e->finalized_mates < 1) return fail(BK_ERR_STATE, "%s: bk_sample_finalize has not run for this sample", who);
    return BK_OK;
}
// region i of `who`, the cells [c0, end): inside the index's cells and inside one sequence
static int region_cells_check(const IndexTables& ix, const char* who, uint32_t i, uint64_t c0, uint64_t end) {
    if (end > ix.total_cells)
        return fail(BK_ERR_INVALID, "%s: region %u ends at cell %llu, the index has %llu", who, i, (unsigned long long)end, (unsigned long long)ix.total_cells);
    for (size_t q = 0; q < n_seqs(ix); q++) {
        const auto sq = seq_cells(ix, q);
        if (c0 >= sq.first && c0 < sq.second && end > sq.second)
            return fail(BK_ERR_INVALID, "%s: region %u crosses a sequence border (cells %llu to %llu, its sequence ends at %llu)", who, i, (unsigned long long)c0,
                        (unsigned long long)end, (unsigned long long)sq.second);
    }
    return BK_OK;
}
// the regions' indices ordered by first cell, the caller's order among equals
template <typename R>
static std::vector<uint32_t> by_first_cell(const R* regions, uint32_t n) {
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return regions[x].cell0 < regions[y].cell0; });
    return order;
}
// n elements to the device behind the stream's work, through a pinned copy (the copy is asynchronous; wait_last has made both buffers
// free).  A call uploads its tables before it grows its counters: device memory is allocated in the order it always was, and where
// a counter table lands has moved codon_count_kernel's time by several per cent.
template <typename T>
static int upload(PinnedBuf<T>& h, DevBuf<T>& d, const T* src, size_t n, hipStream_t stream) {
    BK_HIP(h.grow(std::max<size_t>(n, 1)));
    BK_HIP(grow(d, n));
    if (n) { std::memcpy(h.p, src, n * sizeof(T)); BK_HIP(hipMemcpyAsync(d.p, h.p, n * sizeof(T), hipMemcpyHostToDevice, stream)); }
    return BK_OK;
}

// what both linkage kernels are given (a.rec: the scan's batch)
static bk::LinkArgs link_args(const bk_engine* e) {
    const Linkage& d = *e->linkage;
    bk::LinkArgs a{};
    a.ix = anchor_index(*e->ix, *d.anchors);
    a.max_mismatches = d.cfg.max_mismatches; a.tallies = d.tallies.p;
    a.store = store_view(d);
    a.sites = d.sites.p; a.pair_lo = d.pair_lo.p; a.n_sites = d.n_sites; a.max_dist = d.max_dist; a.n_pairs = d.n_pairs;
    a.counts = d.counts.p;
    return a;
}
// a row per placed record (link_scan_kernel), on the engine stream behind the scan of the same records
int Linkage::push(bk_engine* e, const Records& r) {
    if (!in_sample || r.n == 0) return BK_OK;      // (enabled after this sample began: it has no rows)
    if (r.n >= (1ull << 31)) return fail(BK_ERR_UNSUPPORTED, "bk_link_enable: a batch of 2^31 records or more");
    const uint64_t need = rows_upper + r.n;       // (only the device knows how many of the records are placed: room for all of them)
    if (need >= (1ull << 32)) return fail(BK_ERR_UNSUPPORTED, "bk_link_enable: a sample of 2^32 records or more (%llu)", (unsigned long long)need);
    const uint64_t cap = rows.n / 2;
    if (int rc = link_free_old(*this, false)) return rc;
    if (need > cap) {   // a larger store: allocate, copy behind the scans so far; the old one stays until the stream has passed the copy
        const uint64_t ncap = std::min<uint64_t>(std::max<uint64_t>(need, 2 * cap), 1ull << 32);
        uint4* np = nullptr;
        const hipError_t err = hipMalloc(reinterpret_cast<void**>(&np), (size_t)ncap * 2 * sizeof(uint4));
        if (err != hipSuccess) return fail(BK_ERR_HIP, "bk_link_enable: no memory for a row store of %llu rows: %s", (unsigned long long)ncap, hipGetErrorString(err));
        const uint64_t filled = std::min<uint64_t>(rows_upper, cap);
        if (filled) {
            const hipError_t ce = hipMemcpyAsync(np, rows.p, (size_t)filled * 2 * sizeof(uint4), hipMemcpyDeviceToDevice, e->stream);
            if (ce != hipSuccess) { (void)hipFree(np); return fail(BK_ERR_HIP, "bk_link_enable: copying the row store failed: %s", hipGetErrorString(ce)); }
        }
        Event passed;                                // behind the copy: the old store is free once the stream is here
        hipError_t ee = passed.create();
        if (ee == hipSuccess) ee = hipEventRecord(passed, e->stream);
        if (ee != hipSuccess) { (void)hipStreamSynchronize(e->stream); (void)hipFree(np); return fail(BK_ERR_HIP, "bk_link_enable: hipEventRecord failed: %s", hipGetErrorString(ee)); }
        old.emplace_back(rows.p, std::move(passed));
        rows.p = np; rows.n = (size_t)ncap * 2;
    }
    rows_upper = need;
    bk::LinkArgs a = link_args(e); a.rec = records_view(r);
    bk::launch_link_scan(a, e->ix->n_cus, e->stream);
    return BK_OK;
}

int bk_link_enable(bk_engine* e, const bk_link_config* cfg) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_link_enable comes between samples");
    const IndexTables& ix = *e->ix;
    if (cfg) {
        if (cfg->max_mismatches > 8) return fail(BK_ERR_INVALID, "bk_link_enable: max_mismatches must be 0..8, got %u", cfg->max_mismatches);
        if (cfg->initial_rows < 1 || cfg->initial_rows > (1ull << 32))
            return fail(BK_ERR_INVALID, "bk_link_enable: initial_rows must be 1..2^32, got %llu", (unsigned long long)cfg->initial_rows);
        if (ix.n_files != 1)
            return fail(BK_ERR_INVALID, "bk_link_enable: the index has %d genome files; linkage is counted against an index of one genome file", ix.n_files);
        if (int rc = anchor_index_check(ix, "bk_link_enable")) return rc;
    }
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));   // (the last sample's kernels may still use the buffers being freed)
    e->linkage.reset();
    if (!cfg) return BK_OK;
    std::unique_ptr<Linkage> d(new Linkage());
    d->cfg = *cfg;
    if (int rc = anchor_tables(e, "bk_link_enable", d->anchors)) return rc;
    BK_HIP(d->rows.alloc((size_t)cfg->initial_rows * 2));
    BK_HIP(d->tallies.alloc(4));
    BK_HIP(hipMemsetAsync(d->tallies.p, 0, 4 * sizeof(unsigned long long), e->stream));
    e->linkage = std::move(d);
    return BK_OK;
}

int bk_sample_linkage(bk_engine* e, const uint32_t* cells, uint32_t n_sites, uint32_t max_dist) {
    if (int rc = store_count_ready(e, cells, n_sites, "bk_sample_linkage")) return rc;
    if (n_sites > BK_LINK_MAX_SITES) return fail(BK_ERR_INVALID, "bk_sample_linkage: at most %d sites, got %u", BK_LINK_MAX_SITES, n_sites);
    if (max_dist < 1 || max_dist > BK_LINK_MAX_DIST) return fail(BK_ERR_INVALID, "bk_sample_linkage: max_dist must be 1..%d, got %u", BK_LINK_MAX_DIST, max_dist);
    const IndexTables& ix = *e->ix;
    for (uint32_t i = 0; i < n_sites; i++) {
        if (cells[i] >= ix.total_cells) return fail(BK_ERR_INVALID, "bk_sample_linkage: site %u is cell %u, the index has %llu", i, cells[i], (unsigned long long)ix.total_cells);
        if (i && cells[i] <= cells[i - 1]) return fail(BK_ERR_INVALID, "bk_sample_linkage: the sites must be strictly ascending (site %u is cell %u behind cell %u)", i, cells[i], cells[i - 1]);
    }
    Linkage& d = *e->linkage;
    // the pairs: i < j in one sequence, cell_j - cell_i <= max_dist -- for each i a stretch of j that starts at i + 1
    std::vector<uint32_t> seq_end;               // end cell of every sequence of the genome file
    for (size_t q = 0; q < n_seqs(ix); q++) seq_end.push_back((uint32_t)seq_cells(ix, q).second);
    std::vector<uint32_t> pair_lo(n_sites);
    uint64_t n_pairs = 0;
    for (uint32_t i = 0, j = 0, s = 0; i < n_sites; i++) {
        while (s + 1 < seq_end.size() && cells[i] >= seq_end[s]) s++;
        if (j < i + 1) j = i + 1;
        while (j < n_sites && cells[j] < seq_end[s] && cells[j] - cells[i] <= max_dist) j++;   // (j never moves back: both bounds grow with i)
        pair_lo[i] = (uint32_t)std::min<uint64_t>(n_pairs, 0xffffffffull);
        n_pairs += j - (i + 1);
    }
    if (n_pairs > BK_LINK_MAX_PAIRS)
        return fail(BK_ERR_INVALID, "bk_sample_linkage: %llu pairs of sites within %u cells, at most %u are counted", (unsigned long long)n_pairs, max_dist, BK_LINK_MAX_PAIRS);
    BK_HIP(hipSetDevice(e->device));
    if (int rc = d.wait_last()) return rc;         // (the sites, pair_lo, the counters and the pinned copies are replaced here)
    d.n_sites = n_sites; d.max_dist = max_dist; d.n_pairs = n_pairs;
    bk_engine::Span sp(e, 1);
    if (int rc = upload(d.h_sites, d.sites, cells, n_sites, e->stream)) return rc;
    if (int rc = upload(d.h_pair_lo, d.pair_lo, pair_lo.data(), n_sites, e->stream)) return rc;
    BK_HIP(grow(d.counts, (size_t)n_pairs * 16));
    if (n_pairs) BK_HIP(hipMemsetAsync(d.counts.p, 0, (size_t)n_pairs * 16 * sizeof(unsigned int), e->stream));
    bk::launch_link_count(link_args(e), d.rows_upper, ix.n_cus, e->stream);
    return d.record(e->stream);
}

static int link_finalized(bk_engine* e, const char* who) {
    if (e->in_sample || !e->linkage || !e->linkage->in_sample || e->finalized_mates < 1)
        return fail(BK_ERR_STATE, "%s comes after bk_sample_finalize of a sample that began with linkage enabled", who);
    return BK_OK;
}

int bk_sample_download_linkage(bk_engine* e, bk_link_summary* summary, bk_link_pair* pairs, uint64_t cap) {
    if (!e || !summary) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = link_finalized(e, "bk_sample_download_linkage")) return rc;
    Linkage& d = *e->linkage;
    BK_HIP(hipSetDevice(e->device));
    unsigned long long t[4];
    if (int rc = download(e, t, d.tallies.p, 4)) return rc;
    summary->records = t[0]; summary->placed = t[1]; summary->unplaced = t[2]; summary->discordant = t[3];
    summary->n_pairs = d.made ? d.n_pairs : 0; summary->n_sites = d.made ? d.n_sites : 0; summary->max_dist = d.made ? d.max_dist : 0;
    const uint64_t n = std::min<uint64_t>(summary->n_pairs, cap);
    if (!n || !pairs) return BK_OK;
    std::vector<unsigned int> counts((size_t)n * 16);
    BK_HIP(hipMemcpy(counts.data(), d.counts.p, counts.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (uint32_t i = 0; i < d.n_sites && at < n; i++) {
        const uint64_t end = i + 1 < d.n_sites ? d.h_pair_lo.p[i + 1] : d.n_pairs;
        for (uint64_t p = d.h_pair_lo.p[i]; p < end && at < n; p++, at++) {
            pairs[at].site_a = d.h_sites.p[i]; pairs[at].site_b = d.h_sites.p[i + 1 + (size_t)(p - d.h_pair_lo.p[i])];
            std::memcpy(pairs[at].count, counts.data() + (size_t)p * 16, 16 * sizeof(uint32_t));
        }
    }
    return BK_OK;
}

int bk_sample_download_link_rows(bk_engine* e, bk_link_row* rows, uint64_t cap) {
    static_assert(sizeof(bk_link_row) == 2 * sizeof(uint4), "a row is two 16-byte stores");
    if (!e || (!rows && cap)) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = link_finalized(e, "bk_sample_download_link_rows")) return rc;
    Linkage& d = *e->linkage;
    BK_HIP(hipSetDevice(e->device));
    unsigned long long placed = 0;
    if (int rc = download(e, &placed, d.tallies.p + 1, 1)) return rc;
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(placed, cap), d.rows.n / 2);
    if (n) BK_HIP(hipMemcpy(rows, d.rows.p, (size_t)n * sizeof(bk_link_row), hipMemcpyDeviceToHost));
    return BK_OK;
}

// ---- the triplets the placed records carry at the codons of coding regions (bk_codons.hip) -----------------------------------------
static bk::CodonArgs codon_args(const bk_engine* e) {
    const Linkage& d = *e->linkage;
    const Codons& c = *d.codons;
    bk::CodonArgs a{};
    a.store = store_view(d);
    a.ref_words = e->ix->ref_words.p + bk::scan_ref_pad_words(); a.total_cells = (uint32_t)e->ix->total_cells;   // (anchor_index's)
    a.sorted = c.sorted.p; a.regions = c.regions.p; a.n_regions = c.n_regions; a.n_codons = c.n_codons;
    a.cover_diff = c.cover_diff.p; a.counts = c.counts.p;
    return a;
}

int bk_sample_codons(bk_engine* e, const bk_codon_region* regions, uint32_t n_regions) {
    if (int rc = store_count_ready(e, regions, n_regions, "bk_sample_codons")) return rc;
    if (n_regions > BK_CODON_MAX_REGIONS) return fail(BK_ERR_INVALID, "bk_sample_codons: at most %d regions, got %u", BK_CODON_MAX_REGIONS, n_regions);
    const IndexTables& ix = *e->ix;
    uint64_t n_codons = 0;
    for (uint32_t i = 0; i < n_regions; i++) {
        if (regions[i].n_codons == 0) return fail(BK_ERR_INVALID, "bk_sample_codons: region %u has no codon", i);
        if (int rc = region_cells_check(ix, "bk_sample_codons", i, regions[i].cell0, regions[i].cell0 + 3ull * regions[i].n_codons)) return rc;
        n_codons += regions[i].n_codons;
    }
    if (n_codons > BK_CODON_MAX_CODONS)
        return fail(BK_ERR_INVALID, "bk_sample_codons: %llu codons in %u regions, at most %u are counted", (unsigned long long)n_codons, n_regions, BK_CODON_MAX_CODONS);
    Linkage& d = *e->linkage;
    if (!d.codons) d.codons.reset(new Codons());
    Codons& c = *d.codons;
    BK_HIP(hipSetDevice(e->device));
    if (int rc = c.wait_last()) return rc;         // (the tables, the counters and the pinned copies are replaced here)
    // the caller's order with each region's first codon; the same sorted by first cell, with the running maximum of the ends
    std::vector<uint2> in_order(n_regions);
    std::vector<uint4> sorted(n_regions);
    uint32_t base = 0, reach = 0;
    for (uint32_t i = 0; i < n_regions; i++) { in_order[i] = make_uint2(regions[i].cell0, base); base += regions[i].n_codons; }
    const std::vector<uint32_t> order = by_first_cell(regions, n_regions);
    for (uint32_t i = 0; i < n_regions; i++) {
        const bk_codon_region& r = regions[order[i]];
        reach = std::max(reach, r.cell0 + 3u * r.n_codons);
        sorted[i] = make_uint4(r.cell0, r.n_codons, in_order[order[i]].y, reach);
    }
    c.n_regions = n_regions; c.n_codons = (uint32_t)n_codons;
    bk_engine::Span sp(e, 1);
    if (int rc = upload(c.h_sorted, c.sorted, sorted.data(), n_regions, e->stream)) return rc;
    if (int rc = upload(c.h_regions, c.regions, in_order.data(), n_regions, e->stream)) return rc;
    BK_HIP(grow(c.cover_diff, (size_t)n_codons + 1)); BK_HIP(grow(c.counts, (size_t)n_codons * 64));
    if (n_regions) {
        BK_HIP(hipMemsetAsync(c.cover_diff.p, 0, ((size_t)n_codons + 1) * sizeof(unsigned int), e->stream));
        BK_HIP(hipMemsetAsync(c.counts.p, 0, (size_t)n_codons * 64 * sizeof(unsigned int), e->stream));
    }
    const bk::CodonArgs a = codon_args(e);
    bk::launch_codon_count(a, d.rows_upper, ix.n_cus, e->stream);
    bk::launch_codon_finish(a, e->stream);
    return c.record(e->stream);
}

int bk_sample_download_codons(bk_engine* e, bk_codon_summary* summary, uint32_t* counts, uint64_t cap_codons) {
    if (!e || (!summary && !counts) || (!counts && cap_codons)) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = link_finalized(e, "bk_sample_download_codons")) return rc;
    Linkage& d = *e->linkage;
    const Codons* c = d.codons && d.codons->made ? d.codons.get() : nullptr;
    BK_HIP(hipSetDevice(e->device));
    unsigned long long placed = 0;
    if (int rc = download(e, &placed, d.tallies.p + 1, 1)) return rc;
    if (summary) { summary->rows = placed; summary->n_codons = c ? c->n_codons : 0; summary->n_regions = c ? c->n_regions : 0; }
    const uint64_t n = std::min<uint64_t>(c ? c->n_codons : 0, cap_codons);
    if (n) BK_HIP(hipMemcpy(counts, c->counts.p, (size_t)n * 64 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return BK_OK;
}

// ---- the lists of substitutions the placed records carry across whole regions (bk_haplotypes.hip) ----------------------------------
static bk::HapArgs hap_args(const bk_engine* e) {
    const Linkage& d = *e->linkage;
    const Haplotypes& h = *d.haps;
    bk::HapArgs a{};
    a.store = store_view(d);
    a.sorted = h.sorted.p; a.regions = h.regions.p; a.n_regions = h.n_regions; a.table_log2 = h.table_log2;
    a.hot = h.hot.p; a.owner = h.owner.p; a.count = h.count.p; a.tallies = h.tallies.p;
    a.entries = h.entries.p; a.entry_cap = std::min<uint64_t>(h.entries.n, 1ull << h.table_log2);
    return a;
}

int bk_sample_haplotypes(bk_engine* e, const bk_hap_region* regions, uint32_t n_regions, uint32_t table_log2) {
    static_assert(sizeof(bk_hap_entry) == 40 && sizeof(bk_hap_region) == sizeof(uint2), "hap_finish_kernel writes an entry as ten words");
    if (int rc = store_count_ready(e, regions, n_regions, "bk_sample_haplotypes")) return rc;
    if (n_regions > BK_HAP_MAX_REGIONS) return fail(BK_ERR_INVALID, "bk_sample_haplotypes: at most %d regions, got %u", BK_HAP_MAX_REGIONS, n_regions);
    if (table_log2 < 10 || table_log2 > 24) return fail(BK_ERR_INVALID, "bk_sample_haplotypes: table_log2 must be 10..24, got %u", table_log2);
    if (const char* v = test_env("BK_HAP_TABLE_SHRINK"))   // testing build: 2^-v of the slots asked for, not below 2^10 -- a small sample fills a table
        table_log2 -= std::min<uint32_t>(table_log2 - 10, (uint32_t)std::max(0, atoi(v)));
    const IndexTables& ix = *e->ix;
    for (uint32_t i = 0; i < n_regions; i++) {
        if (regions[i].len == 0) return fail(BK_ERR_INVALID, "bk_sample_haplotypes: region %u has no cell", i);
        if (regions[i].len > BK_HAP_MAX_LEN) return fail(BK_ERR_INVALID, "bk_sample_haplotypes: region %u has %u cells, at most %d", i, regions[i].len, BK_HAP_MAX_LEN);
        if (int rc = region_cells_check(ix, "bk_sample_haplotypes", i, regions[i].cell0, (uint64_t)regions[i].cell0 + regions[i].len)) return rc;
    }
    Linkage& d = *e->linkage;
    if (!d.haps) d.haps.reset(new Haplotypes());
    Haplotypes& h = *d.haps;
    BK_HIP(hipSetDevice(e->device));
    if (int rc = h.wait_last()) return rc;         // (the tables, the counters and the pinned copies are replaced here)
    // the caller's order (a bk_hap_region is the uint2 {cell0, len}); the same sorted by first cell, each with its index in the caller's order
    const std::vector<uint32_t> order = by_first_cell(regions, n_regions);
    std::vector<uint2> sorted(n_regions);
    for (uint32_t i = 0; i < n_regions; i++) sorted[i] = make_uint2(regions[order[i]].cell0, regions[order[i]].len | (order[i] << 16));
    const size_t slots = (size_t)1 << table_log2;
    h.n_regions = n_regions; h.table_log2 = table_log2;
    bk_engine::Span sp(e, 1);
    if (int rc = upload(h.h_sorted, h.sorted, sorted.data(), n_regions, e->stream)) return rc;
    if (int rc = upload(h.h_regions, h.regions, reinterpret_cast<const uint2*>(regions), n_regions, e->stream)) return rc;
    BK_HIP(grow(h.hot, (size_t)n_regions * 2));
    if (h.owner.n < slots) { BK_HIP(h.owner.alloc(slots)); BK_HIP(h.count.alloc(slots)); BK_HIP(h.entries.alloc(slots)); }
    if (!h.tallies.p) BK_HIP(h.tallies.alloc(2));
    BK_HIP(hipMemsetAsync(h.tallies.p, 0, 2 * sizeof(unsigned long long), e->stream));
    if (n_regions) {
        BK_HIP(hipMemsetAsync(h.hot.p, 0, (size_t)n_regions * 2 * sizeof(unsigned int), e->stream));
        BK_HIP(hipMemsetAsync(h.owner.p, 0, slots * sizeof(unsigned long long), e->stream));
        BK_HIP(hipMemsetAsync(h.count.p, 0, slots * sizeof(unsigned int), e->stream));
    }
    const bk::HapArgs a = hap_args(e);
    bk::launch_hap_count(a, d.rows_upper, ix.n_cus, e->stream);
    bk::launch_hap_finish(a, e->stream);
    return h.record(e->stream);
}

// by region, then by list as a sequence of (offset, base), a proper prefix first
static bool hap_entry_less(const bk_hap_entry& x, const bk_hap_entry& y) {
    if (x.region != y.region) return x.region < y.region;
    for (uint32_t i = 0; i < std::min<uint32_t>(x.n_mm, y.n_mm); i++) {
        if (bk::mm_offset(x.mm, i) != bk::mm_offset(y.mm, i)) return bk::mm_offset(x.mm, i) < bk::mm_offset(y.mm, i);
        if (bk::mm_base(x.mm, i) != bk::mm_base(y.mm, i)) return bk::mm_base(x.mm, i) < bk::mm_base(y.mm, i);
    }
    return x.n_mm < y.n_mm;
}

int bk_sample_download_haplotypes(bk_engine* e, bk_hap_summary* summary, uint32_t* cover, uint32_t* ref_count, bk_hap_entry* entries, uint64_t cap) {
    if (!e || !summary || (!entries && cap)) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = link_finalized(e, "bk_sample_download_haplotypes")) return rc;
    Linkage& d = *e->linkage;
    const Haplotypes* h = d.haps && d.haps->made ? d.haps.get() : nullptr;
    BK_HIP(hipSetDevice(e->device));
    unsigned long long placed = 0, t[2] = {0, 0};
    if (int rc = download(e, &placed, d.tallies.p + 1, 1)) return rc;
    if (h) { if (int rc = download(e, t, h->tallies.p, 2)) return rc; }
    summary->rows = placed; summary->entries = t[0]; summary->dropped = t[1];
    summary->n_regions = h ? h->n_regions : 0; summary->table_log2 = h ? h->table_log2 : 0;
    if (!h) return BK_OK;
    if (h->n_regions && (cover || ref_count)) {
        std::vector<unsigned int> hot((size_t)h->n_regions * 2);
        BK_HIP(hipMemcpy(hot.data(), h->hot.p, hot.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < h->n_regions; i++) {
            if (cover) cover[i] = hot[2 * (size_t)i];
            if (ref_count) ref_count[i] = hot[2 * (size_t)i + 1];
        }
    }
    if (t[1])
        return fail(BK_ERR_RANGE, "bk_sample_download_haplotypes: the table of 2^%u slots (table_log2 = %u) is full, %llu haplotype counts were dropped: call bk_sample_haplotypes again with a larger table_log2",
                    h->table_log2, h->table_log2, (unsigned long long)t[1]);
    const uint64_t have = std::min<uint64_t>(t[0], (uint64_t)1 << h->table_log2);
    if (!have || !cap) return BK_OK;
    std::vector<bk_hap_entry> all((size_t)have);
    BK_HIP(hipMemcpy(all.data(), h->entries.p, all.size() * sizeof(bk_hap_entry), hipMemcpyDeviceToHost));
    std::sort(all.begin(), all.end(), hap_entry_less);
    std::memcpy(entries, all.data(), (size_t)std::min<uint64_t>(cap, have) * sizeof(bk_hap_entry));
    return BK_OK;
}

// ---- the bases the placed records carry at every cell, by strand and near their ends (bk_read_pileup.hip) --------------------------
static bk::ReadPileupArgs read_pileup_args(const bk_engine* e) {
    const Linkage& d = *e->linkage;
    const ReadPileup& p = *d.read_pileup;
    const size_t n = (size_t)e->ix->total_cells;
    bk::ReadPileupArgs a{};
    a.store = store_view(d);
    a.ref_words = e->ix->ref_words.p + bk::scan_ref_pad_words(); a.total_cells = (uint32_t)n;   // (anchor_index's)
    a.end_dist = p.end_dist;
    a.mm = p.work.p; a.mm_near = p.work.p + 8 * n; a.diff = p.work.p + 12 * n;   // (the two that are read 16 bytes at a time come first)
    a.cells = p.cells.p; a.tallies = p.tallies.p;
    return a;
}

int bk_sample_read_pileup(bk_engine* e, uint32_t end_dist) {
    static_assert(sizeof(bk_read_pileup_cell) == 3 * sizeof(uint4), "read_pileup_finish_kernel writes a cell as three 16-byte stores");
    if (int rc = store_count_ready(e, nullptr, 0, "bk_sample_read_pileup")) return rc;
    if (end_dist > BK_READ_PILEUP_MAX_END) return fail(BK_ERR_INVALID, "bk_sample_read_pileup: end_dist must be 0..%d, got %u", BK_READ_PILEUP_MAX_END, end_dist);
    const IndexTables& ix = *e->ix;
    if (ix.total_cells > BK_READ_PILEUP_MAX_CELLS)
        return fail(BK_ERR_UNSUPPORTED, "bk_sample_read_pileup: the index has %llu cells, the read pileup is made for at most %u", (unsigned long long)ix.total_cells,
                    BK_READ_PILEUP_MAX_CELLS);
    Linkage& d = *e->linkage;
    if (!d.read_pileup) d.read_pileup.reset(new ReadPileup());
    ReadPileup& p = *d.read_pileup;
    BK_HIP(hipSetDevice(e->device));
    if (int rc = p.wait_last()) return rc;         // (the work arrays and the cells are replaced here)
    const size_t n = (size_t)ix.total_cells, words = 15 * n + 3;
    if (p.work.n < words) { BK_HIP(p.work.alloc(words)); BK_HIP(p.cells.alloc(std::max<size_t>(n, 1))); BK_HIP(p.tallies.alloc(2)); }
    p.end_dist = end_dist;
    bk_engine::Span sp(e, 1);
    BK_HIP(hipMemsetAsync(p.work.p, 0, words * sizeof(unsigned int), e->stream));
    BK_HIP(hipMemsetAsync(p.tallies.p, 0, 2 * sizeof(unsigned long long), e->stream));
    const bk::ReadPileupArgs a = read_pileup_args(e);
    bk::launch_read_pileup_count(a, d.rows_upper, ix.n_cus, e->stream);
    bk::launch_read_pileup_finish(a, e->stream);
    return p.record(e->stream);
}

int bk_sample_download_read_pileup(bk_engine* e, bk_read_pileup_summary* summary, bk_read_pileup_cell* cells, uint64_t cap_cells) {
    if (!e || !summary || (!cells && cap_cells)) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = link_finalized(e, "bk_sample_download_read_pileup")) return rc;
    Linkage& d = *e->linkage;
    if (!d.read_pileup || !d.read_pileup->made) return fail(BK_ERR_STATE, "bk_sample_download_read_pileup comes after this sample's bk_sample_read_pileup");
    const ReadPileup& p = *d.read_pileup;
    BK_HIP(hipSetDevice(e->device));
    unsigned long long placed = 0, t[2] = {0, 0};
    if (int rc = download(e, &placed, d.tallies.p + 1, 1)) return rc;
    if (int rc = download(e, t, p.tallies.p, 2)) return rc;
    summary->rows = placed; summary->n_cells = e->ix->total_cells; summary->end_dist = p.end_dist; summary->pad = 0;
    summary->covered = t[0]; summary->bases = t[1];
    const uint64_t n = std::min<uint64_t>(e->ix->total_cells, cap_cells);
    if (n) BK_HIP(hipMemcpy(cells, p.cells.p, (size_t)n * sizeof(bk_read_pileup_cell), hipMemcpyDeviceToHost));
    return BK_OK;
}
