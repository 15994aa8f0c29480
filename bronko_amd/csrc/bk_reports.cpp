// bk_reports.cpp -- the reports made of a finalized sample's pileup on the device, and their downloads: the calls and the noise
// (bk_sample_call, bk_caller.hip), the consensus (consensus_kernel, bk_caller.hip) with the sample's indels applied to it (bk_consensus_indels.hip) and the per-region depths (bk_regions.hip).  Their
// buffers and the flags that say whose sample a result is (called, cons_made, minor_made, ci_made, regions_made) are bk_engine's (bk_engine.h).  The entry
// points are extern "C" by their declarations in bronko_hip.h.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "bk_engine.h"

// ---- after the pileup, on the device (bk_caller.hip) -----------------------------------------------------------
void bk_call_params_default(bk_call_params* p) {
    if (!p) return;
    p->k = 21;                          // consts.rs:3
    p->no_end_filter = 0; p->no_strand_filter = 0; p->no_strand_balance_filter = 0;
    p->min_af = 0.03;                   // consts.rs:8
    p->strand_balance_ratio = 0.1;      // consts.rs:10
    p->strand_odds_max = 6.0;           // cli.rs --strand_odds
    p->variant_multiplier = 1.5;        // consts.rs:15
    p->n_per_strand = 2; p->min_depth = 300; p->min_variant_depth = 3;
}

int bk_sample_call(bk_engine* e, int n_mates, const bk_call_params* p) {
    if (!e || !p) return fail(BK_ERR_INVALID, "null argument");
    const IndexTables& ix = *e->ix;
    if (n_mates < 1 || n_mates > 2) return fail(BK_ERR_INVALID, "n_mates must be 1 or 2");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_sample_call comes after bk_sample_finalize");
    if (e->finalized_mates == 0) return fail(BK_ERR_STATE, "bk_sample_call: no sample has been finalized on this engine");
    if (e->finalized_mates != n_mates) return fail(BK_ERR_STATE, "bk_sample_call(n_mates = %d): the sample was finalized with %d mate file(s)", n_mates, e->finalized_mates);
    BK_HIP(hipSetDevice(e->device));
    const uint64_t cap = std::max<uint64_t>(3 * ix.max_file_cells, 1);   // at most three alternative bases per position
    if (!e->call_out.p) {
        BK_HIP(e->call_noise.alloc((size_t)ix.total_cells));
        const size_t mc = std::max<uint64_t>(ix.max_file_cells, 1);
        BK_HIP(e->noise_maf.alloc(mc * 3));
        BK_HIP(e->noise_tbl.alloc((mc + 64 * (size_t)std::max(ix.max_seqs_per_file, 1) + 64) * 10));
        BK_HIP(e->noise_state.alloc(mc));
        BK_HIP(e->noise_sums.alloc(mc * 2));
        BK_HIP(e->noise_cnt.alloc(mc));
        BK_HIP(e->call_records.alloc((size_t)cap));
        BK_HIP(e->call_out.alloc(1));
    }
    bk::CallArgs a{};
    a.prm = *p;
    a.n_files = ix.n_files; a.n_mates = n_mates;
    a.stats = e->stats.p; a.present = e->present.p;
    a.genome_len = ix.genome_len.p; a.seq_first = ix.seq_first.p; a.n_seqs = ix.n_seqs_d.p; a.seq_cell = ix.seq_cell.p; a.seq_len = ix.seq_len_d.p;
    a.ref_words = ix.ref_words.p + bk::scan_ref_pad_words();
    a.pileup = e->pileup.p; a.plane = (size_t)ix.total_cells * 4;
    a.noise = e->call_noise.p; a.records = e->call_records.p; a.record_cap = cap; a.out = e->call_out.p;
    a.noise_maf = e->noise_maf.p; a.noise_tbl = e->noise_tbl.p; a.noise_sums = e->noise_sums.p; a.noise_cnt = e->noise_cnt.p; a.noise_state = e->noise_state.p;
    if (const char* ns = test_env("BK_NOISE_SERIAL")) a.noise_serial = atoi(ns);
    bk_engine::Span sp(e, 1);
    bk::launch_call(a, ix.max_seqs_per_file, ix.max_file_cells, e->stream);
    BK_HIP(hipGetLastError());
    e->called = true; e->cons_made = false; e->minor_made = false; e->ci_made = false; e->regions_made = false;   // (a consensus or a region report made before this call was of another selection)
    return BK_OK;
}

int bk_sample_download_calls(bk_engine* e, bk_call_summary* summary, bk_call_record* records, uint64_t cap) {
    if (!e || !summary) return fail(BK_ERR_INVALID, "null argument");
    if (!e->call_out.p) return fail(BK_ERR_STATE, "bk_sample_download_calls comes after bk_sample_call");
    BK_HIP(hipSetDevice(e->device));
    if (int rc = download(e, summary, e->call_out.p, 1)) return rc;
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(summary->n_records, cap), e->call_records.n);
    if (n && records) {
        BK_HIP(hipMemcpy(records, e->call_records.p, (size_t)n * sizeof(bk_call_record), hipMemcpyDeviceToHost));
        std::sort(records, records + n, [](const bk_call_record& x, const bk_call_record& y) {
            if (x.seq_id != y.seq_id) return x.seq_id < y.seq_id;
            if (x.pos != y.pos) return x.pos < y.pos;
            return x.alt_base < y.alt_base;
        });
    }
    return BK_OK;
}

int bk_sample_download_noise(bk_engine* e, double* out, uint64_t cap, uint64_t* n) {
    if (!e || !n) return fail(BK_ERR_INVALID, "null argument");
    if (!e->call_out.p) return fail(BK_ERR_STATE, "bk_sample_download_noise comes after bk_sample_call");
    BK_HIP(hipSetDevice(e->device));
    bk_call_summary summ;
    if (int rc = download(e, &summ, e->call_out.p, 1)) return rc;
    *n = 0;
    if (summ.file_id < 0 || summ.file_id >= e->ix->n_files) return BK_OK;
    const uint64_t lo = e->ix->file_cell_lo[(size_t)summ.file_id], hi = summ.file_id + 1 < e->ix->n_files ? e->ix->file_cell_lo[(size_t)summ.file_id + 1] : e->ix->total_cells;
    *n = hi - lo;
    if (out && cap) BK_HIP(hipMemcpy(out, e->call_noise.p + lo, (size_t)std::min<uint64_t>(cap, hi - lo) * sizeof(double), hipMemcpyDeviceToHost));
    return BK_OK;
}

// ---- per-sample consensus (consensus_kernel, bk_caller.hip) ------------------------------------------------------
void bk_consensus_params_default(bk_consensus_params* p) {
    if (!p) return;
    p->min_depth = 10; p->min_freq = 0.5;
}

int bk_sample_consensus(bk_engine* e, const bk_consensus_params* p) {
    if (!e || !p) return fail(BK_ERR_INVALID, "null argument");
    if (p->min_depth < 1) return fail(BK_ERR_INVALID, "bk_sample_consensus: min_depth must be at least 1, got %llu", (unsigned long long)p->min_depth);
    if (!(p->min_freq >= 0.0 && p->min_freq <= 1.0)) return fail(BK_ERR_INVALID, "bk_sample_consensus: min_freq must be between 0 and 1, got %g", p->min_freq);
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_sample_consensus comes after bk_sample_finalize and bk_sample_call");
    if (!e->called) return fail(BK_ERR_STATE, "bk_sample_consensus: bk_sample_call has not run for this sample");
    const IndexTables& ix = *e->ix;
    BK_HIP(hipSetDevice(e->device));
    if (!e->cons_out.p) {
        BK_HIP(e->cons_letters.alloc((size_t)ix.max_file_cells));
        BK_HIP(e->cons_out.alloc(1));
    }
    bk::ConsensusArgs a{};
    a.prm = *p;
    a.seq_first = ix.seq_first.p; a.n_seqs = ix.n_seqs_d.p; a.seq_cell = ix.seq_cell.p; a.seq_len = ix.seq_len_d.p;
    a.ref_words = ix.ref_words.p + bk::scan_ref_pad_words();
    a.pileup = e->pileup.p; a.plane = (size_t)ix.total_cells * 4;
    a.out = e->call_out.p; a.letters = e->cons_letters.p; a.summary = e->cons_out.p;
    bk_engine::Span sp(e, 1);
    BK_HIP(hipMemsetAsync(e->cons_out.p, 0, sizeof(bk_consensus_summary), e->stream));
    bk::launch_consensus(a, ix.max_file_cells, e->stream);
    BK_HIP(hipGetLastError());
    e->cons_made = true; e->cons_prm = *p;
    e->ci_made = false;                     // (fresh letters: the indels are not in them)
    return BK_OK;
}

int bk_sample_download_consensus(bk_engine* e, bk_consensus_summary* summary, uint8_t* letters, uint64_t cap) {
    if (!e || !summary) return fail(BK_ERR_INVALID, "null argument");
    if (!e->cons_made) return fail(BK_ERR_STATE, "bk_sample_download_consensus comes after this sample's bk_sample_consensus");
    BK_HIP(hipSetDevice(e->device));
    if (int rc = download(e, summary, e->cons_out.p, 1)) return rc;
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(summary->positions, cap), e->cons_letters.n);
    if (n && letters) return download(e, letters, e->cons_letters.p, (size_t)n);
    return BK_OK;
}

// ---- per-sample minor alleles (minor_alleles_kernel, bk_caller.hip) -----------------------------------------------
void bk_minor_params_default(bk_minor_params* p) {
    if (!p) return;
    p->min_reads = 10; p->min_freq = 0.03;
}

int bk_sample_minor_alleles(bk_engine* e, const bk_minor_params* p) {
    if (!e) return fail(BK_ERR_INVALID, "bk_sample_minor_alleles: e is null");
    if (!p) return fail(BK_ERR_INVALID, "bk_sample_minor_alleles: p is null");
    if (p->min_reads < 1) return fail(BK_ERR_INVALID, "bk_sample_minor_alleles: min_reads must be at least 1, got %llu", (unsigned long long)p->min_reads);
    if (!(p->min_freq >= 0.0 && p->min_freq <= 1.0)) return fail(BK_ERR_INVALID, "bk_sample_minor_alleles: min_freq must be between 0 and 1, got %g", p->min_freq);
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_sample_minor_alleles comes after bk_sample_finalize and bk_sample_call");
    if (!e->called) return fail(BK_ERR_STATE, "bk_sample_minor_alleles: bk_sample_call has not run for this sample");
    const IndexTables& ix = *e->ix;
    BK_HIP(hipSetDevice(e->device));
    if (!e->minor_out.p) {
        BK_HIP(e->minor_masks.alloc((size_t)ix.max_file_cells));
        BK_HIP(e->minor_out.alloc(1));
    }
    bk::MinorArgs a{};
    a.prm = *p;
    a.seq_first = ix.seq_first.p; a.n_seqs = ix.n_seqs_d.p; a.seq_cell = ix.seq_cell.p; a.seq_len = ix.seq_len_d.p;
    a.pileup = e->pileup.p; a.plane = (size_t)ix.total_cells * 4;
    a.out = e->call_out.p; a.masks = e->minor_masks.p; a.summary = e->minor_out.p;
    bk_engine::Span sp(e, 1);
    BK_HIP(hipMemsetAsync(e->minor_out.p, 0, sizeof(bk_minor_summary), e->stream));
    bk::launch_minor_alleles(a, ix.max_file_cells, e->stream);
    BK_HIP(hipGetLastError());
    e->minor_made = true;
    return BK_OK;
}

int bk_sample_download_minor_alleles(bk_engine* e, bk_minor_summary* summary, uint8_t* masks, uint64_t cap) {
    if (!e) return fail(BK_ERR_INVALID, "bk_sample_download_minor_alleles: e is null");
    if (!summary) return fail(BK_ERR_INVALID, "bk_sample_download_minor_alleles: summary is null");
    if (!e->minor_made) return fail(BK_ERR_STATE, "bk_sample_download_minor_alleles comes after this sample's bk_sample_minor_alleles");
    BK_HIP(hipSetDevice(e->device));
    if (int rc = download(e, summary, e->minor_out.p, 1)) return rc;
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(summary->positions, cap), e->minor_masks.n);
    if (n && masks) return download(e, masks, e->minor_masks.p, (size_t)n);
    return BK_OK;
}

// ---- the sample's indels applied to its consensus (bk_consensus_indels.hip) --------------------------------------------
int bk_sample_consensus_indels(bk_engine* e) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_sample_consensus_indels comes after bk_sample_finalize, bk_sample_consensus and bk_sample_indels");
    if (!e->indels || !e->indels->in_sample)
        return fail(BK_ERR_STATE, "bk_sample_consensus_indels: indels were not enabled for this sample (bk_indels_enable before bk_sample_begin)");
    if (!e->cons_made) return fail(BK_ERR_STATE, "bk_sample_consensus_indels: bk_sample_consensus has not run for this sample");
    if (!e->indels->made) return fail(BK_ERR_STATE, "bk_sample_consensus_indels: bk_sample_indels has not run for this sample");
    const IndexTables& ix = *e->ix;
    const Indels& d = *e->indels;
    BK_HIP(hipSetDevice(e->device));
    const size_t bounds = (size_t)ix.total_cells + 1;
    if (!e->ci_out.p) {
        BK_HIP(e->ci_bounds.alloc(2 * bounds));
        BK_HIP(e->ci_rows.alloc(BK_CONSENSUS_INDEL_MAX));
        BK_HIP(e->ci_out.alloc(1));
    }
    bk::ConsensusIndelArgs a{};
    a.prm = e->cons_prm;
    a.key0 = d.key0.p; a.key1 = d.key1.p; a.counts = d.counts.p; a.log2n = d.table_log2;
    a.total_cells = (uint32_t)ix.total_cells;   // (below 2^27: bk_indels_enable)
    a.span = d.span.p; a.table_overflow = d.tallies.p + bk::IndelArgs::kOverflow;
    a.out = e->call_out.p; a.seq_first = ix.seq_first.p; a.seq_cell = ix.seq_cell.p;
    a.best = e->ci_bounds.p; a.ties = e->ci_bounds.p + bounds;
    a.letters = e->cons_letters.p; a.n_letters = e->cons_letters.n;
    a.rows = e->ci_rows.p; a.summary = e->ci_out.p;
    bk_engine::Span sp(e, 1);
    BK_HIP(hipMemsetAsync(e->ci_bounds.p, 0, 2 * bounds * sizeof(unsigned int), e->stream));
    BK_HIP(hipMemsetAsync(e->ci_out.p, 0, sizeof(bk_consensus_indel_summary), e->stream));
    bk::launch_consensus_indels(a, e->stream);
    BK_HIP(hipGetLastError());
    e->ci_made = true;
    return BK_OK;
}

int bk_sample_download_consensus_indels(bk_engine* e, bk_consensus_indel_summary* s, bk_consensus_indel_record* rows, uint64_t cap) {
    if (!e || !s) return fail(BK_ERR_INVALID, "null argument");
    if (!e->ci_made) return fail(BK_ERR_STATE, "bk_sample_download_consensus_indels comes after this sample's bk_sample_consensus_indels");
    BK_HIP(hipSetDevice(e->device));
    if (int rc = download(e, s, e->ci_out.p, 1)) return rc;
    if (s->overflow)
        return fail(BK_ERR_INVALID, "bk_sample_download_consensus_indels: more than %d accepted events, or a full indel event table (bk_sample_download_indels tells)",
                    BK_CONSENSUS_INDEL_MAX);
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(s->accepted, cap), e->ci_rows.n);
    if (n && rows) return download(e, rows, e->ci_rows.p, (size_t)n);
    return BK_OK;
}

// ---- per-region depth report (region_depth_kernel, bk_regions.hip) ------------------------------------------------
int bk_regions_set(bk_engine* e, const bk_region* regions, uint64_t n) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_regions_set comes between samples");
    if (n > BK_MAX_REGIONS) return fail(BK_ERR_INVALID, "%llu regions: at most %u", (unsigned long long)n, (unsigned)BK_MAX_REGIONS);
    if (n && !regions) return fail(BK_ERR_INVALID, "null argument");
    const IndexTables& ix = *e->ix;
    std::vector<uint32_t> off((size_t)ix.n_files + 1, 0u);
    for (uint64_t i = 0; i < n; i++) {
        const bk_region& r = regions[i];
        if (r.file_id < 0 || r.file_id >= ix.n_files) return fail(BK_ERR_INVALID, "region %llu: no genome file %d (the index has %d)", (unsigned long long)i, r.file_id, ix.n_files);
        if ((int64_t)r.seq >= (int64_t)ix.h_n_seqs[(size_t)r.file_id])
            return fail(BK_ERR_INVALID, "region %llu: no sequence %u in genome file %d (it has %d)", (unsigned long long)i, r.seq, r.file_id, ix.h_n_seqs[(size_t)r.file_id]);
        const uint64_t len = ix.h_seq_len[(size_t)ix.h_seq_first[(size_t)r.file_id] + r.seq];
        if (!(r.start < r.end && (uint64_t)r.end <= len))
            return fail(BK_ERR_INVALID, "region %llu: [%u, %u) is not a range inside sequence %u of genome file %d (length %llu)", (unsigned long long)i, r.start, r.end,
                        r.seq, r.file_id, (unsigned long long)len);
        off[(size_t)r.file_id + 1] += 1;
    }
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));   // (the last sample's kernel may still use the table and the buffers being freed)
    e->regions.reset();
    e->regions_made = false;
    if (n == 0) return BK_OK;
    std::unique_ptr<Regions> rg(new Regions());
    for (int f = 0; f < ix.n_files; f++) { rg->max_file_regions = std::max(rg->max_file_regions, off[(size_t)f + 1]); off[(size_t)f + 1] += off[(size_t)f]; }
    std::vector<uint2> tab((size_t)n);
    std::vector<uint32_t> at(off.begin(), off.end() - 1);   // grouped by file, the caller's order within a file
    for (uint64_t i = 0; i < n; i++) {
        const bk_region& r = regions[i];
        const uint64_t cell = ix.h_seq_cell[(size_t)ix.h_seq_first[(size_t)r.file_id] + r.seq] + r.start;   // (below 2^32: build_index_tables)
        tab[at[(size_t)r.file_id]++] = make_uint2((uint32_t)cell, r.end - r.start);
    }
    BK_HIP(rg->table.upload(tab)); BK_HIP(rg->file_off.upload(off));
    BK_HIP(rg->rows.alloc(rg->max_file_regions)); BK_HIP(rg->out.alloc(1));
    e->regions = std::move(rg);
    return BK_OK;
}

int bk_sample_region_depths(bk_engine* e, uint64_t min_depth) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (min_depth < 1) return fail(BK_ERR_INVALID, "bk_sample_region_depths: min_depth must be at least 1, got 0");
    if (e->in_sample) return fail(BK_ERR_STATE, "bk_sample_region_depths comes after bk_sample_finalize and bk_sample_call");
    if (!e->called) return fail(BK_ERR_STATE, "bk_sample_region_depths: bk_sample_call has not run for this sample");
    if (!e->regions) return fail(BK_ERR_STATE, "bk_sample_region_depths: no regions are set (bk_regions_set)");
    const IndexTables& ix = *e->ix;
    Regions& rg = *e->regions;
    BK_HIP(hipSetDevice(e->device));
    bk::RegionArgs a{};
    a.min_depth = min_depth;
    a.table = rg.table.p; a.file_off = rg.file_off.p;
    a.pileup = e->pileup.p; a.plane = (size_t)ix.total_cells * 4;
    a.out = e->call_out.p; a.rows = rg.rows.p; a.summary = rg.out.p;
    bk_engine::Span sp(e, 1);
    BK_HIP(hipMemsetAsync(rg.out.p, 0, sizeof(bk_region_summary), e->stream));
    bk::launch_region_depths(a, rg.max_file_regions, e->stream);
    BK_HIP(hipGetLastError());
    e->regions_made = true;
    return BK_OK;
}

int bk_sample_download_region_depths(bk_engine* e, bk_region_summary* summary, bk_region_depth* out, uint64_t cap) {
    if (!e || !summary) return fail(BK_ERR_INVALID, "null argument");
    if (!e->regions_made || !e->regions) return fail(BK_ERR_STATE, "bk_sample_download_region_depths comes after this sample's bk_sample_region_depths");
    BK_HIP(hipSetDevice(e->device));
    if (int rc = download(e, summary, e->regions->out.p, 1)) return rc;
    const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(summary->n_regions, cap), e->regions->rows.n);
    if (n && out) return download(e, out, e->regions->rows.p, (size_t)n);
    return BK_OK;
}
