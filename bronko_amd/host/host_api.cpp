// host_api.cpp -- flat C entry points over the C++ host code (index build / .bkdb codec) so that the Python
// test + bench harness can drive the same code the `bronko` binary runs.  Not the drop-in boundary (that is
// include/bronko_hip.h); errors are returned as NULL / non-zero with bh_last_error().
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "breakends.hpp"
#include "caller.hpp"
#include "chimeras.hpp"
#include "codons.hpp"
#include "cohort.hpp"
#include "copybacks.hpp"
#include "duplications.hpp"
#include "haplotypes.hpp"
#include "consensus_indels.hpp"
#include "indels.hpp"
#include "junctions.hpp"
#include "linkage.hpp"
#include "index.hpp"
#include "read_pileup.hpp"

namespace {
thread_local std::string g_err;

// reads joined by '\n'
std::vector<std::string> split_lines(const char* reads) {
    std::vector<std::string> rd;
    for (const char* at = reads; at && *at;) {
        const char* nl = strchr(at, '\n');
        rd.emplace_back(nl ? std::string(at, nl) : std::string(at));
        at = nl ? nl + 1 : nullptr;
    }
    return rd;
}
// tables of named things (--codons' genes, --haplotypes' windows) cross this boundary as n rows of W u32 and their names joined by '\n'
// in: get(item, row) reads a row; a missing name is "."
template <int W, class T, class F>
std::vector<T> named_rows_in(const uint32_t* rows, const char* names, uint64_t n, F get) {
    std::vector<T> out((size_t)n);
    const char* at = names;
    for (uint64_t i = 0; i < n; i++) {
        get(out[i], rows + i * W);
        out[i].name = ".";
        if (at) {
            const char* nl = strchr(at, '\n');
            out[i].name = nl ? std::string(at, nl) : std::string(at);
            at = nl ? nl + 1 : nullptr;
        }
    }
    return out;
}
// out: put(item, row) writes a row; *n items, *names_len bytes of joined names, both written only where they fit cap / names_cap
template <int W, class T, class F>
int named_rows_out(const std::vector<T>& r, F put, uint64_t cap, uint32_t* rows, char* names, uint64_t names_cap, uint64_t* n, uint64_t* names_len) {
    std::string joined;
    for (size_t i = 0; i < r.size(); i++) joined += (i ? "\n" : "") + r[i].name;
    *n = r.size();
    if (names_len) *names_len = joined.size() + 1;
    if (rows && r.size() <= cap)
        for (size_t i = 0; i < r.size(); i++) put(r[i], rows + i * W);
    if (names && joined.size() + 1 <= names_cap) std::memcpy(names, joined.c_str(), joined.size() + 1);
    return 0;
}
// what every bh_*_events hands back: *n rows of which at most cap are written, the span of all cells, the counters in the order given
template <class Result, size_t N>
int events_out(const Result& r, const uint64_t (&c)[N], uint64_t cap, void* rows, uint64_t* n, uint32_t* span, uint64_t* counters) {
    *n = r.events.size();
    if (rows) std::memcpy(rows, r.events.data(), (size_t)std::min<uint64_t>(cap, r.events.size()) * sizeof r.events[0]);
    if (span) std::memcpy(span, r.span.data(), r.span.size() * sizeof(uint32_t));
    if (counters) std::memcpy(counters, c, sizeof c);
    return 0;
}
}  // namespace

extern "C" {

const char* bh_last_error(void) { return g_err.c_str(); }

void* bh_index_build(int k, const char* const* paths, int n, int threads) {
    try {
        std::vector<std::string> g(paths, paths + n);
        return new bronko::Index(bronko::build_indexes(k, g, threads));
    } catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

// files given in memory: one sequence list per file (names/seqs flattened in (file, seq) order)
void* bh_index_build_mem(int k, int n_files, const char* const* file_names, const int* n_seqs, const char* const* seq_names,
                         const uint8_t* const* seqs, const uint64_t* seq_lens, int threads) {
    try {
        std::vector<bronko::FileMeta> files(n_files);
        size_t q = 0;
        for (int f = 0; f < n_files; f++) {
            files[f].name = file_names[f];
            for (int s = 0; s < n_seqs[f]; s++, q++) {
                bronko::SeqMeta sm;
                sm.name = seq_names[q];
                sm.len = seq_lens[q];
                sm.seq.assign(seqs[q], seqs[q] + seq_lens[q]);
                files[f].sequences.push_back(std::move(sm));
            }
        }
        return new bronko::Index(bronko::build_indexes_mem(k, std::move(files), threads));
    } catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

void* bh_index_load(const char* path) {
    try { return new bronko::Index(bronko::load_index(path)); }
    catch (const std::exception& e) { g_err = e.what(); return nullptr; }
}

int bh_index_save(const void* h, const char* path) {
    try { bronko::save_index(*static_cast<const bronko::Index*>(h), path); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}

void bh_index_free(void* h) { delete static_cast<bronko::Index*>(h); }

#define IX static_cast<const bronko::Index*>(h)
int bh_index_k(const void* h) { return IX->k; }
int bh_index_meta_k(const void* h) { return IX->meta_k; }
uint64_t bh_index_n_buckets(const void* h) { return IX->ids.size(); }
uint64_t bh_index_n_entries(const void* h) { return IX->entries.size(); }
const uint64_t* bh_index_bucket_ids(const void* h) { return IX->ids.data(); }
const uint64_t* bh_index_bucket_off(const void* h) { return IX->off.data(); }
const void* bh_index_entries(const void* h) { return IX->entries.data(); }
int bh_index_n_files(const void* h) { return (int)IX->files.size(); }
const char* bh_index_file_name(const void* h, int f) { return IX->files[f].name.c_str(); }
int bh_index_n_seqs(const void* h, int f) { return (int)IX->files[f].sequences.size(); }
const char* bh_index_seq_name(const void* h, int f, int s) { return IX->files[f].sequences[s].name.c_str(); }
uint64_t bh_index_seq_len(const void* h, int f, int s) { return IX->files[f].sequences[s].len; }
const uint8_t* bh_index_seq(const void* h, int f, int s) { return IX->files[f].sequences[s].seq.data(); }
uint64_t bh_index_total_cells(const void* h) { return IX->total_cells(); }
#undef IX

// ---- caller stages (so that tests can drive the same code the `bronko` binary runs) ---------------------------
struct bh_call_params {   // mirrors bronko::CallParams
    int32_t k; double min_af; int32_t no_end_filter, no_strand_filter, no_strand_balance_filter; double strand_balance_ratio;
    uint64_t n_per_strand; double strand_odds_max; uint64_t min_depth, min_variant_depth; double variant_multiplier;
};

int bh_pick_best_genome(const void* h, const uint64_t* stats, const uint8_t* present) {
    const auto* ix = static_cast<const bronko::Index*>(h);
    const size_t nf = ix->files.size();
    return bronko::pick_best_genome(*ix, std::vector<uint64_t>(stats, stats + nf * 3), std::vector<uint8_t>(present, present + nf));
}

void bh_baseline_noise_max(const uint64_t* fwd4, const uint64_t* rev4, uint64_t len, double* out) {
    const std::vector<double> v = bronko::baseline_noise_max(fwd4, rev4, len);
    std::memcpy(out, v.data(), v.size() * sizeof(double));
}

// call_variants on the given arrays + writers.  summary = {n_records, n_major, n_minor}; cov = {breadth, depth}.
int bh_call_and_write(const void* h, int file_id, const uint64_t* fwd_depth, const uint64_t* rev_depth, const uint64_t* fwd_nk,
                      const uint64_t* rev_nk, const bh_call_params* cp, const char* vcf_path, const char* reads_path,
                      const char* pileup_path, uint64_t* summary, double* cov) {
    try {
        const auto* ix = static_cast<const bronko::Index*>(h);
        const size_t n = ix->total_cells() * 4;
        bronko::Pileup p;
        p.fwd_depth.assign(fwd_depth, fwd_depth + n); p.rev_depth.assign(rev_depth, rev_depth + n);
        p.fwd_nk.assign(fwd_nk, fwd_nk + n); p.rev_nk.assign(rev_nk, rev_nk + n);
        bronko::CallParams c;
        c.k = cp->k; c.min_af = cp->min_af; c.no_end_filter = cp->no_end_filter; c.no_strand_filter = cp->no_strand_filter;
        c.no_strand_balance_filter = cp->no_strand_balance_filter; c.strand_balance_ratio = cp->strand_balance_ratio;
        c.n_per_strand = cp->n_per_strand; c.strand_odds_max = cp->strand_odds_max; c.min_depth = cp->min_depth;
        c.min_variant_depth = cp->min_variant_depth; c.variant_multiplier = cp->variant_multiplier;
        const bronko::CallSummary cs = bronko::call_variants(*ix, file_id, p, c);
        if (vcf_path) bronko::write_vcf(vcf_path, reads_path ? reads_path : "", *ix, file_id, cs.records);
        if (pileup_path) bronko::write_pileup_tsv(pileup_path, *ix, file_id, p);
        if (summary) { summary[0] = cs.records.size(); summary[1] = cs.n_major; summary[2] = cs.n_minor; }
        if (cov) { cov[0] = cs.breadth; cov[1] = cs.depth; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// the host twin of bk_sample_consensus on the two depth arrays: letters[genome_len(file_id)], tallies = {positions, called,
// ambiguous, masked, substitutions}
int bh_consensus(const void* h, int file_id, const uint64_t* fwd_depth, const uint64_t* rev_depth, uint64_t min_depth, double min_freq,
                 uint8_t* letters, uint64_t* tallies) {
    try {
        const auto* ix = static_cast<const bronko::Index*>(h);
        if (file_id < 0 || (size_t)file_id >= ix->files.size()) throw std::runtime_error("bh_consensus: no such genome file");
        const size_t n = ix->total_cells() * 4;
        bronko::Pileup p;
        p.fwd_depth.assign(fwd_depth, fwd_depth + n); p.rev_depth.assign(rev_depth, rev_depth + n);
        bronko::ConsensusParams c;
        c.min_depth = min_depth; c.min_freq = min_freq;
        const bronko::Consensus r = bronko::consensus(*ix, file_id, p, c);
        std::memcpy(letters, r.letters.data(), r.letters.size());
        tallies[0] = r.positions; tallies[1] = r.called; tallies[2] = r.ambiguous; tallies[3] = r.masked; tallies[4] = r.substitutions;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_consensus_fasta(const void* h, int file_id, const char* path, const char* stem, const uint8_t* letters, uint64_t n) {
    try { bronko::write_consensus_fasta(path, stem, *static_cast<const bronko::Index*>(h), file_id, letters, n); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --regions / --region-window: regions travel as [n][4] u32 (file_id, seq, start, end), their names joined by '\n' ----------
namespace {
std::vector<bronko::Region> regions_of(const uint32_t* regs, const char* names, uint64_t n) {
    std::vector<bronko::Region> out((size_t)n);
    const char* at = names;
    for (uint64_t i = 0; i < n; i++) {
        out[i].file_id = (int)regs[i * 4]; out[i].seq = regs[i * 4 + 1]; out[i].start = regs[i * 4 + 2]; out[i].end = regs[i * 4 + 3];
        out[i].name = ".";
        if (at) {
            const char* nl = strchr(at, '\n');
            out[i].name = nl ? std::string(at, nl) : std::string(at);
            at = nl ? nl + 1 : nullptr;
        }
    }
    return out;
}
// *n regions, *names_len bytes of joined names; both written only where they fit cap / names_cap
int regions_out(const std::vector<bronko::Region>& r, uint64_t cap, uint32_t* regs, char* names, uint64_t names_cap, uint64_t* n, uint64_t* names_len) {
    std::string joined;
    for (size_t i = 0; i < r.size(); i++) joined += (i ? "\n" : "") + r[i].name;
    *n = r.size();
    if (names_len) *names_len = joined.size() + 1;
    if (regs && r.size() <= cap)
        for (size_t i = 0; i < r.size(); i++) { regs[i * 4] = (uint32_t)r[i].file_id; regs[i * 4 + 1] = r[i].seq; regs[i * 4 + 2] = r[i].start; regs[i * 4 + 3] = r[i].end; }
    if (names && joined.size() + 1 <= names_cap) std::memcpy(names, joined.c_str(), joined.size() + 1);
    return 0;
}
}  // namespace

// read_bed + resolve_bed of a --regions file against the index
int bh_bed_regions(const void* h, const char* path, uint64_t cap, uint32_t* regs, char* names, uint64_t names_cap, uint64_t* n, uint64_t* names_len) {
    try {
        const auto* ix = static_cast<const bronko::Index*>(h);
        return regions_out(bronko::resolve_bed(*ix, bronko::read_bed(path), path), cap, regs, names, names_cap, n, names_len);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_window_regions(const void* h, uint64_t window, uint64_t cap, uint32_t* regs, uint64_t* n) {
    try { return regions_out(bronko::window_regions(*static_cast<const bronko::Index*>(h), window), cap, regs, nullptr, 0, n, nullptr); }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// the host twin of bk_sample_region_depths on the two depth arrays: rows[regions of file_id][5] = sum, min, max, median, covered;
// tallies = {rows, full, partial, empty}
int bh_region_depths(const void* h, int file_id, const uint64_t* fwd_depth, const uint64_t* rev_depth, const uint32_t* regs, uint64_t n, uint64_t min_depth,
                     uint64_t* rows, uint64_t* tallies) {
    try {
        const auto* ix = static_cast<const bronko::Index*>(h);
        if (file_id >= (int)ix->files.size()) throw std::runtime_error("bh_region_depths: no such genome file");
        const size_t cells4 = ix->total_cells() * 4;
        bronko::Pileup p;
        p.fwd_depth.assign(fwd_depth, fwd_depth + cells4); p.rev_depth.assign(rev_depth, rev_depth + cells4);
        const bronko::RegionReport r = bronko::region_depths(*ix, file_id, p, regions_of(regs, nullptr, n), min_depth);
        for (size_t i = 0; i < r.rows.size(); i++) {
            const bronko::RegionDepth& o = r.rows[i];
            const uint64_t v[5] = {o.sum, o.min, o.max, o.median, o.covered};
            std::memcpy(rows + i * 5, v, sizeof v);
        }
        tallies[0] = r.rows.size(); tallies[1] = r.full; tallies[2] = r.partial; tallies[3] = r.empty;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_regions_tsv(const void* h, int file_id, const char* path, const uint32_t* regs, const char* names, uint64_t n, const uint64_t* rows, uint64_t n_rows,
                         uint64_t min_depth) {
    try {
        std::vector<bronko::RegionDepth> r((size_t)n_rows);
        for (size_t i = 0; i < r.size(); i++) { r[i].sum = rows[i * 5]; r[i].min = rows[i * 5 + 1]; r[i].max = rows[i * 5 + 2]; r[i].median = rows[i * 5 + 3]; r[i].covered = rows[i * 5 + 4]; }
        bronko::write_regions_tsv(path, *static_cast<const bronko::Index*>(h), file_id, regions_of(regs, names, n), r.data(), n_rows, min_depth);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_kmer_counts(const char* path, int k, const uint64_t* kmers, const uint64_t* counts, uint64_t n, int threads) {
    try { bronko::write_kmer_counts(path, k, kmers, counts, n, threads); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --indels: the host twin of the engine's indel pass (indels.cpp) -------------------------------------------------
// reads joined by '\n'; rows as bk_indel_record (= bronko::IndelEvent), at most cap written, *n their number; span: NULL or
// [total_cells], prefix-summed; counters = {records, anchored, ref_spanning, supporting, discordant}
int bh_indel_events(const void* h, int file_id, const char* reads, int max_len, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint32_t* span,
                    uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::IndelEvent) == 32, "IndelEvent is bk_indel_record");
        const bronko::IndelResult r = bronko::indel_events(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), max_len, max_mismatches);
        const uint64_t c[5] = {r.n.records, r.n.anchored, r.n.ref_spanning, r.n.supporting, r.n.discordant};
        return events_out(r, c, cap, rows, n, span, counters);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_indels_vcf(const void* h, int file_id, const char* path, const char* reads_path, const void* rows, uint64_t n, uint32_t max_len,
                        uint32_t max_mismatches, uint64_t min_reads, uint32_t min_af_ppm) {
    try {
        const auto* ev = static_cast<const bronko::IndelEvent*>(rows);
        bronko::IndelParams p;
        p.max_len = max_len; p.max_mismatches = max_mismatches; p.min_reads = min_reads; p.min_af_ppm = min_af_ppm;
        bronko::write_indels_vcf(path, reads_path ? reads_path : "", *static_cast<const bronko::Index*>(h), file_id,
                                 std::vector<bronko::IndelEvent>(ev, ev + n), p);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --consensus-indels: the host twin of bk_sample_consensus_indels (consensus_indels.cpp) --------------------------
// events as bk_indel_record (n of them: the whole table), span[total_cells] prefix-summed, letters[n_letters] of the genome file:
// '-' is stored at the applied deletions; rows as bk_consensus_indel_record (= bronko::ConsensusIndel), sorted, at most cap
// written, *n_rows their number; tallies = {candidates, accepted, applied, contested, deletions, insertions, deleted_bases,
// inserted_bases, frameshifts}
int bh_consensus_indels(const void* h, int file_id, const void* events, uint64_t n, const uint32_t* span, uint64_t min_depth, double min_freq, uint8_t* letters,
                        uint64_t n_letters, uint64_t cap, void* rows, uint64_t* n_rows, uint64_t* tallies) {
    try {
        static_assert(sizeof(bronko::ConsensusIndel) == 32, "ConsensusIndel is bk_consensus_indel_record");
        const auto* ix = static_cast<const bronko::Index*>(h);
        const auto* ev = static_cast<const bronko::IndelEvent*>(events);
        const bronko::ConsensusIndels r = bronko::consensus_indels(*ix, file_id, std::vector<bronko::IndelEvent>(ev, ev + n),
                                                                   std::vector<uint32_t>(span, span + ix->total_cells()), min_depth, min_freq, letters, n_letters);
        *n_rows = r.events.size();
        if (rows) std::memcpy(rows, r.events.data(), (size_t)std::min<uint64_t>(cap, r.events.size()) * sizeof(bronko::ConsensusIndel));
        if (tallies) {
            const uint64_t t[9] = {r.n.candidates, r.n.accepted, r.n.applied, r.n.contested, r.n.deletions, r.n.insertions, r.n.deleted_bases, r.n.inserted_bases,
                                   r.n.frameshifts};
            std::memcpy(tallies, t, sizeof t);
        }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_consensus_indels_fasta(const void* h, int file_id, const char* path, const char* stem, const uint8_t* letters, uint64_t n, const void* rows,
                                    uint64_t n_rows) {
    try {
        const auto* ev = static_cast<const bronko::ConsensusIndel*>(rows);
        bronko::write_consensus_indels_fasta(path, stem, *static_cast<const bronko::Index*>(h), file_id, letters, n, std::vector<bronko::ConsensusIndel>(ev, ev + n_rows));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_consensus_indels_tsv(const void* h, int file_id, const char* path, const void* rows, uint64_t n_rows, uint64_t min_depth, double min_freq) {
    try {
        const auto* ev = static_cast<const bronko::ConsensusIndel*>(rows);
        bronko::write_consensus_indels_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::ConsensusIndel>(ev, ev + n_rows), min_depth, min_freq);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --junctions: the host twin of the engine's junction pass (junctions.cpp) ----------------------------------------
// reads joined by '\n'; rows as bk_junction_record (= bronko::JunctionEvent), at most cap written, *n their number; span: NULL or
// [total_cells], prefix-summed; counters = {records, anchored, ref_spanning, supporting, short, backward, discordant}
int bh_junction_events(const void* h, int file_id, const char* reads, uint32_t min_len, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint32_t* span,
                       uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::JunctionEvent) == 24, "JunctionEvent is bk_junction_record");
        const bronko::JunctionResult r = bronko::junction_events(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), min_len, max_mismatches);
        const uint64_t c[7] = {r.n.records, r.n.anchored, r.n.ref_spanning, r.n.supporting, r.n.short_, r.n.backward, r.n.discordant};
        return events_out(r, c, cap, rows, n, span, counters);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_junctions_tsv(const void* h, int file_id, const char* path, const void* rows, uint64_t n, uint32_t min_len, uint32_t max_mismatches, uint64_t min_reads) {
    try {
        const auto* ev = static_cast<const bronko::JunctionEvent*>(rows);
        bronko::JunctionParams p;
        p.min_len = min_len; p.max_mismatches = max_mismatches; p.min_reads = min_reads;
        bronko::write_junctions_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::JunctionEvent>(ev, ev + n), p);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --copybacks: the host twin of the engine's copy-back pass (copybacks.cpp) ------------------------------------------
// reads joined by '\n'; rows as bk_copyback_record (= bronko::CopybackEvent), at most cap written, *n their number; span: NULL or
// [total_cells], prefix-summed; counters = {records, same_strand, ref_spanning, switched, supporting, discordant}
int bh_copyback_events(const void* h, int file_id, const char* reads, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint32_t* span, uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::CopybackEvent) == 32, "CopybackEvent is bk_copyback_record");
        const bronko::CopybackResult r = bronko::copyback_events(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), max_mismatches);
        const uint64_t c[6] = {r.n.records, r.n.same_strand, r.n.ref_spanning, r.n.switched, r.n.supporting, r.n.discordant};
        return events_out(r, c, cap, rows, n, span, counters);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_copybacks_tsv(const void* h, int file_id, const char* path, const void* rows, uint64_t n, uint32_t max_mismatches, uint64_t min_reads, uint32_t min_dist) {
    try {
        const auto* ev = static_cast<const bronko::CopybackEvent*>(rows);
        bronko::CopybackParams p;
        p.max_mismatches = max_mismatches; p.min_reads = min_reads; p.min_dist = min_dist;
        bronko::write_copybacks_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::CopybackEvent>(ev, ev + n), p);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --chimeras: the host twin of the engine's chimera pass (chimeras.cpp) ------------------------------------------------
// reads joined by '\n'; rows as bk_chimera_record (= bronko::ChimeraEvent), at most cap written, *n their number; span: NULL or
// [total_cells], prefix-summed; counters = {records, same_strand, ref_spanning, crossed, supporting, discordant}
int bh_chimera_events(const void* h, int file_id, const char* reads, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint32_t* span, uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::ChimeraEvent) == 32, "ChimeraEvent is bk_chimera_record");
        const bronko::ChimeraResult r = bronko::chimera_events(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), max_mismatches);
        const uint64_t c[6] = {r.n.records, r.n.same_strand, r.n.ref_spanning, r.n.crossed, r.n.supporting, r.n.discordant};
        return events_out(r, c, cap, rows, n, span, counters);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_chimeras_tsv(const void* h, int file_id, const char* path, const void* rows, uint64_t n, uint32_t max_mismatches, uint64_t min_reads, uint64_t supporting,
                          uint64_t ref_spanning) {
    try {
        const auto* ev = static_cast<const bronko::ChimeraEvent*>(rows);
        bronko::ChimeraParams p;
        p.max_mismatches = max_mismatches; p.min_reads = min_reads;
        bronko::write_chimeras_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::ChimeraEvent>(ev, ev + n), p, supporting, ref_spanning);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --breakends: the host twin of the engine's breakend pass (breakends.cpp) ----------------------------------------------
// reads joined by '\n'; rows as bk_breakend_record (= bronko::BreakendEvent), at most cap written, *n their number; span: NULL or
// [total_cells], prefix-summed; counters = {records, one_anchor, ref_spanning, supporting, short, through, discordant, unplaced}
int bh_breakend_events(const void* h, int file_id, const char* reads, int min_clip, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint32_t* span,
                       uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::BreakendEvent) == 32, "BreakendEvent is bk_breakend_record");
        const bronko::BreakendResult r = bronko::breakend_events(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), min_clip, max_mismatches);
        const uint64_t c[8] = {r.n.records, r.n.one_anchor, r.n.ref_spanning, r.n.supporting, r.n.short_, r.n.through, r.n.discordant, r.n.unplaced};
        return events_out(r, c, cap, rows, n, span, counters);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// tallies: the ten of the ##breakend_tallies line, in bk_breakend_summary's order
int bh_write_breakends_tsv(const void* h, int file_id, const char* path, const void* rows, uint64_t n, uint32_t min_clip, uint32_t max_mismatches, uint64_t min_reads,
                           const uint64_t* tallies) {
    try {
        const auto* ev = static_cast<const bronko::BreakendEvent*>(rows);
        bronko::BreakendParams p;
        p.min_clip = min_clip; p.max_mismatches = max_mismatches; p.min_reads = min_reads;
        bronko::BreakendTallies t;
        t.records = tallies[0]; t.one_anchor = tallies[1]; t.ref_spanning = tallies[2]; t.supporting = tallies[3]; t.short_ = tallies[4];
        t.through = tallies[5]; t.discordant = tallies[6]; t.unplaced = tallies[7]; t.candidates = tallies[8]; t.reported = tallies[9];
        bronko::write_breakends_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::BreakendEvent>(ev, ev + n), p, t);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --duplications: the host twin of the engine's duplication pass (duplications.cpp) ------------------------------------
// reads joined by '\n'; rows as bk_duplication_record (= bronko::DuplicationEvent), at most cap written, *n their number; span: NULL or
// [total_cells], prefix-summed; counters = {records, anchored, ref_spanning, supporting, short, forward, discordant}
int bh_duplication_events(const void* h, int file_id, const char* reads, uint32_t min_len, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint32_t* span,
                       uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::DuplicationEvent) == 24, "DuplicationEvent is bk_duplication_record");
        const bronko::DuplicationResult r = bronko::duplication_events(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), min_len, max_mismatches);
        const uint64_t c[7] = {r.n.records, r.n.anchored, r.n.ref_spanning, r.n.supporting, r.n.short_, r.n.forward, r.n.discordant};
        return events_out(r, c, cap, rows, n, span, counters);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

int bh_write_duplications_tsv(const void* h, int file_id, const char* path, const void* rows, uint64_t n, uint32_t min_len, uint32_t max_mismatches, uint64_t min_reads) {
    try {
        const auto* ev = static_cast<const bronko::DuplicationEvent*>(rows);
        bronko::DuplicationParams p;
        p.min_len = min_len; p.max_mismatches = max_mismatches; p.min_reads = min_reads;
        bronko::write_duplications_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::DuplicationEvent>(ev, ev + n), p);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --linkage: the host twin of the engine's linkage passes (linkage.cpp) ---------------------------------------------
// reads joined by '\n'; rows as bk_link_row (= bronko::LinkRow), at most cap written, *n their number; counters = {records, placed,
// unplaced, discordant}
int bh_link_rows(const void* h, int file_id, const char* reads, int max_mismatches, uint64_t cap, void* rows, uint64_t* n, uint64_t* counters) {
    try {
        static_assert(sizeof(bronko::LinkRow) == 32 && sizeof(bronko::LinkPair) == 72, "LinkRow is bk_link_row, LinkPair is bk_link_pair");
        const bronko::LinkResult r = bronko::link_rows(*static_cast<const bronko::Index*>(h), file_id, split_lines(reads), max_mismatches);
        *n = r.rows.size();
        if (rows) std::memcpy(rows, r.rows.data(), (size_t)std::min<uint64_t>(cap, r.rows.size()) * sizeof(bronko::LinkRow));
        if (counters) { counters[0] = r.n.records; counters[1] = r.n.placed; counters[2] = r.n.unplaced; counters[3] = r.n.discordant; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// pairs as bk_link_pair, at most cap written, *n their number
int bh_link_count(const void* h, int file_id, const void* rows, uint64_t n_rows, const uint32_t* sites, uint64_t n_sites, uint32_t max_dist, uint64_t cap,
                  void* pairs, uint64_t* n) {
    try {
        const auto* rw = static_cast<const bronko::LinkRow*>(rows);
        const std::vector<bronko::LinkPair> r = bronko::link_count(*static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::LinkRow>(rw, rw + n_rows),
                                                                   std::vector<uint32_t>(sites, sites + n_sites), max_dist);
        *n = r.size();
        if (pairs) std::memcpy(pairs, r.data(), (size_t)std::min<uint64_t>(cap, r.size()) * sizeof(bronko::LinkPair));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// recs: n_recs x {cell, ref base, alt base} as three u32; returns the lines written through *lines
int bh_write_linkage_tsv(const void* h, int file_id, const char* path, const uint32_t* recs, uint64_t n_recs, const void* pairs, uint64_t n_pairs,
                         uint32_t max_mismatches, uint32_t max_dist, uint64_t min_reads, uint64_t* lines) {
    try {
        std::vector<bronko::LinkSite> rs((size_t)n_recs);
        for (uint64_t i = 0; i < n_recs; i++) { rs[i].cell = recs[3 * i]; rs[i].ref_base = (uint8_t)recs[3 * i + 1]; rs[i].alt_base = (uint8_t)recs[3 * i + 2]; }
        const auto* pr = static_cast<const bronko::LinkPair*>(pairs);
        bronko::LinkParams p;
        p.max_mismatches = max_mismatches; p.max_dist = max_dist; p.min_reads = min_reads;
        const uint64_t w = bronko::write_linkage_tsv(path, *static_cast<const bronko::Index*>(h), file_id, rs, std::vector<bronko::LinkPair>(pr, pr + n_pairs), p);
        if (lines) *lines = w;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --codons: the host twin of the engine's codon count, the BED reader and the writer (codons.cpp) -----------------------------
// regs: n_regions x {cell0, n_codons}; counts: [codons of all regions][64], the caller's room for them given as cap_codons
int bh_codon_count(const void* h, int file_id, const void* rows, uint64_t n_rows, const uint32_t* regs, uint64_t n_regions, uint64_t cap_codons, uint32_t* counts,
                   uint64_t* n_codons) {
    try {
        static_assert(sizeof(bronko::CodonRegion) == 8, "CodonRegion is bk_codon_region");
        const auto* rw = static_cast<const bronko::LinkRow*>(rows);
        std::vector<bronko::CodonRegion> rg((size_t)n_regions);
        for (uint64_t i = 0; i < n_regions; i++) { rg[i].cell0 = regs[2 * i]; rg[i].n_codons = regs[2 * i + 1]; }
        const std::vector<uint32_t> c = bronko::codon_count(*static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::LinkRow>(rw, rw + n_rows), rg);
        if (n_codons) *n_codons = c.size() / 64;
        if (counts) std::memcpy(counts, c.data(), (size_t)std::min<uint64_t>(cap_codons * 64, c.size()) * sizeof(uint32_t));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// genes travel as [n][5] u32 (cell0, n_codons, seq, start, 1 for the '-' strand), their names joined by '\n'
namespace {
std::vector<bronko::CodonGene> genes_of(const uint32_t* genes, const char* names, uint64_t n) {
    return named_rows_in<5, bronko::CodonGene>(genes, names, n, [](bronko::CodonGene& g, const uint32_t* w) {
        g.reg.cell0 = w[0]; g.reg.n_codons = w[1]; g.seq = w[2]; g.start = w[3]; g.strand = w[4] ? '-' : '+';
    });
}
}  // namespace
// read_codon_bed + resolve_codon_bed; *n genes, *names_len bytes of joined names, both written only where they fit cap / names_cap
int bh_codon_bed(const void* h, int file_id, const char* path, uint64_t cap, uint32_t* genes, char* names, uint64_t names_cap, uint64_t* n, uint64_t* names_len) {
    try {
        return named_rows_out<5>(bronko::resolve_codon_bed(*static_cast<const bronko::Index*>(h), file_id, bronko::read_codon_bed(path), path),
                                 [](const bronko::CodonGene& g, uint32_t* w) { w[0] = g.reg.cell0; w[1] = g.reg.n_codons; w[2] = g.seq; w[3] = g.start; w[4] = g.strand == '-' ? 1u : 0u; },
                                 cap, genes, names, names_cap, n, names_len);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int bh_write_codons_tsv(const void* h, int file_id, const char* path, const uint32_t* genes, const char* names, uint64_t n, const uint32_t* counts, uint64_t n_codons,
                        uint32_t max_mismatches, uint64_t min_reads, double min_freq, uint64_t* lines) {
    try {
        bronko::CodonParams p;
        p.max_mismatches = max_mismatches; p.min_reads = min_reads; p.min_freq = min_freq;
        const uint64_t w = bronko::write_codons_tsv(path, *static_cast<const bronko::Index*>(h), file_id, genes_of(genes, names, n),
                                                    std::vector<uint32_t>(counts, counts + n_codons * 64), p);
        if (lines) *lines = w;
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int bh_translate(const char* triplet) { return bronko::translate(triplet); }

// ---- --haplotypes: the host twin of the engine's haplotype count, the regions and the writer (haplotypes.cpp) --------------------
// regs: n_regions x {cell0, len}; cover, ref_count: [n_regions]; entries: 40 bytes each (bk_hap_entry), written only where they fit cap
int bh_hap_count(const void* h, int file_id, const void* rows, uint64_t n_rows, const uint32_t* regs, uint64_t n_regions, uint32_t* cover, uint32_t* ref_count,
                 uint64_t cap, void* entries, uint64_t* n_entries) {
    try {
        const auto* rw = static_cast<const bronko::LinkRow*>(rows);
        std::vector<bronko::HapRegion> rg((size_t)n_regions);
        for (uint64_t i = 0; i < n_regions; i++) { rg[i].cell0 = regs[2 * i]; rg[i].len = regs[2 * i + 1]; }
        const bronko::HapTable t = bronko::hap_count(*static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::LinkRow>(rw, rw + n_rows), rg);
        if (n_entries) *n_entries = t.entries.size();
        if (cover && n_regions) std::memcpy(cover, t.cover.data(), (size_t)n_regions * sizeof(uint32_t));
        if (ref_count && n_regions) std::memcpy(ref_count, t.ref_count.data(), (size_t)n_regions * sizeof(uint32_t));
        if (entries && t.entries.size() <= cap && !t.entries.empty()) std::memcpy(entries, t.entries.data(), t.entries.size() * sizeof(bronko::HapEntry));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// windows travel as [n][4] u32 (cell0, len, seq, start), their names joined by '\n'
namespace {
std::vector<bronko::HapWindow> windows_of(const uint32_t* wins, const char* names, uint64_t n) {
    return named_rows_in<4, bronko::HapWindow>(wins, names, n, [](bronko::HapWindow& x, const uint32_t* w) { x.reg.cell0 = w[0]; x.reg.len = w[1]; x.seq = w[2]; x.start = w[3]; });
}
int windows_out(const std::vector<bronko::HapWindow>& r, uint64_t cap, uint32_t* wins, char* names, uint64_t names_cap, uint64_t* n, uint64_t* names_len) {
    return named_rows_out<4>(r, [](const bronko::HapWindow& x, uint32_t* w) { w[0] = x.reg.cell0; w[1] = x.reg.len; w[2] = x.seq; w[3] = x.start; }, cap, wins, names, names_cap,
                             n, names_len);
}
}  // namespace
// read_hap_bed + resolve_hap_bed (path) or hap_windows (path null); *n windows, *names_len bytes of joined names, both written only where they fit
int bh_hap_regions(const void* h, int file_id, const char* path, uint64_t window, uint64_t step, uint64_t cap, uint32_t* wins, char* names, uint64_t names_cap, uint64_t* n,
                   uint64_t* names_len) {
    try {
        const bronko::Index& ix = *static_cast<const bronko::Index*>(h);
        return windows_out(path ? bronko::resolve_hap_bed(ix, file_id, bronko::read_hap_bed(path), path) : bronko::hap_windows(ix, file_id, window, step), cap, wins, names,
                           names_cap, n, names_len);
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// stats: lines written, regions without cover, distinct haplotypes
int bh_write_haplotypes_tsv(const void* h, int file_id, const char* path, const uint32_t* wins, const char* names, uint64_t n, const uint32_t* cover,
                            const uint32_t* ref_count, const void* entries, uint64_t n_entries, uint32_t max_mismatches, uint64_t min_reads, double min_freq, uint64_t* stats) {
    try {
        bronko::HapParams p;
        p.max_mismatches = max_mismatches; p.min_reads = min_reads; p.min_freq = min_freq;
        bronko::HapTable t;
        t.cover.assign(cover, cover + n); t.ref_count.assign(ref_count, ref_count + n);
        const auto* en = static_cast<const bronko::HapEntry*>(entries);
        t.entries.assign(en, en + n_entries);
        const bronko::HapStats st = bronko::write_haplotypes_tsv(path, *static_cast<const bronko::Index*>(h), file_id, windows_of(wins, names, n), t, p);
        if (stats) { stats[0] = st.lines; stats[1] = st.no_cover; stats[2] = st.distinct; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --read-pileup: the host twin of the engine's read pileup and the writer (read_pileup.cpp) ------------------------------------
// cells: 48 bytes each (bk_read_pileup_cell), one per position of the genome file, written only where they fit cap; *n_cells: how many
int bh_read_pileup_count(const void* h, int file_id, const void* rows, uint64_t n_rows, uint32_t end_dist, uint64_t cap, void* cells, uint64_t* n_cells) {
    try {
        const auto* rw = static_cast<const bronko::LinkRow*>(rows);
        const std::vector<bronko::ReadPileupCell> c =
            bronko::read_pileup_count(*static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::LinkRow>(rw, rw + n_rows), end_dist);
        if (n_cells) *n_cells = c.size();
        if (cells && c.size() <= cap && !c.empty()) std::memcpy(cells, c.data(), c.size() * sizeof(bronko::ReadPileupCell));
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// stats: cells with at least one row, the sum of all fwd and rev counters
int bh_write_read_pileup_tsv(const void* h, int file_id, const char* path, const void* cells, uint64_t n_cells, uint32_t max_mismatches, uint32_t end_dist, uint64_t* stats) {
    try {
        bronko::ReadPileupParams p;
        p.max_mismatches = max_mismatches; p.end_dist = end_dist;
        const auto* c = static_cast<const bronko::ReadPileupCell*>(cells);
        const bronko::ReadPileupStats st = bronko::write_read_pileup_tsv(path, *static_cast<const bronko::Index*>(h), file_id, std::vector<bronko::ReadPileupCell>(c, c + n_cells), p);
        if (stats) { stats[0] = st.covered; stats[1] = st.bases; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --distances: the host twin of the engine's cohort kernels, the clusterer and the three writers (cohort.cpp) ---------------------
// letters: n rows of `positions` bytes; diff, compared: [n_rows][n] each, either may be null
int bh_cohort_distances(const uint8_t* letters, uint64_t n, uint64_t positions, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared, uint32_t threads) {
    try {
        if (!letters) throw std::runtime_error("bh_cohort_distances: letters is null");
        bronko::cohort_distances_host(letters, n, positions, row0, n_rows, diff, compared, threads);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// the matrices go to the clusterer in blocks of block_rows rows (0: all at once); cluster, size: [n]; stats: clusters, the largest's size
int bh_cohort_clusters(uint64_t n, uint64_t positions, const uint32_t* diff, const uint32_t* compared, uint64_t threshold, double min_breadth, uint64_t block_rows,
                       uint32_t* cluster, uint32_t* size, uint32_t* stats) {
    try {
        bronko::CohortClusterer cl(n, positions, threshold, min_breadth);
        const uint64_t step = block_rows ? block_rows : std::max<uint64_t>(n, 1);
        for (uint64_t r = 0; r < n; r += step) cl.add_rows(r, std::min(step, n - r), diff + r * n, compared + r * n);
        const bronko::CohortClusters c = cl.finish();
        for (uint64_t i = 0; i < n; i++) { cluster[i] = c.cluster[i]; size[i] = c.size[i]; }
        if (stats) { stats[0] = c.n_clusters; stats[1] = c.largest; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// names: the samples' names joined by '\n'
int bh_write_cohort_distances_tsv(const char* path, const char* names, const uint32_t* diff) {
    try { bronko::write_cohort_distances_tsv(path, split_lines(names), diff); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int bh_write_cohort_compared_tsv(const char* path, const char* names, const uint32_t* compared) {
    try { bronko::write_cohort_compared_tsv(path, split_lines(names), compared); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// --mst: the twin of bk_cohort_mst (Prim), the rooting and the writer.  edges: [n - 1][4] lo, hi, diff, compared; nearest: [n][3] sample,
// diff, compared; either may be null
uint32_t bh_cohort_min_compared(double min_breadth, uint64_t positions) { return bronko::cohort_min_compared(min_breadth, positions); }
int bh_cohort_mst(const uint8_t* letters, uint64_t n, uint64_t positions, uint32_t min_compared, uint32_t threads, uint32_t* edges, uint64_t* n_edges, uint32_t* nearest) {
    try {
        if (!letters || !n_edges) throw std::runtime_error("bh_cohort_mst: letters or n_edges is null");
        const bronko::CohortMst m = bronko::cohort_mst_host(bronko::cohort_pack_host(letters, n, positions, threads), min_compared, threads);
        *n_edges = m.edges.size();
        for (size_t k = 0; edges && k < m.edges.size(); k++) { edges[4 * k] = m.edges[k].lo; edges[4 * k + 1] = m.edges[k].hi; edges[4 * k + 2] = m.edges[k].diff; edges[4 * k + 3] = m.edges[k].compared; }
        for (size_t i = 0; nearest && i < m.nearest.size(); i++) { nearest[3 * i] = m.nearest[i].sample; nearest[3 * i + 1] = m.nearest[i].diff; nearest[3 * i + 2] = m.nearest[i].compared; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
static std::vector<bronko::CohortMstEdge> mst_edges_of(const uint32_t* edges, uint64_t n_edges) {
    std::vector<bronko::CohortMstEdge> ev((size_t)n_edges);
    for (size_t k = 0; k < ev.size(); k++) ev[k] = bronko::CohortMstEdge{edges[4 * k], edges[4 * k + 1], edges[4 * k + 2], edges[4 * k + 3]};
    return ev;
}
// parent, diff, compared, component, size: [n]; stats: components, the largest's size, the longest edge
int bh_cohort_root_forest(uint64_t n, const uint32_t* edges, uint64_t n_edges, uint32_t* parent, uint32_t* diff, uint32_t* compared, uint32_t* component, uint32_t* size, uint32_t* stats) {
    try {
        const bronko::CohortForest f = bronko::root_forest(n, mst_edges_of(edges, n_edges));
        for (uint64_t i = 0; i < n; i++) { parent[i] = f.parent[i]; diff[i] = f.diff[i]; compared[i] = f.compared[i]; component[i] = f.component[i]; size[i] = f.size[i]; }
        if (stats) { stats[0] = f.n_components; stats[1] = f.largest; stats[2] = f.longest; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int bh_write_cohort_mst_tsv(const char* path, const char* names, const uint32_t* edges, uint64_t n_edges, const uint32_t* nearest, double min_breadth, uint32_t min_compared) {
    try {
        const std::vector<std::string> nm = split_lines(names);
        std::vector<bronko::CohortMstNearest> nr(nm.size());
        for (size_t i = 0; i < nr.size(); i++) nr[i] = bronko::CohortMstNearest{nearest[3 * i], nearest[3 * i + 1], nearest[3 * i + 2]};
        bronko::write_cohort_mst_tsv(path, nm, bronko::root_forest(nm.size(), mst_edges_of(edges, n_edges)), nr, min_breadth, min_compared);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int bh_write_cohort_clusters_tsv(const char* path, const char* names, const uint32_t* cluster, const uint32_t* size, uint64_t threshold, double min_breadth) {
    try {
        const std::vector<std::string> nm = split_lines(names);
        bronko::CohortClusters c;
        c.cluster.assign(cluster, cluster + nm.size()); c.size.assign(size, size + nm.size());
        bronko::write_cohort_clusters_tsv(path, nm, c, threshold, min_breadth);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

// ---- --contamination: the host twins, the scanner and the three writers (cohort.cpp) ------------------------------------------------
// fwd, rev: four counts a position; masks: a byte a position (may be null); tallies: positions, mixed, present
int bh_minor_mask(const uint64_t* fwd, const uint64_t* rev, uint64_t positions, uint64_t min_reads, double min_freq, uint8_t* masks, uint64_t* tallies) {
    try {
        if (!fwd || !rev) throw std::runtime_error("bh_minor_mask: fwd or rev is null");
        const bronko::MinorSummary s = bronko::minor_mask_host(fwd, rev, positions, min_reads, min_freq, masks);
        if (tallies) { tallies[0] = s.positions; tallies[1] = s.mixed; tallies[2] = s.present; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// letters, masks: n rows of `positions` bytes; explained: [n_rows][n], minor_sites: [n_rows], either may be null
int bh_cohort_explained(const uint8_t* letters, const uint8_t* masks, uint64_t n, uint64_t positions, uint64_t row0, uint64_t n_rows, uint32_t* explained,
                        uint32_t* minor_sites, uint32_t threads) {
    try {
        if (!letters || !masks) throw std::runtime_error("bh_cohort_explained: letters or masks is null");
        bronko::cohort_explained_host(letters, masks, n, positions, row0, n_rows, explained, minor_sites, threads);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
namespace {
bronko::Contamination scan_contamination(uint64_t n, const uint32_t* diff, const uint32_t* compared, const uint32_t* explained, uint32_t min_sites, double min_share,
                                         uint64_t block_rows) {
    bronko::ContaminationScanner sc(n, min_sites, min_share);
    const uint64_t step = block_rows ? block_rows : std::max<uint64_t>(n, 1);
    for (uint64_t r = 0; r < n; r += step) sc.add_rows(r, std::min(step, n - r), diff + r * n, compared + r * n, explained + r * n);
    return sc.finish();
}
}  // namespace
// the three [n][n] matrices go to the scanner in blocks of block_rows rows (0: all at once).  flagged: [cap][5] recipient, source, diff,
// compared, explained, written where they fit; *n_flagged: how many; best: [n][3] source (0xffffffff: none), explained, diff; counts: [n];
// stats: recipients, the largest explained
int bh_contamination_scan(uint64_t n, const uint32_t* diff, const uint32_t* compared, const uint32_t* explained, uint32_t min_sites, double min_share, uint64_t block_rows,
                          uint32_t* flagged, uint64_t cap, uint64_t* n_flagged, uint32_t* best, uint32_t* counts, uint32_t* stats) {
    try {
        const bronko::Contamination c = scan_contamination(n, diff, compared, explained, min_sites, min_share, block_rows);
        if (n_flagged) *n_flagged = c.flagged.size();
        for (size_t k = 0; flagged && k < c.flagged.size() && k < cap; k++) {
            const auto& x = c.flagged[k];
            flagged[5 * k] = x.recipient; flagged[5 * k + 1] = x.source; flagged[5 * k + 2] = x.diff; flagged[5 * k + 3] = x.compared; flagged[5 * k + 4] = x.explained;
        }
        for (uint64_t i = 0; i < n; i++) {
            if (best) { best[3 * i] = c.best[i].source; best[3 * i + 1] = c.best[i].explained; best[3 * i + 2] = c.best[i].diff; }
            if (counts) counts[i] = c.n_flagged[i];
        }
        if (stats) { stats[0] = c.recipients; stats[1] = c.largest; }
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}
int bh_write_cohort_explained_tsv(const char* path, const char* names, const uint32_t* explained) {
    try { bronko::write_cohort_explained_tsv(path, split_lines(names), explained); return 0; }
    catch (const std::exception& e) { g_err = e.what(); return -1; }
}
// which: 0 OUT/<genome>.contamination.tsv, 1 OUT/<genome>.mixture.tsv, of the scanner's result over the three matrices
int bh_write_contamination_tsv(int which, const char* path, const char* names, const uint32_t* diff, const uint32_t* compared, const uint32_t* explained,
                               const uint32_t* minor_sites, uint64_t minor_min_reads, double minor_min_freq, uint32_t min_sites, double min_share, uint64_t block_rows) {
    try {
        const std::vector<std::string> nm = split_lines(names);
        bronko::ContaminationParams p;
        p.minor_min_reads = minor_min_reads; p.minor_min_freq = minor_min_freq; p.min_sites = min_sites; p.min_share = min_share;
        const bronko::Contamination c = scan_contamination(nm.size(), diff, compared, explained, min_sites, min_share, block_rows);
        const std::vector<uint32_t> ms(minor_sites, minor_sites + nm.size());
        if (which == 0) bronko::write_contamination_tsv(path, nm, c, ms, p);
        else bronko::write_mixture_tsv(path, nm, c, ms, p);
        return 0;
    } catch (const std::exception& e) { g_err = e.what(); return -1; }
}

void bh_clean_sample_id(const char* path, char* buf, size_t n) {
    const std::string s = bronko::clean_sample_id(path);
    snprintf(buf, n, "%s", s.c_str());
}

}  // extern "C"
