// cli.hpp -- what the three units of the `bronko` binary share: the logger, die, hip_check, the parsed arguments (a field per
// option, one record of the options given) and the settings of one `bronko call` (cli.cpp: the option table, the rules, build, main;
// reads.cpp: FASTQ files -> engine; call_run.cpp: engines, lanes and the per-sample report units).
#pragma once
#include <algorithm>
#include <bitset>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/bronko_hip.h"
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

namespace bronko {

bool log_enabled(int lvl);   // 0 error, 1 warn, 2 info, 3 debug, 4 trace (simple_logger levels, call.rs:31-43)
void logf(int lvl, const char* tag, const char* target, const std::string& msg);
#define LOG_ERROR(t, m) logf(0, "ERROR", t, m)
#define LOG_WARN(t, m) logf(1, "WARN", t, m)
#define LOG_INFO(t, m) logf(2, "INFO", t, m)
#define LOG_DEBUG(t, m) logf(3, "DEBUG", t, m)
#define LOG_TRACE(t, m) logf(4, "TRACE", t, m)

[[noreturn]] void die(const char* target, const std::string& msg);   // `error!(..); std::process::exit(1)`
void hip_check(int rc, const char* what);                            // a bk_* status: dies with bk_last_error()

// ---- argument parsing (clap derive surface of cli.rs) -------------------------------------------------------
// One field per option that takes a value or is a switch; which options were given at all is one record, a bit per row of the option
// table (cli.cpp), read by the option's long name.
struct Args {
    std::string mode;
    std::bitset<128> given_rows;
    bool given(const char* name) const;   // cli.cpp; name: the option's long name, as the table has it
    bool has_genomes() const { return given("--genomes"); }
    bool has_db() const { return given("--db"); }
    bool has_primers() const { return given("--primers"); }
    bool has_regions() const { return given("--regions"); }
    bool has_region_window() const { return given("--region-window"); }
    bool has_codons() const { return given("--codons"); }
    bool has_haplotypes() const { return given("--haplotypes"); }
    bool has_hap_window() const { return given("--hap-window"); }
    bool has_clusters() const { return given("--clusters"); }
    std::vector<std::string> genomes, reads, first_pairs, second_pairs;
    std::string db;
    long kmer = 21;                 // consts.rs:3
    long min_kmers = 3;             // consts.rs:5
    bool use_full_kmer = false;
    long n_fixed = 2;               // consts.rs:17
    double min_af = 0.03;
    bool no_end_filter = false, no_strand_filter = false, no_strand_balance_filter = false;
    double balance_ratio = 0.1;
    long n_per_strand = 2;
    double strand_odds = 6.0;
    long min_depth = 300;
    long min_variant_depth = 3;
    double noise_multiplier = 1.5;
    long min_base_qual = 0;         // --min-base-qual: bases below this Phred+33 quality are N before k-mer counting (0: off)
    std::string primers;            // --primers: FASTA of amplicon primers trimmed from the read ends (empty: none)
    long primer_mismatches = 1;     // --primer-mismatches: Hamming distance a primer match may have (0..3)
    std::vector<std::string> adapters;   // --adapter: 3' adapters cut off the reads, preset names or sequences (empty: none)
    long adapter_min_overlap = 5;   // --adapter-min-overlap: bases of an adapter's start that count as a match at the read's end
    double adapter_error_rate = 0.1;   // --adapter-error-rate: mismatches allowed per compared base (0..0.3)
    bool consensus = false;         // --consensus: <DIR>/<stem>.consensus.fa, one IUPAC letter per position of the selected genome
    long consensus_min_depth = 10;  // --consensus-min-depth: positions with less depth are N
    double consensus_min_freq = 0.5;   // --consensus-min-freq: share of the depth the letter's bases must reach together (0..1)
    std::string regions;            // --regions: BED file of the regions whose depths go to <DIR>/<stem>.regions.tsv (empty: none)
    long region_window = 0;         // --region-window: tile every sequence with windows of this many positions instead
    long region_min_depth = 10;     // --region-min-depth: a position with at least this depth counts as covered
    bool indels = false;            // --indels: <DIR>/<stem>.indels.vcf, short insertions and deletions from the reads
    long indel_max_len = 32;        // --indel-max-len: longest insertion or deletion looked for (1..32)
    long indel_max_mismatches = 2;  // --indel-max-mismatches: substitutions a record may have beside its indel (0..8)
    long indel_min_reads = 5;       // --indel-min-reads: supporting records an event needs
    double indel_min_af = 0.03;     // --indel-min-af: support / (support + reference-spanning records) an event needs (default: --min-af)
    bool consensus_indels = false;  // --consensus-indels: the sample's indels in <DIR>/<stem>.consensus.fa, <DIR>/<stem>.consensus_indels.tsv (needs --consensus and --indels)
    bool junctions = false;         // --junctions: <DIR>/<stem>.junctions.tsv, long deletions and subgenomic-RNA junctions from the reads
    long junction_min_len = 33;     // --junction-min-len: shortest jump counted as a junction (with 33 it begins where --indels ends)
    long junction_max_mismatches = 2;   // --junction-max-mismatches: substitutions a record may have beside its junction (0..8)
    long junction_min_reads = 5;    // --junction-min-reads: supporting records a junction needs
    bool copybacks = false;         // --copybacks: <DIR>/<stem>.copybacks.tsv, strand-switch (copy-back, snap-back) junctions from the reads
    long copyback_max_mismatches = 2;   // --copyback-max-mismatches: substitutions a record may have beside its turn (0..8)
    long copyback_min_reads = 5;    // --copyback-min-reads: supporting records an event needs
    long copyback_min_dist = 0;     // --copyback-min-dist: cells an event's two breakpoints must lie apart
    bool chimeras = false;          // --chimeras: <DIR>/<stem>.chimeras.tsv, junctions between two sequences of the genome file from the reads
    long chimera_max_mismatches = 2;    // --chimera-max-mismatches: substitutions a record may have beside its junction (0..8)
    long chimera_min_reads = 5;     // --chimera-min-reads: supporting records an event needs
    bool breakends = false;         // --breakends: <DIR>/<stem>.breakends.tsv, reads that leave the reference (an anchor at one end only)
    long breakend_min_clip = 20;    // --breakend-min-clip: clipped bases a record needs to support an event (16..65519)
    long breakend_max_mismatches = 2;   // --breakend-max-mismatches: substitutions the held part of a record may have (0..8)
    long breakend_min_reads = 5;    // --breakend-min-reads: supporting records an event needs
    bool duplications = false;      // --duplications: <DIR>/<stem>.duplications.tsv, tandem duplications and circular-origin reads
    long duplication_min_len = 33;  // --duplication-min-len: shortest backward jump counted (with 33 it begins where --indels ends)
    long duplication_max_mismatches = 2;   // --duplication-max-mismatches: substitutions a record may have beside its junction (0..8)
    long duplication_min_reads = 5; // --duplication-min-reads: supporting records an event needs
    bool linkage = false;           // --linkage: <DIR>/<stem>.linkage.tsv, which of the sample's substitutions the same reads carry
    long link_max_mismatches = 8;   // --link-max-mismatches: substitutions a placed record may have (0..8)
    long link_max_dist = 1000;      // --link-max-dist: pairs of substitutions at most this far apart are counted (1..65519)
    long link_min_reads = 1;        // --link-min-reads: records that cover both positions a pair needs to be written
    std::string codons;             // --codons: BED file of the coding regions whose codons go to <DIR>/<stem>.codons.tsv (empty: none)
    long codon_min_reads = 5;       // --codon-min-reads: records that carry a triplet for it to be written
    double codon_min_freq = 0.03;   // --codon-min-freq: count / cover a triplet needs to be written (default: --min-af)
    long codon_max_mismatches = 8;  // --codon-max-mismatches: substitutions a placed record may have (0..8; the row store's, shared with --linkage)
    std::string haplotypes;         // --haplotypes: BED file of the regions whose read haplotypes go to <DIR>/<stem>.haplotypes.tsv (empty: none)
    long hap_window = 0;            // --hap-window: tile every sequence with windows of this many positions instead (1..65520)
    long hap_step = 0;              // --hap-step: positions from one window's start to the next (default: the window)
    long hap_min_reads = 5;         // --hap-min-reads: records that carry a haplotype for it to be written
    double hap_min_freq = 0.03;     // --hap-min-freq: count / cover a haplotype needs to be written (default: --min-af)
    long hap_max_mismatches = 8;    // --hap-max-mismatches: substitutions a placed record may have (0..8; the row store's, shared with --linkage and --codons)
    bool haps() const { return has_haplotypes() || has_hap_window(); }
    bool read_pileup = false;       // --read-pileup: <DIR>/<stem>.read_pileup.tsv, per position the bases the placed reads carry, by strand and near their ends
    long read_pileup_end = 10;      // --read-pileup-end: a base within this many positions of a read's end counts as near it (0..255)
    long read_pileup_max_mismatches = 8;   // --read-pileup-max-mismatches: substitutions a placed record may have (0..8; the row store's, shared with the other three)
    bool distances = false;         // --distances: <DIR>/<genome>.distances.tsv and .compared.tsv, the samples' pairwise consensus distances (needs --consensus)
    long clusters = 0;              // --clusters T: <DIR>/<genome>.clusters.tsv, single-linkage clusters of the samples at most T apart (needs --distances)
    double cluster_min_breadth = 0.9;   // --cluster-min-breadth B: share of the genome's positions a pair must have compared to be linked (0..1)
    bool mst = false;               // --mst: <DIR>/<genome>.mst.tsv, the minimum spanning forest of the samples' distances (needs --distances)
    double mst_min_breadth = 0.9;   // --mst-min-breadth B: share of the genome's positions a pair must have compared to be an edge (0..1)
    bool contamination = false;     // --contamination: <DIR>/<genome>.explained.tsv, .contamination.tsv and .mixture.tsv, which sample's alleles another carries (needs --distances)
    long minor_min_reads = 10;      // --minor-min-reads R: reads of a base for it to be present at a position (at least 1)
    double minor_min_freq = 0.03;   // --minor-min-freq F: share of the position's depth a present base reaches (0..1; not given: the value of --min-af)
    long contamination_min_sites = 3;      // --contamination-min-sites S: explained positions a flagged pair has at least (at least 1)
    double contamination_min_share = 0.75; // --contamination-min-share P: share of the pair's differences that are explained, at least (0..1)
    std::string output;             // default depends on the mode
    bool pileup = false, alignment = false, keep_kmer_info = false;
    long threads = 4;
    bool debug = false, verbose = false;
};

// threads a FASTQ file's inflate may take (pargz.hpp): -t over the files that are open at the same time.  With many files open at
// once the files are the parallelism: 16 lanes x 4 inflate threads measured slower than 16 x 1 -- 3.5 s against 2.8 s for
// 32 x 1 M reads -- while 7 lanes x 9 threads, a hundred-genome index, gain 19.2 -> 13.8 s.
inline unsigned inflate_threads(long threads, size_t open_files) {
    if (const char* it = getenv("BRONKO_INFLATE_THREADS")) return (unsigned)std::max(1, atoi(it));
    return open_files > 8 ? 1u : (unsigned)std::max<size_t>(1, std::min<size_t>(64, (size_t)threads / open_files));
}

// The settings of one `bronko call` that the reader threads and the per-sample code share: made once from the checked arguments
// (make_call_config, cli.cpp) before the first reader thread starts, const from then on.
struct CallConfig {
    int k = 21;                             // (the records a reader thread packs drop runs shorter than k)
    int min_qual = 0;                       // --min-base-qual: bases below '!' + min_qual are N
    std::vector<std::string> primers;       // --primers: the file's records
    int primer_mismatches = 1;
    std::vector<std::string> adapters;      // --adapter: preset names expanded
    uint32_t adapter_min_overlap = 5;
    double adapter_error_rate = 0.1;
    unsigned ahead_inflate_threads = 1;     // for the files that are read ahead of their turn: -t over the files ReadAhead has open at once
    CallParams cp;                          // the printed strand odds (strand_odds, caller.hpp)
    bk_call_params call;                    // bk_sample_call
    bk_consensus_params consensus;          // bk_sample_consensus (--consensus)
    bk_minor_params minor;                  // bk_sample_minor_alleles (--contamination)
    ContaminationParams contamination;      // ... the scanner's thresholds and the values the three files' header lines print
    // --regions: the file's data lines (resolved against the index once it is open, call_run.cpp); --region-window; neither: no report
    std::string regions_path;
    std::vector<BedLine> bed;
    uint64_t region_window = 0;
    uint64_t region_min_depth = 10;         // bk_sample_region_depths
    // --indels: bk_indels_enable / bk_sample_indels and the values the .indels.vcf header prints
    bool indels = false;
    IndelParams indel;
    // --junctions: bk_junctions_enable / bk_sample_junctions and the values the .junctions.tsv header prints
    bool junctions = false;
    JunctionParams junction;
    // --copybacks: bk_copybacks_enable / bk_sample_copybacks and the values the .copybacks.tsv header prints
    bool copybacks = false;
    CopybackParams copyback;
    // --chimeras: bk_chimeras_enable / bk_sample_chimeras and the values the .chimeras.tsv header prints
    bool chimeras = false;
    ChimeraParams chimera;
    // --breakends: bk_breakends_enable / bk_sample_breakends and the values the .breakends.tsv header prints
    bool breakends = false;
    BreakendParams breakend;
    // --duplications: bk_duplications_enable / bk_sample_duplications and the values the .duplications.tsv header prints
    bool duplications = false;
    DuplicationParams duplication;
    // --linkage: bk_link_enable / bk_sample_linkage and the values the .linkage.tsv header prints
    bool linkage = false;
    LinkParams link;
    // --codons: the file's lines (resolved against the index once it is open, call_run.cpp), bk_sample_codons and the values the
    // .codons.tsv header prints; codon.max_mismatches is the row store's when --linkage is not given (equal to link's when it is)
    std::string codons_path;
    std::vector<BedLine> codon_bed;
    CodonParams codon;
    bool codons() const { return !codons_path.empty(); }
    // --haplotypes / --hap-window: the file's lines or the tiling (resolved against the index once it is open, call_run.cpp),
    // bk_sample_haplotypes and the values the .haplotypes.tsv header prints; hap.max_mismatches is the row store's when neither
    // --linkage nor --codons is given (equal to theirs when one is)
    std::string haps_path;
    std::vector<BedLine> hap_bed;
    uint64_t hap_window = 0, hap_step = 0;
    HapParams hap;
    bool haps() const { return !haps_path.empty() || hap_window > 0; }
    // --read-pileup: bk_sample_read_pileup and the values the .read_pileup.tsv header prints; read_pile.max_mismatches is the row
    // store's when none of the other three is given (equal to theirs when one is)
    bool read_pileup = false;
    ReadPileupParams read_pile;
    bool row_store() const { return linkage || codons() || haps() || read_pileup; }   // bk_link_enable
    uint32_t row_store_mismatches() const {
        return linkage ? link.max_mismatches : codons() ? codon.max_mismatches : haps() ? hap.max_mismatches : read_pile.max_mismatches;
    }
    bool region_report() const { return !regions_path.empty() || region_window > 0; }
    // reads are trimmed on the engine: a packed batch carries end flags and goes to bk_push_reads_packed_ends
    bool trims() const { return !primers.empty() || !adapters.empty(); }
};

Index build_index_any(const char* T, int k, const std::vector<std::string>& genomes, int threads);   // cli.cpp
int call_samples(const Args& a, const CallConfig& cfg);                                                // call_run.cpp

}  // namespace bronko
