// caller.hpp -- host stages after the pileup: reference selection, baseline-noise filter, variant calling and
// the output writers (product code).  Reference behaviour: /root/reference/src/call.rs:422-502 (selection),
// :792-967 (noise), :969-1150 (calls), :648-695 (pileup TSV), :698-732 (overview TSV), :735-774 (VCF);
// file naming /root/reference/src/util.rs:30-50.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

// The four OutputData arrays of one sample (call.rs:1235-1239,1451-1454), flat in (file, seq, pos, base) order,
// plus map_kmers' per-genome statistics (call.rs:1272), already summed over mate files.
struct Pileup {
    std::vector<uint64_t> fwd_depth, rev_depth, fwd_nk, rev_nk;   // total_cells * 4 each
    std::vector<uint64_t> stats;                                   // n_files * 3: perfect, variant, unique
    std::vector<uint8_t>  present;                                 // n_files
};

struct CallParams {                  // CallArgs fields that reach calling (cli.rs:92-135; defaults consts.rs)
    int      k = 21;
    double   min_af = 0.03;
    bool     no_end_filter = false;
    bool     no_strand_filter = false;
    bool     no_strand_balance_filter = false;
    double   strand_balance_ratio = 0.1;
    uint64_t n_per_strand = 2;
    double   strand_odds_max = 6.0;
    uint64_t min_depth = 300;
    uint64_t min_variant_depth = 3;
    double   variant_multiplier = 1.5;
};

struct VcfRecord {                   // call.rs:776-789
    int      seq_id;
    uint64_t pos;                    // 1-based
    uint8_t  ref_base, alt_base;     // 2-bit codes
    uint64_t fwd_ref, rev_ref, fwd_alt, rev_alt, depth;
    double   af, sor;
};

struct CallSummary {
    std::vector<VcfRecord> records;
    uint64_t n_major = 0, n_minor = 0;
    double breadth = 0.0, depth = 0.0;
};

// call.rs:422-450 / :452-502.  Ties are broken towards the lower file id (upstream: hash-map order).  -1 = None.
int pick_best_genome(const Index& ix, const std::vector<uint64_t>& stats, const std::vector<uint8_t>& present);

// call.rs:799-967 -- only Noise.max is consumed downstream (call.rs:1107); returned per position.
std::vector<double> baseline_noise_max(const uint64_t* fwd4, const uint64_t* rev4, uint64_t len);

// The strand odds ratio of an alternative base as the VCF prints it (call.rs:1059-1096), from its DP4 counts: strand_odds_max + 1
// without the strand filter, -1.0 where the strand balance filter lets the base through untested.  *tested: the ratio was computed.
double strand_odds(uint64_t fwd_ref, uint64_t rev_ref, uint64_t fwd_alt, uint64_t rev_alt, const CallParams& prm, bool* tested = nullptr);

// call.rs:969-1150 over the sequences of `file_id` in metadata order.
CallSummary call_variants(const Index& ix, int file_id, const Pileup& p, const CallParams& prm);

// --consensus: the rule of include/bronko_hip.h (bk_sample_consensus) in plain C++, for the genome's positions in metadata order.
// The product's letters come from the device (consensus_kernel); this is its twin for the tests that need no GPU.
struct ConsensusParams {
    uint64_t min_depth = 10;
    double   min_freq = 0.5;
};
struct Consensus {
    std::string letters;             // one per position of the genome, in (sequence, position) order
    uint64_t positions = 0, called = 0, ambiguous = 0, masked = 0, substitutions = 0;
};
Consensus consensus(const Index& ix, int file_id, const Pileup& p, const ConsensusParams& prm);
// OUT/<stem>.consensus.fa: one record per sequence of the genome, in metadata order; header ">" stem "|" the sequence-name
// token of the VCF's CHROM column; the letters (`n` of them, genome_len(file_id)) in lines of 60
void write_consensus_fasta(const std::string& out_path, const std::string& stem, const Index& ix, int file_id, const uint8_t* letters, uint64_t n);

// --regions / --region-window: the rule of include/bronko_hip.h (bk_sample_region_depths) in plain C++.  The product's numbers
// come from the device (region_depth_kernel); region_depths is its twin for the tests that need no GPU.
struct BedLine {                     // one data line of a BED file: columns 1-3, column 4 or "."
    std::string chrom, name;
    std::string strand;              // column 6 as the file gives it, "" when absent: read by --codons alone (codons.hpp)
    uint64_t start = 0, end = 0;
    size_t line = 0;                 // 1-based, as an editor counts
};
struct Region {                      // [start, end) of sequence `seq` (index within the file) of genome file `file_id`
    int file_id = 0;
    uint32_t seq = 0, start = 0, end = 0;
    std::string name;                // "." when the BED gives none, and in window mode
};
struct RegionDepth { uint64_t sum = 0, min = 0, max = 0, median = 0, covered = 0; };
struct RegionReport {
    std::vector<RegionDepth> rows;   // the regions of the genome file, in the order given
    uint64_t full = 0, partial = 0, empty = 0;
};
constexpr size_t kMaxBedRegions = 65536;          // data lines of a --regions file
constexpr uint64_t kMaxRegions = 1ull << 22;      // BK_MAX_REGIONS: resolved regions, windows
// The data lines of a BED file, plain or gzip: tab-separated chrom, 0-based start, end (exclusive), optional name; column 6 is kept as it is and never looked at here, other columns
// are ignored, blank lines and lines beginning '#', "track" or "browser" are skipped, a trailing CR is tolerated.  Throws with the
// file and the line named: a missing column, a start or end that is no number, start >= end, more than kMaxBedRegions lines.
std::vector<BedLine> read_bed(const std::string& path);
// Each line's chrom against the CHROM token (as the VCF prints it) of every sequence of every genome file: one region per sequence
// that carries the name, in the lines' order.  Throws (file and line named) for a name found in no file and an end beyond the sequence.
std::vector<Region> resolve_bed(const Index& ix, const std::vector<BedLine>& bed, const std::string& path);
// [iW, min((i + 1)W, len)) over every sequence of every genome file; throws above kMaxRegions windows (the message says to raise W)
std::vector<Region> window_regions(const Index& ix, uint64_t window);
// the numbers of the regions of `file_id` among `regions` (the others are passed over), literally: copy the depths, sort, index (L - 1) / 2
RegionReport region_depths(const Index& ix, int file_id, const Pileup& p, const std::vector<Region>& regions, uint64_t min_depth);
// OUT/<stem>.regions.tsv: "##min_depth=D", the header line, one line per region of `file_id` among `regions` (rows: theirs, in
// order; file_id < 0: the two header lines).  The mean from integers: m = 100 * sum / L as m / 100 "." two digits of m % 100.
void write_regions_tsv(const std::string& out_path, const Index& ix, int file_id, const std::vector<Region>& regions,
                       const RegionDepth* rows, uint64_t n_rows, uint64_t min_depth);

std::string clean_sample_id(const std::string& path);                               // util.rs:30-50
void write_vcf(const std::string& out_path, const std::string& reads_path_as_given, const Index& ix, int file_id,
               const std::vector<VcfRecord>& recs);                                 // call.rs:735-774
// --keep-kmer-info: <output>/<stem>_counts.txt of one reads file (call.rs:1202-1211), "KMER\tCOUNT\n" per entry, k-mers as MSB-first
// 2-bit codes (A=0 C=1 G=2 T=3) written in upper-case ACGT, in the order given; formatted on `threads` threads
void write_kmer_counts(const std::string& out_path, int k, const uint64_t* kmers, const uint64_t* counts, uint64_t n, int threads);
void write_pileup_tsv(const std::string& out_path, const Index& ix, int file_id, const Pileup& p);  // call.rs:648-695

struct OverviewRow {                 // call.rs:138-149
    std::string filename, selected_genome;
    uint64_t n_major, n_minor;
    double breadth, depth;
    uint64_t n_perfect, n_variant, n_unmapped;
};
void write_overview_tsv(const std::string& out_path, const std::vector<OverviewRow>& rows);  // call.rs:698-732

// --alignment (call.rs:504-628): per selected genome with at least three samples of breadth >= 0.90, OUT/<genome>.mfa =
// the columns of all positions at which some sample has a major variant (AF >= 0.5), reference row first, then one row per
// sample (its alternative base where it has a major variant, the reference base elsewhere).  Columns are ordered by
// (sequence name, position).  Upstream emits genomes and samples in hash-map order; here: index order, input order.
// `note` receives the "Skipping ..." / "Building ..." log lines of call.rs:521,541,551.
struct SampleCalls {
    std::string filename, selected_genome;
    double breadth;
    std::vector<VcfRecord> records;
};
void write_alignments(const std::string& out_dir, const Index& ix, const std::vector<SampleCalls>& samples,
                      void (*note)(const std::string&));

}  // namespace bronko
