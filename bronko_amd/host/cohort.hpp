// cohort.hpp -- --distances: the host twin of the engine's cohort kernels (bk_cohort.hip), the single-linkage clusterer and the writers
// of OUT/<genome>.distances.tsv, .compared.tsv and .clusters.tsv.  The rule is stated in include/bronko_hip.h (bk_cohort_set) and
// DESIGN.md section W; tests/cohort_ref.py restates it.  The `bronko` binary never computes distances here: the twin is the tests'
// and the measurements' yardstick, the clusterer and the writers are the product's.  --mst: the twin of bk_cohort_mst (the same
// split: the twin is a yardstick), the rooting of a forest's edges and the writer of OUT/<genome>.mst.tsv (DESIGN.md section Y;
// tests/mst_ref.py restates the rule).  --contamination: the twins of the present-mask kernel and of the explained kernel (yardsticks),
// the scanner of the flagged pairs and the writers of OUT/<genome>.explained.tsv, .contamination.tsv and .mixture.tsv (DESIGN.md
// section Z; tests/contamination_ref.py restates the rule).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace bronko {

// The letters of n samples as three bit planes per sample, [sample][W] each, W = ceil(positions / 64): valid (the letter is exactly
// one of ACGT), b0 and b1 (the 2-bit code A C G T = 0 1 2 3, zero where not valid)
struct CohortPlanes {
    uint64_t n = 0, positions = 0, W = 0;
    std::vector<uint64_t> valid, b0, b1;
};
CohortPlanes cohort_pack_host(const uint8_t* letters, uint64_t n, uint64_t positions, unsigned threads);

// diff and compared of rows [row0, row0 + n_rows) against all n columns, row-major, on `threads` host threads; either output may be null
void cohort_distances_host(const CohortPlanes& p, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared, unsigned threads);
// ... from the letters (n rows of `positions` bytes)
void cohort_distances_host(const uint8_t* letters, uint64_t n, uint64_t positions, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared,
                           unsigned threads);

// --clusters T --cluster-min-breadth B: samples i != j are linked iff diff[i][j] <= T and (double)compared[i][j] >= B * (double)positions;
// clusters are the connected components (single linkage), numbered from 1 in the order of their first sample.  The rows arrive in
// blocks, in any order: a union-find over the samples, the matrix is never held.
struct CohortClusters {
    std::vector<uint32_t> cluster, size;    // per sample: its cluster's number and size
    uint32_t n_clusters = 0, largest = 0;
};
class CohortClusterer {
public:
    CohortClusterer(uint64_t n, uint64_t positions, uint64_t threshold, double min_breadth);
    void add_rows(uint64_t row0, uint64_t n_rows, const uint32_t* diff, const uint32_t* compared);
    CohortClusters finish();
private:
    uint64_t n_, positions_, threshold_;
    double min_breadth_;
    std::vector<uint32_t> parent_;
    uint32_t find(uint32_t x);
};

// OUT/<genome>.distances.tsv and OUT/<genome>.compared.tsv: "sample" and the samples' names, tab-separated; then per sample its name
// and its row.  The rows arrive in blocks, in order.  Throws std::runtime_error when the file cannot be written.
class CohortMatrixWriter {
public:
    CohortMatrixWriter(const std::string& path, const std::vector<std::string>& names);
    ~CohortMatrixWriter();
    CohortMatrixWriter(const CohortMatrixWriter&) = delete;
    CohortMatrixWriter& operator=(const CohortMatrixWriter&) = delete;
    void add_rows(uint64_t row0, uint64_t n_rows, const uint32_t* values);
    void close();
private:
    std::string path_;
    const std::vector<std::string>& names_;
    FILE* f_ = nullptr;
    uint64_t next_ = 0;
};
void write_cohort_distances_tsv(const std::string& path, const std::vector<std::string>& names, const uint32_t* diff);       // [n][n]
void write_cohort_compared_tsv(const std::string& path, const std::vector<std::string>& names, const uint32_t* compared);    // [n][n]
// OUT/<genome>.clusters.tsv: "##cluster_threshold=T", "##cluster_min_breadth=B" (%g), "sample<TAB>cluster<TAB>size", a line per sample in input order
void write_cohort_clusters_tsv(const std::string& path, const std::vector<std::string>& names, const CohortClusters& c, uint64_t threshold, double min_breadth);

// --mst --mst-min-breadth B: the cohort's minimum spanning forest (the rule: include/bronko_hip.h, bk_cohort_mst).  A pair i < j is
// admissible iff compared >= 1 and compared >= min_compared; edges are ordered by (diff, i, j); the forest is the unique minimum
// spanning forest of the admissible graph under that order; nearest[i] is the admissible j != i with the least (diff, j).
constexpr uint32_t kCohortNone = 0xffffffffu;
struct CohortMstEdge { uint32_t lo, hi, diff, compared; };          // lo < hi
struct CohortMstNearest { uint32_t sample, diff, compared; };       // sample = kCohortNone: none
struct CohortMst {
    std::vector<CohortMstEdge> edges;       // ascending in the edge order
    std::vector<CohortMstNearest> nearest;  // per sample
};
// the smallest integer c with (double)c >= min_breadth * (double)positions: the compare --clusters makes, as a count
uint32_t cohort_min_compared(double min_breadth, uint64_t positions);
// The twin of bk_cohort_mst, by another algorithm: Prim per component from the component's first sample, one row of the distances at
// a time, always the least edge that leaves the tree under (diff, lo, hi).  O(n^2 W) time, O(n) memory.
CohortMst cohort_mst_host(const CohortPlanes& p, uint32_t min_compared, unsigned threads);
// The forest rooted: a component's root is its smallest sample, every other sample's parent is its neighbour on the path to the root;
// components are numbered from 1 in the order of their first sample, as clusters are.
struct CohortForest {
    std::vector<uint32_t> parent, diff, compared;   // per sample: its parent (kCohortNone: a root) and the edge to it
    std::vector<uint32_t> component, size;          // per sample: its component's number and size
    uint32_t n_components = 0, largest = 0, longest = 0;   // longest: the largest diff of an edge
};
CohortForest root_forest(uint64_t n, const std::vector<CohortMstEdge>& edges);
// OUT/<genome>.mst.tsv: "##mst_min_breadth=B" (%g), "##mst_min_compared=C", "sample parent diff compared component size nearest
// nearest_diff nearest_compared" (tab-separated), a line per sample in input order; "." for a root's parent, diff and compared and
// for the three nearest columns of a sample without a nearest neighbour
void write_cohort_mst_tsv(const std::string& path, const std::vector<std::string>& names, const CohortForest& f, const std::vector<CohortMstNearest>& nearest,
                          double min_breadth, uint32_t min_compared);

// --contamination: which sample's alleles another carries (the rule: include/bronko_hip.h, bk_sample_minor_alleles and
// bk_cohort_set_minor; tests/contamination_ref.py restates it).  The twins are yardsticks, the scanner and the
// writers are the product's.
struct MinorSummary { uint64_t positions = 0, mixed = 0, present = 0; };
// The twin of bk_sample_minor_alleles over `positions` consecutive cells: fwd and rev hold four counts a cell (A C G T), masks gets a
// byte a cell (may be null).  Bit b iff tot[b] >= min_reads and (double)tot[b] >= min_freq * (double)depth.
MinorSummary minor_mask_host(const uint64_t* fwd, const uint64_t* rev, uint64_t positions, uint64_t min_reads, double min_freq, uint8_t* masks);
// The twin of bk_cohort_set_minor and bk_cohort_explained: explained ([n_rows][n]) and minor_sites ([n_rows]) of rows
// [row0, row0 + n_rows) of n samples' letters and masks (n rows of `positions` bytes each); either output may be null
void cohort_explained_host(const uint8_t* letters, const uint8_t* masks, uint64_t n, uint64_t positions, uint64_t row0, uint64_t n_rows, uint32_t* explained,
                           uint32_t* minor_sites, unsigned threads);

struct ContaminationParams {
    uint64_t minor_min_reads = 10;          // --minor-min-reads, --minor-min-freq: what the masks were made with (the files' header lines)
    double minor_min_freq = 0.03;
    uint32_t min_sites = 3;                 // --contamination-min-sites S
    double min_share = 0.75;                // --contamination-min-share P
};
struct ContaminationPair { uint32_t recipient, source, diff, compared, explained; };
struct ContaminationBest { uint32_t source = kCohortNone, explained = 0, diff = 0; };   // source = kCohortNone: none
struct Contamination {
    std::vector<ContaminationPair> flagged;     // ordered by (recipient, source)
    std::vector<ContaminationBest> best;        // per sample
    std::vector<uint32_t> n_flagged;            // per sample: the sources it is flagged for
    uint32_t recipients = 0, largest = 0;       // samples flagged at least once; the largest explained of any pair i != j
};
// An ordered pair (i, j), i != j, is flagged iff explained >= S and (double)explained >= P * (double)diff; best[i] is the j != i with
// the largest explained >= 1, ties to the smaller diff, then to the earlier sample.  The rows arrive in blocks, in any order; the
// matrices are never held: O(n + flagged) memory.
class ContaminationScanner {
public:
    ContaminationScanner(uint64_t n, uint32_t min_sites, double min_share);
    void add_rows(uint64_t row0, uint64_t n_rows, const uint32_t* diff, const uint32_t* compared, const uint32_t* explained);
    Contamination finish();
private:
    uint64_t n_;
    uint32_t min_sites_;
    double min_share_;
    Contamination c_;
};
// OUT/<genome>.explained.tsv: the layout of .distances.tsv, the row is the recipient
void write_cohort_explained_tsv(const std::string& path, const std::vector<std::string>& names, const uint32_t* explained);   // [n][n]
// OUT/<genome>.contamination.tsv: "##minor_min_reads=R", "##minor_min_freq=F" (%g), "##contamination_min_sites=S",
// "##contamination_min_share=P" (%g), "recipient source diff compared explained share minor_sites minor_share" (tab-separated), a line
// per flagged pair; share = explained / diff and minor_share = explained / minor_sites[recipient], from the integers, four decimals,
// truncated
void write_contamination_tsv(const std::string& path, const std::vector<std::string>& names, const Contamination& c, const std::vector<uint32_t>& minor_sites,
                             const ContaminationParams& p);
// OUT/<genome>.mixture.tsv: the same four header lines, "sample minor_sites flagged best_source explained diff share", a line per
// sample in input order; "." in the last four columns of a sample without a best source
void write_mixture_tsv(const std::string& path, const std::vector<std::string>& names, const Contamination& c, const std::vector<uint32_t>& minor_sites,
                       const ContaminationParams& p);

}  // namespace bronko
