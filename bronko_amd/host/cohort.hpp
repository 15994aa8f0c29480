// cohort.hpp -- --distances: the host twin of the engine's cohort kernels (bk_cohort.hip), the single-linkage clusterer and the writers
// of OUT/<genome>.distances.tsv, .compared.tsv and .clusters.tsv.  The rule is stated in include/bronko_hip.h (bk_cohort_set) and
// DESIGN.md section W; tests/cohort_ref.py restates it.  The `bronko` binary never computes distances here: the twin is the tests'
// and the measurements' yardstick, the clusterer and the writers are the product's.
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

}  // namespace bronko
