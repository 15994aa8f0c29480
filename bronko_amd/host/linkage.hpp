// linkage.hpp -- `bronko call --linkage`: the host twin of the engine's linkage passes (bk_linkage.hip) and the writer of
// OUT/<stem>.linkage.tsv.  The rule is stated in include/bronko_hip.h (bk_link_enable) and DESIGN.md section L; this file restates it
// in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the Python restatement
// (tests/linkage_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr int kLinkMaxMismatches = 8;
constexpr uint32_t kLinkMaxSites = 65536, kLinkMaxPairs = 1u << 20, kLinkMaxDist = 65519;   // BK_LINK_MAX_*

// bk_link_row: a placed record.  mm[3 i ..] = the i-th mismatch ascending by offset: offset from cell0 (16 bits, little endian), the
// record's base there in the reference's orientation (A C G T = 0 1 2 3); zero from n_mm on
struct LinkRow {
    uint32_t cell0 = 0;
    uint16_t n = 0;
    uint8_t strand = 0, n_mm = 0;
    uint8_t mm[24] = {};
};
// mismatch t of a row's mm (or of a HapEntry's, whose offsets are from its region's first cell)
inline uint32_t mm_offset(const uint8_t* mm, int t) { return (uint32_t)mm[3 * t] | ((uint32_t)mm[3 * t + 1] << 8); }
inline uint32_t mm_base(const uint8_t* mm, int t) { return mm[3 * t + 2]; }
// the row's base at `cell`: one of its mismatches, else `ref_base` (the reference's there)
inline uint32_t row_base(const LinkRow& row, uint32_t cell, uint32_t ref_base) {
    for (int t = 0; t < row.n_mm; t++)
        if (mm_offset(row.mm, t) == cell - row.cell0) return mm_base(row.mm, t);
    return ref_base;
}
// bk_link_pair: count[4 bA + bB]
struct LinkPair {
    uint32_t site_a = 0, site_b = 0;
    uint32_t count[16] = {};
};
struct LinkCounters { uint64_t records = 0, placed = 0, unplaced = 0, discordant = 0; };
struct LinkResult {
    std::vector<LinkRow> rows;            // in the order of the records
    LinkCounters n;
};
struct LinkParams {
    uint32_t max_mismatches = 8, max_dist = 1000;
    uint64_t min_reads = 1;
};
// one VCF record as the linkage file sees it: its cell among the genome file's cells, its 2-bit bases
struct LinkSite {
    uint32_t cell = 0;
    uint8_t ref_base = 0, alt_base = 0;
};

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
LinkResult link_rows(const Index& ix, int file, const std::vector<std::string>& reads, int max_mismatches);

// The 16 counters of every pair i < j of `sites` (strictly ascending cells) in one sequence and at most max_dist apart, in (i, j)
// order.  Throws for sites that are not strictly ascending, more than kLinkMaxSites of them or more than kLinkMaxPairs pairs.
std::vector<LinkPair> link_count(const Index& ix, int file, const std::vector<LinkRow>& rows, const std::vector<uint32_t>& sites, uint32_t max_dist);

// the distinct cells of the records, ascending: the sites of bk_sample_linkage
std::vector<uint32_t> link_sites(const std::vector<LinkSite>& recs);

// OUT/<stem>.linkage.tsv: three ## lines, the column line, one line per pair of records (A:a, B:b), A before B, whose pair is in
// `pairs` and whose cover >= min_reads, ordered by (cell A, a, cell B, b).  Returns the lines written.
uint64_t write_linkage_tsv(const std::string& out_path, const Index& ix, int file, std::vector<LinkSite> recs, const std::vector<LinkPair>& pairs,
                           const LinkParams& p);

}  // namespace bronko
