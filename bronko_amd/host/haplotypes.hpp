// haplotypes.hpp -- `bronko call --haplotypes`: the host twin of the engine's haplotype count (bk_haplotypes.hip), the regions of the
// BED file or the window tiling, and the writer of OUT/<stem>.haplotypes.tsv.  The rule is stated in include/bronko_hip.h
// (bk_sample_haplotypes) and DESIGN.md section H; hap_count restates it in plain C++ with a std::map over the rows of linkage.hpp, so
// that the CPU tests can hold it against the Python restatement (tests/haplotypes_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "caller.hpp"
#include "index.hpp"
#include "linkage.hpp"

namespace bronko {

constexpr uint32_t kHapMaxRegions = 4096, kHapMaxLen = 65520;   // BK_HAP_MAX_REGIONS, BK_HAP_MAX_LEN

// bk_hap_region: the forward-strand cells [cell0, cell0 + len)
struct HapRegion {
    uint32_t cell0 = 0, len = 0;
};
// bk_hap_entry: one distinct non-empty haplotype of a region; mm as in a LinkRow, the offsets from the region's first cell
struct HapEntry {
    uint32_t region = 0, count = 0;
    uint8_t n_mm = 0, pad[7] = {};
    uint8_t mm[24] = {};
};
static_assert(sizeof(HapEntry) == 40, "HapEntry is bk_hap_entry");
// what the count gives: per region the spanning rows and those of them without a substitution inside it; the other haplotypes by
// region, then by list (a proper prefix first) -- the order of bk_sample_download_haplotypes
struct HapTable {
    std::vector<uint32_t> cover, ref_count;
    std::vector<HapEntry> entries;
};
// one region as the output names it
struct HapWindow {
    HapRegion reg;
    uint32_t seq = 0, start = 0;         // sequence within the genome file, 0-based start in it
    std::string name;                    // BED column 4, "." when the file gives none and in window mode
};
struct HapParams {
    uint32_t max_mismatches = 8;
    uint64_t min_reads = 5;
    double min_freq = 0.03;
};
struct HapStats {
    uint64_t lines = 0, no_cover = 0, distinct = 0;   // lines written, regions with cover 0, distinct haplotypes (the reference's included)
};

// Throws for a region of no cell or of more than kHapMaxLen, outside the genome file or across a sequence border, and for more than
// kHapMaxRegions regions.
HapTable hap_count(const Index& ix, int file, const std::vector<LinkRow>& rows, const std::vector<HapRegion>& regions);

// read_bed's lines (strand is not looked at).  Throws, the file and the line named, for a line longer than kHapMaxLen and for more than
// kHapMaxRegions lines.
std::vector<BedLine> read_hap_bed(const std::string& path);
// resolve_bed's regions of genome file `file`, in the lines' order
std::vector<HapWindow> resolve_hap_bed(const Index& ix, int file, const std::vector<BedLine>& bed, const std::string& path);
// the windows [i step, i step + window) that lie wholly inside a sequence, over every sequence of genome file `file`; throws for a
// window outside 1..kHapMaxLen, a step below 1 and more than kHapMaxRegions windows
std::vector<HapWindow> hap_windows(const Index& ix, int file, uint64_t window, uint64_t step);
inline std::vector<HapRegion> hap_regions(const std::vector<HapWindow>& w) {
    std::vector<HapRegion> r;
    for (const HapWindow& x : w) r.push_back(x.reg);
    return r;
}

// OUT/<stem>.haplotypes.tsv: three ##hap_* lines, the column line, then per region in the order given its haplotypes -- the reference's
// included -- ranked by count descending, then by list ascending; a line for each with count >= min_reads and count >= min_freq *
// cover.  t: hap_count's or the engine's for hap_regions(windows).
HapStats write_haplotypes_tsv(const std::string& out_path, const Index& ix, int file, const std::vector<HapWindow>& windows, const HapTable& t, const HapParams& p);

}  // namespace bronko
