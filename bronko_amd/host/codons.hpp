// codons.hpp -- `bronko call --codons`: the host twin of the engine's codon count (bk_codons.hip), the reader of the coding regions'
// BED file, the translation and the writer of OUT/<stem>.codons.tsv.  The rule is stated in include/bronko_hip.h (bk_sample_codons)
// and DESIGN.md section T; codon_count restates it in plain C++ over the rows of linkage.hpp, so that the CPU tests can hold it
// against the Python restatement (tests/codons_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "caller.hpp"
#include "index.hpp"
#include "linkage.hpp"

namespace bronko {

constexpr uint32_t kCodonMaxRegions = 4096, kCodonMaxCodons = 1u << 18;   // BK_CODON_MAX_*

// bk_codon_region: the forward-strand cells [cell0, cell0 + 3 n_codons)
struct CodonRegion {
    uint32_t cell0 = 0, n_codons = 0;
};
// one line of the --codons BED file against the index: its region, where it lies and how it is read
struct CodonGene {
    CodonRegion reg;
    uint32_t seq = 0, start = 0;         // sequence within the genome file, 0-based start in it
    char strand = '+';
    std::string name;                    // column 4, "." when the file gives none
};
struct CodonParams {
    uint32_t max_mismatches = 8;
    uint64_t min_reads = 5;
    double min_freq = 0.03;
};

// count[codon][16 b0 + 4 b1 + b2] for the codons of `regions`, numbered in the order given: the rows that cover all three cells of the
// codon with those bases.  Throws for a region of no codon, outside the genome file or across a sequence border, and above the limits.
std::vector<uint32_t> codon_count(const Index& ix, int file, const std::vector<LinkRow>& rows, const std::vector<CodonRegion>& regions);

// read_bed's lines with column 6 as the strand ('+', '-'; '.' or absent: '+').  Throws, the file and the line named, for another
// strand, an end - start that is no positive multiple of 3, more than kCodonMaxRegions lines or kCodonMaxCodons codons.
std::vector<BedLine> read_codon_bed(const std::string& path);
// resolve_bed's regions of genome file `file`, in the lines' order
std::vector<CodonGene> resolve_codon_bed(const Index& ix, int file, const std::vector<BedLine>& bed, const std::string& path);
inline std::vector<CodonRegion> codon_regions(const std::vector<CodonGene>& genes) {
    std::vector<CodonRegion> r;
    for (const CodonGene& g : genes) r.push_back(g.reg);
    return r;
}

// the standard code (NCBI table 1) of three letters ACGT; '*' a stop, 'X' with any other letter
char translate(const char* triplet);

// OUT/<stem>.codons.tsv: three ##codon_* lines, the column line, one line per (codon, triplet other than the reference's) with
// count >= min_reads and count >= min_freq * cover, by gene in the file's order, codon number, forward triplet.  counts: codon_count's
// or the engine's for codon_regions(genes).  Returns the lines written.
uint64_t write_codons_tsv(const std::string& out_path, const Index& ix, int file, const std::vector<CodonGene>& genes, const std::vector<uint32_t>& counts,
                          const CodonParams& p);

}  // namespace bronko
