// file_cells.hpp -- one genome file of the index as the host twins and the report writers see it: its cells, where its sequences start
// and which of them holds a cell, the CHROM token of a sequence name, and whether a region of cells lies in the file and inside one
// sequence.  Used by the row-store passes (linkage.cpp, codons.cpp, haplotypes.cpp, read_pileup.cpp), by the writers of the six event
// passes, and through AnchorGenome (anchor_genome.hpp) by every twin that places records.
#pragma once
#include <cctype>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

// One genome file's cells.  Signed, because the twins place records by differences of cells that may fall in front of the file.
struct FileCells {
    int64_t cell0 = 0;                               // first cell of the file among all cells of the index
    std::string text;                                // the file's cells (upper-cased FASTA letters)
    std::vector<int64_t> first;                      // first cell of each sequence, relative to cell0; one more entry: the end
    FileCells(const Index& ix, int file) {
        if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("no such genome file");
        for (int f = 0; f < file; f++) cell0 += (int64_t)ix.genome_len((size_t)f);
        for (const SeqMeta& s : ix.files[(size_t)file].sequences) {
            first.push_back((int64_t)text.size());
            for (uint8_t c : s.seq) text.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
        }
        first.push_back((int64_t)text.size());
    }
    // the sequence that holds a cell (relative to cell0); the last one for every cell behind it
    int seq_of(int64_t cell) const {
        int s = 0;
        while (s + 2 < (int)first.size() && first[(size_t)s + 1] <= cell) s++;
        return s;
    }
    // the cells [lo, hi) of the index (lo < hi) lie in the file and in one sequence; `who` begins the message
    void check_region(const std::string& who, uint64_t lo, uint64_t hi) const {
        const int64_t a = (int64_t)lo - cell0, b = (int64_t)hi - cell0;
        if (a < 0 || b > (int64_t)text.size()) throw std::runtime_error(who + " lies outside the genome file");
        for (size_t s = 0; s + 1 < first.size(); s++)
            if (a >= first[s] && a < first[s + 1] && b > first[s + 1]) throw std::runtime_error(who + " crosses a sequence border");
    }
};

// the CHROM token of a sequence name as write_vcf prints it: its first run of characters that are not white space
inline std::string chrom_of(const std::string& name) {
    size_t a = 0;
    while (a < name.size() && isspace((unsigned char)name[a])) a++;
    size_t b = a;
    while (b < name.size() && !isspace((unsigned char)name[b])) b++;
    return name.substr(a, b - a);
}

}  // namespace bronko
