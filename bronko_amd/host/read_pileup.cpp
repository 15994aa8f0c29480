// read_pileup.cpp -- the host twin of bk_read_pileup.hip and the .read_pileup.tsv writer (read_pileup.hpp).
#include "read_pileup.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

#include "file_cells.hpp"

namespace bronko {

namespace {

int base_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

}  // namespace

// Written from the rule, not from the kernel: difference arrays per base for the stretches a row covers with the reference's base --
// the cells between its substitutions -- and single increments at the substitutions; one prefix sum per counter at the end.
std::vector<ReadPileupCell> read_pileup_count(const Index& ix, int file, const std::vector<LinkRow>& rows, uint32_t end_dist) {
    if (end_dist > kReadPileupMaxEnd) throw std::runtime_error("read_pileup_count: end_dist must be 0..255, got " + std::to_string(end_dist));
    const FileCells g(ix, file);
    const int64_t n_cells = (int64_t)g.text.size(), E = (int64_t)end_dist;
    std::vector<ReadPileupCell> cells((size_t)n_cells);
    // ref_diff[which][c]: +1 where a stretch of rows that carry the reference's base begins, -1 behind it; which = strand 0, strand 1, near
    std::vector<int64_t> ref_diff[3];
    for (auto& d : ref_diff) d.assign((size_t)n_cells + 1, 0);
    const auto stretch = [&](int which, int64_t lo, int64_t hi) { if (lo < hi) { ref_diff[which][(size_t)lo]++; ref_diff[which][(size_t)hi]--; } };
    for (size_t r = 0; r < rows.size(); r++) {
        const LinkRow& row = rows[r];
        const int64_t c0 = (int64_t)row.cell0 - g.cell0, n = row.n, end = c0 + n;
        if (c0 < 0 || end > n_cells || n == 0 || row.n_mm > kLinkMaxMismatches || row.strand > 1)
            throw std::runtime_error("read_pileup_count: row " + std::to_string(r) + " is no placed record of the genome file");
        // the cells at which the row is near an end: [c0, near_lo) and [near_hi, end); every cell when n <= 2 E
        const int64_t near_lo = n <= 2 * E ? end : c0 + E, near_hi = n <= 2 * E ? end : end - E;
        int64_t at = c0;                                           // the reference's base from here up to the next substitution
        for (int t = 0; t <= row.n_mm; t++) {
            const int64_t cell = t < row.n_mm ? c0 + (int64_t)mm_offset(row.mm, t) : end;
            if (cell < at || cell > end || (t < row.n_mm && cell == end)) throw std::runtime_error("read_pileup_count: row " + std::to_string(r) + " has a mismatch outside its cells");
            stretch(row.strand, at, cell);
            stretch(2, at, std::min(cell, near_lo));
            stretch(2, std::max(at, near_hi), cell);
            if (t < row.n_mm) {
                ReadPileupCell& c = cells[(size_t)cell];
                const uint32_t b = mm_base(row.mm, t) & 3u;
                (row.strand ? c.rev : c.fwd)[b]++;
                if (cell < near_lo || cell >= near_hi) c.near[b]++;
            }
            at = cell + 1;
        }
    }
    int64_t acc[3] = {0, 0, 0};
    for (int64_t c = 0; c < n_cells; c++) {
        for (int w = 0; w < 3; w++) acc[w] += ref_diff[w][(size_t)c];
        const int b = base_code(g.text[(size_t)c]);
        if (b < 0) {                                               // no row lies over a letter that is not ACGT
            if (acc[0] || acc[1] || acc[2]) throw std::runtime_error("read_pileup_count: a row lies over a reference letter that is not ACGT");
            continue;
        }
        cells[(size_t)c].fwd[b] += (uint32_t)acc[0]; cells[(size_t)c].rev[b] += (uint32_t)acc[1]; cells[(size_t)c].near[b] += (uint32_t)acc[2];
    }
    return cells;
}

ReadPileupStats write_read_pileup_tsv(const std::string& out_path, const Index& ix, int file, const std::vector<ReadPileupCell>& cells, const ReadPileupParams& p) {
    if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("write_read_pileup_tsv: no such genome file");
    if (cells.size() != ix.genome_len((size_t)file)) throw std::runtime_error("write_read_pileup_tsv: the cells are not the genome file's");
    FILE* fp = fopen(out_path.c_str(), "w");
    if (!fp) throw std::runtime_error("Failed to create read pileup output file " + out_path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    fprintf(fp, "##read_pileup_max_mismatches=%u\n##read_pileup_end=%u\n", p.max_mismatches, p.end_dist);
    fputs("reference\tindex\tref\tA\tC\tG\tT\ta\tc\tg\tt\tnear_A\tnear_C\tnear_G\tnear_T\n", fp);
    ReadPileupStats st;
    size_t cell = 0;
    for (const SeqMeta& s : ix.files[(size_t)file].sequences) {
        for (uint64_t i = 0; i < s.len; i++, cell++) {
            const ReadPileupCell& c = cells[cell];
            fprintf(fp, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", s.name.c_str(), (unsigned long long)(i + 1), (char)s.seq[i], c.fwd[0], c.fwd[1], c.fwd[2],
                    c.fwd[3], c.rev[0], c.rev[1], c.rev[2], c.rev[3], c.near[0], c.near[1], c.near[2], c.near[3]);
            uint64_t sum = 0;
            for (int b = 0; b < 4; b++) sum += (uint64_t)c.fwd[b] + c.rev[b];
            st.bases += sum;
            st.covered += sum ? 1 : 0;
        }
    }
    if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write read pileup file " + out_path);
    return st;
}

}  // namespace bronko
