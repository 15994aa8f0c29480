// codons.cpp -- the host twin of bk_codons.hip, the --codons BED reader, the translation and the .codons.tsv writer (codons.hpp).
#include "codons.hpp"

#include <cstdio>
#include <stdexcept>

#include "file_cells.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

void check_regions(const FileCells& g, const std::vector<CodonRegion>& regions) {
    if (regions.size() > kCodonMaxRegions) throw std::runtime_error("codon_count: at most 4096 regions, got " + std::to_string(regions.size()));
    uint64_t total = 0;
    for (size_t i = 0; i < regions.size(); i++) {
        const CodonRegion& r = regions[i];
        const std::string who = "codon_count: region " + std::to_string(i);
        if (r.n_codons == 0) throw std::runtime_error(who + " has no codon");
        g.check_region(who, r.cell0, r.cell0 + 3ull * r.n_codons);
        total += r.n_codons;
    }
    if (total > kCodonMaxCodons) throw std::runtime_error("codon_count: " + std::to_string(total) + " codons, at most 262144 are counted");
}

char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }

}  // namespace

std::vector<uint32_t> codon_count(const Index& ix, int file, const std::vector<LinkRow>& rows, const std::vector<CodonRegion>& regions) {
    const FileCells g(ix, file);
    check_regions(g, regions);
    size_t total = 0;
    for (const CodonRegion& r : regions) total += r.n_codons;
    std::vector<uint32_t> count(total * 64, 0u);
    for (const LinkRow& row : rows) {
        auto base_at = [&](uint32_t cell) { return row_base(row, cell, nt_to_bits((uint8_t)g.text[(size_t)(cell - g.cell0)])); };
        size_t codon = 0;
        for (const CodonRegion& r : regions)
            for (uint32_t i = 0; i < r.n_codons; i++, codon++) {
                const uint32_t c = r.cell0 + 3 * i;
                if (c < row.cell0 || c + 3 > row.cell0 + row.n) continue;
                count[codon * 64 + 16 * base_at(c) + 4 * base_at(c + 1) + base_at(c + 2)]++;
            }
    }
    return count;
}

std::vector<BedLine> read_codon_bed(const std::string& path) {
    std::vector<BedLine> bed = read_bed(path);
    uint64_t codons = 0;
    for (BedLine& b : bed) {
        const std::string where = path + ": line " + std::to_string(b.line);
        if (b.strand.empty() || b.strand == ".") b.strand = "+";
        if (b.strand != "+" && b.strand != "-") throw std::runtime_error(where + ": strand '" + b.strand + "' is neither '+' nor '-' (nor '.')");
        if ((b.end - b.start) % 3 != 0)
            throw std::runtime_error(where + ": a coding region's length is a multiple of 3, " + std::to_string(b.start) + " to " + std::to_string(b.end) + " are " +
                                     std::to_string(b.end - b.start) + " positions");
        codons += (b.end - b.start) / 3;
    }
    if (bed.size() > kCodonMaxRegions) throw std::runtime_error(path + ": " + std::to_string(bed.size()) + " coding regions, at most " + std::to_string(kCodonMaxRegions) + " are counted");
    if (codons > kCodonMaxCodons) throw std::runtime_error(path + ": " + std::to_string(codons) + " codons, at most " + std::to_string(kCodonMaxCodons) + " are counted");
    return bed;
}

std::vector<CodonGene> resolve_codon_bed(const Index& ix, int file, const std::vector<BedLine>& bed, const std::string& path) {
    const FileCells g(ix, file);
    std::vector<CodonGene> out;
    uint64_t codons = 0;
    for (const BedLine& b : bed)
        for (const Region& r : resolve_bed(ix, std::vector<BedLine>{b}, path)) {   // (a chrom no file carries, an end beyond the sequence: its errors)
            if (r.file_id != file) continue;
            CodonGene c;
            c.reg.cell0 = (uint32_t)(g.cell0 + g.first[r.seq] + r.start); c.reg.n_codons = (r.end - r.start) / 3;
            c.seq = r.seq; c.start = r.start; c.strand = b.strand == "-" ? '-' : '+'; c.name = r.name;
            codons += c.reg.n_codons;
            out.push_back(std::move(c));
        }
    if (out.size() > kCodonMaxRegions) throw std::runtime_error(path + ": " + std::to_string(out.size()) + " coding regions, at most " + std::to_string(kCodonMaxRegions) + " are counted");
    if (codons > kCodonMaxCodons) throw std::runtime_error(path + ": " + std::to_string(codons) + " codons, at most " + std::to_string(kCodonMaxCodons) + " are counted");
    return out;
}

char translate(const char* t) {
    static const char* const kTable = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";   // NCBI table 1, letters in the order T C A G
    int at = 0;
    for (int i = 0; i < 3; i++) {
        const int v = t[i] == 'T' ? 0 : t[i] == 'C' ? 1 : t[i] == 'A' ? 2 : t[i] == 'G' ? 3 : -1;
        if (v < 0) return 'X';
        at = at * 4 + v;
    }
    return kTable[at];
}

uint64_t write_codons_tsv(const std::string& out_path, const Index& ix, int file, const std::vector<CodonGene>& genes, const std::vector<uint32_t>& counts,
                          const CodonParams& p) {
    const FileCells g(ix, file);
    size_t total = 0;
    for (const CodonGene& c : genes) total += c.reg.n_codons;
    if (counts.size() != total * 64) throw std::runtime_error("write_codons_tsv: the counters are not the regions'");
    FILE* fp = fopen(out_path.c_str(), "w");
    if (!fp) throw std::runtime_error("Failed to create codons output file " + out_path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    fprintf(fp, "##codon_max_mismatches=%u\n##codon_min_reads=%llu\n##codon_min_freq=%g\n", p.max_mismatches, (unsigned long long)p.min_reads, p.min_freq);
    fputs("chrom\tregion\tstrand\tcodon\tpos\tref_codon\tref_aa\talt_codon\talt_aa\tcount\tcover\tfreq\ttype\n", fp);
    uint64_t lines = 0;
    size_t base = 0;
    for (const CodonGene& c : genes) {
        const std::string chrom = chrom_of(ix.files[(size_t)file].sequences[c.seq].name);
        const bool minus = c.strand == '-';
        // a forward triplet's letters as the gene reads them
        auto letters = [&](uint32_t t, char* out) {
            const char f[3] = {"ACGT"[t >> 4], "ACGT"[(t >> 2) & 3], "ACGT"[t & 3]};
            for (int i = 0; i < 3; i++) out[i] = minus ? complement(f[2 - i]) : f[i];
            out[3] = 0;
        };
        for (uint32_t j = 1; j <= c.reg.n_codons; j++) {           // in the direction of translation
            const uint32_t d = minus ? c.reg.n_codons - j : j - 1;   // the device's codon of the region
            const uint32_t* cnt = counts.data() + (base + d) * 64;
            uint64_t cover = 0;
            for (int t = 0; t < 64; t++) cover += cnt[t];
            if (!cover) continue;
            const char* ref = g.text.data() + (size_t)(c.reg.cell0 - g.cell0) + 3 * (size_t)d;
            const uint32_t ref_t = 16u * nt_to_bits((uint8_t)ref[0]) + 4u * nt_to_bits((uint8_t)ref[1]) + nt_to_bits((uint8_t)ref[2]);
            char rc[4], ac[4];
            letters(ref_t, rc);
            const char ra = translate(rc);
            for (uint32_t t = 0; t < 64; t++) {
                const uint64_t n = cnt[t];
                if (t == ref_t || n < p.min_reads || !((double)n >= p.min_freq * (double)cover)) continue;
                letters(t, ac);
                const char aa = translate(ac);
                const char* type = aa == ra ? "synonymous" : aa == '*' ? "nonsense" : ra == '*' ? "stop_lost" : "missense";
                const uint64_t q = 10000ull * n / cover;
                fprintf(fp, "%s\t%s\t%c\t%u\t%llu\t%s\t%c\t%s\t%c\t%llu\t%llu\t%llu.%04llu\t%s\n", chrom.c_str(), c.name.c_str(), c.strand, j,
                        (unsigned long long)c.start + 3ull * d + 1, rc, ra, ac, aa, (unsigned long long)n, (unsigned long long)cover, (unsigned long long)(q / 10000),
                        (unsigned long long)(q % 10000), type);
                lines++;
            }
        }
        base += c.reg.n_codons;
    }
    if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write codons file " + out_path);
    return lines;
}

}  // namespace bronko
