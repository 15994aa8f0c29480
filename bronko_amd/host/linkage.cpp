// linkage.cpp -- the host twin of bk_linkage.hip and the .linkage.tsv writer (linkage.hpp).
#include "linkage.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <tuple>

#include "anchor_genome.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

void place_record(const AnchorGenome& g, const std::string& rec, int M, LinkResult& out) {
    const int k = g.k, n = (int)rec.size();
    out.n.records++;
    if (n < 2 * k || n > 65535) { out.n.unplaced++; return; }
    const EndAnchors ends = end_anchors(g, rec);
    if (!ends.both() || ends.f_ag != ends.b_ag) { out.n.unplaced++; return; }
    const Oriented o = orient(rec, k, ends);
    const bool against = o.against;
    const std::string& r = o.r;
    const int64_t a = o.a, b = o.b, ca = o.ca, cb = o.cb;
    const int64_t dL = ca - a, dR = cb - b;
    const int s = g.seq_of(ca);
    bool ok = a + k <= b && dL == dR && g.seq_of(cb) == s && dL >= g.first[(size_t)s] && dL + n <= g.first[(size_t)s + 1];
    for (int64_t c = dL; ok && c < dL + n; c++) ok = is_acgt(g.text[(size_t)c]);
    if (!ok) { out.n.unplaced++; return; }
    LinkRow row;
    int m = 0;
    for (int j = 0; j < n; j++) {
        if (r[(size_t)j] == g.text[(size_t)(dL + j)]) continue;
        if (m < kLinkMaxMismatches) { row.mm[3 * m] = (uint8_t)(j & 255); row.mm[3 * m + 1] = (uint8_t)(j >> 8); row.mm[3 * m + 2] = nt_to_bits((uint8_t)r[(size_t)j]); }
        m++;
    }
    if (m > M) { out.n.discordant++; return; }
    row.cell0 = (uint32_t)(g.cell0 + dL); row.n = (uint16_t)n; row.strand = against ? 1 : 0; row.n_mm = (uint8_t)m;
    out.n.placed++;
    out.rows.push_back(row);
}

}  // namespace

LinkResult link_rows(const Index& ix, int file, const std::vector<std::string>& reads, int max_mismatches) {
    if (max_mismatches < 0 || max_mismatches > kLinkMaxMismatches) throw std::runtime_error("link_rows: max_mismatches must be 0..8");
    const AnchorGenome g(ix, file);
    LinkResult out;
    for_each_record(reads, g.k, [&](const std::string& rec) { place_record(g, rec, max_mismatches, out); });
    return out;
}

std::vector<LinkPair> link_count(const Index& ix, int file, const std::vector<LinkRow>& rows, const std::vector<uint32_t>& sites, uint32_t max_dist) {
    if (sites.size() > kLinkMaxSites) throw std::runtime_error("link_count: at most 65536 sites, got " + std::to_string(sites.size()));
    if (max_dist < 1 || max_dist > kLinkMaxDist) throw std::runtime_error("link_count: max_dist must be 1..65519");
    for (size_t i = 1; i < sites.size(); i++)
        if (sites[i] <= sites[i - 1]) throw std::runtime_error("link_count: the sites must be strictly ascending");
    const AnchorGenome g(ix, file);
    std::vector<LinkPair> pairs;
    std::vector<size_t> pair_lo(sites.size());
    for (size_t i = 0; i < sites.size(); i++) {
        pair_lo[i] = pairs.size();
        if ((int64_t)sites[i] < g.cell0 || (int64_t)sites[i] >= g.cell0 + (int64_t)g.text.size()) throw std::runtime_error("link_count: a site outside the genome file");
        const int s = g.seq_of((int64_t)sites[i] - g.cell0);
        for (size_t j = i + 1; j < sites.size() && (int64_t)sites[j] - g.cell0 < g.first[(size_t)s + 1] && sites[j] - sites[i] <= max_dist; j++) {
            if (pairs.size() >= kLinkMaxPairs) throw std::runtime_error("link_count: more than 1048576 pairs of sites");
            LinkPair p;
            p.site_a = sites[i]; p.site_b = sites[j];
            pairs.push_back(p);
        }
    }
    for (const LinkRow& row : rows) {
        auto base_at = [&](uint32_t cell) { return row_base(row, cell, nt_to_bits((uint8_t)g.text[(size_t)((int64_t)cell - g.cell0)])); };
        const size_t s0 = (size_t)(std::lower_bound(sites.begin(), sites.end(), row.cell0) - sites.begin());
        const uint32_t end = row.cell0 + row.n;
        for (size_t i = s0; i < sites.size() && sites[i] < end; i++)
            for (size_t j = i + 1; j < sites.size() && sites[j] < end && sites[j] - sites[i] <= max_dist; j++)
                pairs[pair_lo[i] + (j - i - 1)].count[4 * base_at(sites[i]) + base_at(sites[j])]++;
    }
    return pairs;
}

std::vector<uint32_t> link_sites(const std::vector<LinkSite>& recs) {
    std::vector<uint32_t> sites;
    for (const LinkSite& r : recs) sites.push_back(r.cell);
    std::sort(sites.begin(), sites.end());
    sites.erase(std::unique(sites.begin(), sites.end()), sites.end());
    return sites;
}

uint64_t write_linkage_tsv(const std::string& out_path, const Index& ix, int file, std::vector<LinkSite> recs, const std::vector<LinkPair>& pairs,
                           const LinkParams& p) {
    if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("write_linkage_tsv: no such genome file");
    FILE* fp = fopen(out_path.c_str(), "w");
    if (!fp) throw std::runtime_error("Failed to create linkage output file " + out_path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    fprintf(fp, "##link_max_mismatches=%u\n##link_max_dist=%u\n##link_min_reads=%llu\n", p.max_mismatches, p.max_dist, (unsigned long long)p.min_reads);
    fputs("chrom\tpos_a\tref_a\talt_a\tpos_b\tref_b\talt_b\tcover\tref_ref\tref_alt\talt_ref\talt_alt\tother\n", fp);
    const FileMeta& fm = ix.files[(size_t)file];
    uint64_t cell0 = 0;
    for (int f = 0; f < file; f++) cell0 += ix.genome_len((size_t)f);
    std::sort(recs.begin(), recs.end(), [](const LinkSite& x, const LinkSite& y) { return std::tie(x.cell, x.alt_base) < std::tie(y.cell, y.alt_base); });
    std::map<std::pair<uint32_t, uint32_t>, const LinkPair*> by_cells;
    for (const LinkPair& q : pairs) by_cells[{q.site_a, q.site_b}] = &q;
    uint64_t lines = 0;
    for (size_t x = 0; x < recs.size(); x++) {
        const LinkSite& A = recs[x];
        uint64_t at = cell0;                          // the sequence that holds A (B's pair is in the same one)
        const SeqMeta* sm = nullptr;
        for (const auto& s : fm.sequences) { if (A.cell >= at && A.cell < at + s.len) { sm = &s; break; } at += s.len; }
        if (!sm) throw std::runtime_error("write_linkage_tsv: a record outside the genome file's sequences");
        for (size_t y = x + 1; y < recs.size(); y++) {
            const LinkSite& B = recs[y];
            if (B.cell == A.cell) continue;
            const auto it = by_cells.find({A.cell, B.cell});
            if (it == by_cells.end()) continue;
            const uint32_t* c = it->second->count;
            uint64_t cover = 0;
            for (int t = 0; t < 16; t++) cover += c[t];
            if (cover < p.min_reads) continue;
            const uint64_t rr = c[4 * A.ref_base + B.ref_base], ra = c[4 * A.ref_base + B.alt_base], ar = c[4 * A.alt_base + B.ref_base],
                           aa = c[4 * A.alt_base + B.alt_base];
            fprintf(fp, "%s\t%llu\t%c\t%c\t%llu\t%c\t%c\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", chrom_of(sm->name).c_str(), (unsigned long long)(A.cell - at + 1),
                    "ACGT"[A.ref_base & 3], "ACGT"[A.alt_base & 3], (unsigned long long)(B.cell - at + 1), "ACGT"[B.ref_base & 3], "ACGT"[B.alt_base & 3],
                    (unsigned long long)cover, (unsigned long long)rr, (unsigned long long)ra, (unsigned long long)ar, (unsigned long long)aa,
                    (unsigned long long)(cover - rr - ra - ar - aa));
            lines++;
        }
    }
    if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write linkage file " + out_path);
    return lines;
}

}  // namespace bronko
