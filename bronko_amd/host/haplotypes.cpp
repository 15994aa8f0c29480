// haplotypes.cpp -- the host twin of bk_haplotypes.hip, the --haplotypes regions and the .haplotypes.tsv writer (haplotypes.hpp).
#include "haplotypes.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <utility>

#include "file_cells.hpp"

namespace bronko {

namespace {

void check_regions(const FileCells& g, const std::vector<HapRegion>& regions) {
    if (regions.size() > kHapMaxRegions) throw std::runtime_error("hap_count: at most 4096 regions, got " + std::to_string(regions.size()));
    for (size_t i = 0; i < regions.size(); i++) {
        const HapRegion& r = regions[i];
        const std::string who = "hap_count: region " + std::to_string(i);
        if (r.len == 0) throw std::runtime_error(who + " has no cell");
        if (r.len > kHapMaxLen) throw std::runtime_error(who + " has " + std::to_string(r.len) + " cells, at most 65520");
        g.check_region(who, r.cell0, (uint64_t)r.cell0 + r.len);
    }
}

typedef std::vector<std::pair<uint32_t, uint8_t>> HapList;   // (offset, base): vectors compare as the order asks, a proper prefix first

HapList list_of(const HapEntry& e) {
    HapList l;
    for (int t = 0; t < e.n_mm; t++) l.emplace_back(mm_offset(e.mm, t), (uint8_t)mm_base(e.mm, t));
    return l;
}

}  // namespace

HapTable hap_count(const Index& ix, int file, const std::vector<LinkRow>& rows, const std::vector<HapRegion>& regions) {
    const FileCells g(ix, file);
    check_regions(g, regions);
    HapTable t;
    t.cover.assign(regions.size(), 0u); t.ref_count.assign(regions.size(), 0u);
    for (size_t i = 0; i < regions.size(); i++) {
        const uint64_t c0 = regions[i].cell0, c1 = c0 + regions[i].len;
        std::map<HapList, uint32_t> seen;
        for (const LinkRow& row : rows) {
            if (!(row.cell0 <= c0 && c1 <= (uint64_t)row.cell0 + row.n)) continue;
            t.cover[i]++;
            HapList l;
            for (int s = 0; s < row.n_mm; s++) {
                const uint64_t cell = (uint64_t)row.cell0 + mm_offset(row.mm, s);
                if (cell >= c0 && cell < c1) l.emplace_back((uint32_t)(cell - c0), (uint8_t)mm_base(row.mm, s));
            }
            if (l.empty()) t.ref_count[i]++; else seen[l]++;
        }
        for (const auto& kv : seen) {
            HapEntry e;
            e.region = (uint32_t)i; e.count = kv.second; e.n_mm = (uint8_t)kv.first.size();
            for (size_t s = 0; s < kv.first.size(); s++) {
                e.mm[3 * s] = (uint8_t)(kv.first[s].first & 0xffu); e.mm[3 * s + 1] = (uint8_t)(kv.first[s].first >> 8); e.mm[3 * s + 2] = kv.first[s].second;
            }
            t.entries.push_back(e);
        }
    }
    return t;
}

std::vector<BedLine> read_hap_bed(const std::string& path) {
    std::vector<BedLine> bed = read_bed(path);
    for (const BedLine& b : bed)
        if (b.end - b.start > kHapMaxLen)
            throw std::runtime_error(path + ": line " + std::to_string(b.line) + ": a haplotype region has at most " + std::to_string(kHapMaxLen) + " positions, " +
                                     std::to_string(b.start) + " to " + std::to_string(b.end) + " are " + std::to_string(b.end - b.start));
    if (bed.size() > kHapMaxRegions) throw std::runtime_error(path + ": " + std::to_string(bed.size()) + " haplotype regions, at most " + std::to_string(kHapMaxRegions) + " are counted");
    return bed;
}

std::vector<HapWindow> resolve_hap_bed(const Index& ix, int file, const std::vector<BedLine>& bed, const std::string& path) {
    const FileCells g(ix, file);
    std::vector<HapWindow> out;
    for (const BedLine& b : bed)
        for (const Region& r : resolve_bed(ix, std::vector<BedLine>{b}, path)) {   // (a chrom no file carries, an end beyond the sequence: its errors)
            if (r.file_id != file) continue;
            HapWindow w;
            w.reg.cell0 = (uint32_t)(g.cell0 + g.first[r.seq] + r.start); w.reg.len = r.end - r.start;
            w.seq = r.seq; w.start = r.start; w.name = r.name;
            out.push_back(std::move(w));
        }
    if (out.size() > kHapMaxRegions) throw std::runtime_error(path + ": " + std::to_string(out.size()) + " haplotype regions, at most " + std::to_string(kHapMaxRegions) + " are counted");
    return out;
}

std::vector<HapWindow> hap_windows(const Index& ix, int file, uint64_t window, uint64_t step) {
    if (window < 1 || window > kHapMaxLen) throw std::runtime_error("the haplotype window must be 1.." + std::to_string(kHapMaxLen) + ", got " + std::to_string(window));
    if (step < 1) throw std::runtime_error("the haplotype step must be at least 1");
    const FileCells g(ix, file);
    uint64_t n = 0;
    for (size_t q = 0; q + 1 < g.first.size(); q++) {
        const uint64_t len = g.first[q + 1] - g.first[q];
        if (len >= window) n += (len - window) / step + 1;
    }
    if (n > kHapMaxRegions)
        throw std::runtime_error("--hap-window " + std::to_string(window) + " with step " + std::to_string(step) + " makes " + std::to_string(n) + " windows, at most " +
                                 std::to_string(kHapMaxRegions) + " are counted: raise the step");
    std::vector<HapWindow> out;
    for (size_t q = 0; q + 1 < g.first.size(); q++) {
        const uint64_t len = g.first[q + 1] - g.first[q];
        for (uint64_t s = 0; s + window <= len; s += step) {
            HapWindow w;
            w.reg.cell0 = (uint32_t)(g.cell0 + g.first[q] + s); w.reg.len = (uint32_t)window;
            w.seq = (uint32_t)q; w.start = (uint32_t)s; w.name = ".";
            out.push_back(std::move(w));
        }
    }
    return out;
}

HapStats write_haplotypes_tsv(const std::string& out_path, const Index& ix, int file, const std::vector<HapWindow>& windows, const HapTable& t, const HapParams& p) {
    const FileCells g(ix, file);
    if (t.cover.size() != windows.size() || t.ref_count.size() != windows.size()) throw std::runtime_error("write_haplotypes_tsv: the counters are not the regions'");
    std::vector<std::vector<std::pair<HapList, uint64_t>>> by(windows.size());
    for (const HapEntry& e : t.entries) {
        if (e.region >= windows.size() || e.n_mm < 1 || e.n_mm > 8) throw std::runtime_error("write_haplotypes_tsv: an entry is not the regions'");
        by[e.region].emplace_back(list_of(e), e.count);
    }
    FILE* fp = fopen(out_path.c_str(), "w");
    if (!fp) throw std::runtime_error("Failed to create haplotypes output file " + out_path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    fprintf(fp, "##hap_max_mismatches=%u\n##hap_min_reads=%llu\n##hap_min_freq=%g\n", p.max_mismatches, (unsigned long long)p.min_reads, p.min_freq);
    fputs("chrom\tstart\tend\tname\tcover\thaplotypes\trank\tcount\tfreq\tn_sub\tsubstitutions\n", fp);
    HapStats st;
    for (size_t i = 0; i < windows.size(); i++) {
        const HapWindow& w = windows[i];
        const uint64_t cover = t.cover[i];
        std::vector<std::pair<HapList, uint64_t>>& haps = by[i];
        if (t.ref_count[i]) haps.emplace_back(HapList(), t.ref_count[i]);
        st.distinct += haps.size();
        if (!cover) { st.no_cover++; continue; }
        std::sort(haps.begin(), haps.end(), [](const std::pair<HapList, uint64_t>& x, const std::pair<HapList, uint64_t>& y) {
            return x.second != y.second ? x.second > y.second : x.first < y.first;
        });
        const std::string chrom = chrom_of(ix.files[(size_t)file].sequences[w.seq].name);
        for (size_t r = 0; r < haps.size(); r++) {
            const uint64_t n = haps[r].second;
            if (n < p.min_reads || !((double)n >= p.min_freq * (double)cover)) continue;
            std::string subs;
            for (const auto& ob : haps[r].first) {
                if (!subs.empty()) subs += ',';
                subs += std::to_string((uint64_t)w.start + ob.first + 1);
                subs += g.text[(size_t)(w.reg.cell0 - g.cell0) + ob.first];
                subs += '>';
                subs += "ACGT"[ob.second & 3];
            }
            const uint64_t q = 10000ull * n / cover;
            fprintf(fp, "%s\t%u\t%u\t%s\t%llu\t%llu\t%llu\t%llu\t%llu.%04llu\t%llu\t%s\n", chrom.c_str(), w.start, w.start + w.reg.len, w.name.c_str(),
                    (unsigned long long)cover, (unsigned long long)haps.size(), (unsigned long long)(r + 1), (unsigned long long)n, (unsigned long long)(q / 10000),
                    (unsigned long long)(q % 10000), (unsigned long long)haps[r].first.size(), subs.empty() ? "." : subs.c_str());
            st.lines++;
        }
    }
    if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write haplotypes file " + out_path);
    return st;
}

}  // namespace bronko
