// breakends.cpp -- the host twin of bk_breakends.hip and the .breakends.tsv writer (breakends.hpp).
#include "breakends.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <tuple>

#include "../../include/bronko_hip.h"
#include "anchor_genome.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

struct Tables {
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (cell, side, tag) -> fwd, rev
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> site;                                     // (cell, side) -> supporting records
    std::vector<int64_t> span;                       // difference array over the file's cells (+ 2)
    BreakendCounters n;
};

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

std::string along_reference(const std::string& rec, bool against) {
    if (!against) return rec;
    std::string r(rec.size(), 'A');
    for (size_t j = 0; j < rec.size(); j++) r[j] = comp(rec[rec.size() - 1 - j]);
    return r;
}

// both ends anchored: what the span needs, as junctions.cpp has it
void two_anchors(const AnchorGenome& g, const std::string& rec, int f_off, uint32_t f_cell, bool f_ag, int b_off, uint32_t b_cell, bool b_ag, int M, Tables& t) {
    const int k = g.k, n = (int)rec.size();
    if (f_ag != b_ag) return;
    const std::string r = along_reference(rec, f_ag);
    int64_t a, b, ca, cb;
    if (f_ag) { a = n - k - b_off; ca = b_cell; b = n - k - f_off; cb = f_cell; }
    else { a = f_off; ca = f_cell; b = b_off; cb = b_cell; }
    if (a + k > b) return;
    const size_t s = (size_t)g.seq_of(ca);
    if ((size_t)g.seq_of(cb) != s) return;
    const int64_t dL = ca - a, dR = cb - b;
    const int64_t lo = std::min(dL, dR), hi = std::max(dL, dR) + n;
    if (lo < g.first[s] || hi > g.first[s + 1]) return;
    for (int64_t c = lo; c < hi; c++) if (!is_acgt(g.text[(size_t)c])) return;
    if (dL != dR) return;
    int m = 0;
    for (int64_t j = 0; j < n; j++) m += r[(size_t)j] != g.text[(size_t)(dL + j)] ? 1 : 0;
    if (m > M) return;
    t.n.ref_spanning++;
    t.span[(size_t)(dL + a + k)] += 1; t.span[(size_t)(dL + b + 1)] -= 1;
}

void one_anchor(const AnchorGenome& g, const std::string& rec, bool front, int off, uint32_t cell, bool against, int C, int M, Tables& t) {
    const int64_t k = g.k, n = (int64_t)rec.size();
    t.n.one_anchor++;
    const std::string r = along_reference(rec, against);
    const int64_t a = against ? n - k - off : off, c = cell, d = c - a;
    const bool left = front != against;              // side L
    const size_t s = (size_t)g.seq_of(c);
    // the stretch of ACGT letters of s around c (a cell that holds another letter: empty)
    int64_t lo = c, hi = c;
    while (hi < g.first[s + 1] && is_acgt(g.text[(size_t)hi])) hi++;
    while (lo > g.first[s] && is_acgt(g.text[(size_t)(lo - 1)])) lo--;
    if (c + k > hi || (left ? d < lo : d + n > hi)) { t.n.unplaced++; return; }
    auto score = [&](int64_t j) { return r[(size_t)j] == g.text[(size_t)(d + j)] ? 1 : -BK_BREAKEND_MISMATCH_PENALTY; };
    int64_t edge, S = 0, best = 0, m = 0;
    if (left) {
        const int64_t P = std::min(n, hi - d);
        edge = a + k;
        for (int64_t p = a + k; p < P; p++) { S += score(p); if (S > best) { best = S; edge = p + 1; } }
        for (int64_t j = 0; j < edge; j++) m += r[(size_t)j] != g.text[(size_t)(d + j)] ? 1 : 0;
    } else {
        const int64_t Q = std::max<int64_t>(0, lo - d);
        edge = a;
        for (int64_t q = a - 1; q >= Q; q--) { S += score(q); if (S > best) { best = S; edge = q; } }
        for (int64_t j = edge; j < n; j++) m += r[(size_t)j] != g.text[(size_t)(d + j)] ? 1 : 0;
    }
    if (m > M) { t.n.discordant++; return; }
    const int64_t clip = left ? n - edge : edge;
    if (clip == 0) { t.n.through++; return; }
    if (clip < C) { t.n.short_++; return; }
    t.n.supporting++;
    const int64_t at = left ? edge : edge - 16;
    uint32_t tag = 0;
    for (int i = 0; i < 16; i++) tag |= (uint32_t)code_of(r[(size_t)(at + i)]) << (2 * i);
    const uint32_t ev_cell = (uint32_t)(g.cell0 + (left ? d + edge - 1 : d + edge)), side = left ? 0u : 1u;
    auto& e = t.events[std::make_tuple(ev_cell, side, tag)];
    (against ? e.second : e.first)++;
    t.site[std::make_pair(ev_cell, side)]++;
}

void add_record(const AnchorGenome& g, const std::string& rec, int C, int M, Tables& t) {
    const int k = g.k, n = (int)rec.size();
    t.n.records++;
    if (n < 2 * k) return;
    int f = -1, b = -1;
    uint32_t cf = 0, cb = 0;
    bool f_ag = false, b_ag = false;
    for (int o = 0; o <= 24 && o + k <= n; o += 8)
        if (g.anchor(rec.data() + o, &cf, &f_ag)) { f = o; break; }
    for (int o = n - k; o >= n - k - 24 && o >= 0; o -= 8)
        if (g.anchor(rec.data() + o, &cb, &b_ag)) { b = o; break; }
    if (f < 0 && b < 0) return;
    if (f >= 0 && b >= 0) { two_anchors(g, rec, f, cf, f_ag, b, cb, b_ag, M, t); return; }
    if (f >= 0) one_anchor(g, rec, true, f, cf, f_ag, C, M, t);
    else one_anchor(g, rec, false, b, cb, b_ag, C, M, t);
}

std::string tag_letters(uint32_t tag) {
    std::string s(16, 'A');
    for (int i = 0; i < 16; i++) s[(size_t)i] = "ACGT"[(tag >> (2 * i)) & 3u];
    return s;
}

}  // namespace

BreakendResult breakend_events(const Index& ix, int file, const std::vector<std::string>& reads, int min_clip, int max_mismatches) {
    if (max_mismatches < 0 || max_mismatches > kBreakendMaxMismatches) throw std::runtime_error("breakend_events: max_mismatches must be 0..8");
    if (min_clip < kBreakendMinClipLo || min_clip > kBreakendMinClipHi) throw std::runtime_error("breakend_events: min_clip must be 16..65519");
    const AnchorGenome g(ix, file);
    Tables t;
    t.span.assign(g.text.size() + 2, 0);
    std::string run;
    for (const std::string& read : reads) {
        run.clear();
        for (size_t i = 0; i <= read.size(); i++) {
            const char c = i < read.size() ? (char)(read[i] >= 'a' && read[i] <= 'z' ? read[i] - 32 : read[i]) : 'N';
            if (is_acgt(c)) { run.push_back(c); continue; }
            if ((int)run.size() >= g.k) add_record(g, run, min_clip, max_mismatches, t);
            run.clear();
        }
    }
    BreakendResult out;
    out.n = t.n;
    out.span.assign((size_t)ix.total_cells(), 0u);
    int64_t acc = 0;
    std::vector<uint32_t> sums(g.text.size() + 1);
    for (size_t c = 0; c <= g.text.size(); c++) {
        acc += t.span[c]; sums[c] = (uint32_t)acc;
        if (c < g.text.size()) out.span[(size_t)g.cell0 + c] = (uint32_t)acc;
    }
    for (const auto& kv : t.events) {               // (the map's order is (cell, side, tag))
        BreakendEvent e;
        std::tie(e.cell, e.side, e.tag) = kv.first;
        e.fwd = kv.second.first; e.rev = kv.second.second;
        e.site_reads = t.site[std::make_pair(e.cell, e.side)];
        e.span = sums[(size_t)(e.cell - g.cell0) + (e.side ? 0 : 1)];
        out.events.push_back(e);
    }
    return out;
}

void write_breakends_tsv(const std::string& out_path, const Index& ix, int file, std::vector<BreakendEvent> events, const BreakendParams& p,
                         const BreakendTallies& t) {
    const FileCells g(ix, file);
    FILE* fp = fopen(out_path.c_str(), "w");
    if (!fp) throw std::runtime_error("Failed to create breakends output file " + out_path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    fprintf(fp, "##breakend_min_clip=%u\n##breakend_max_mismatches=%u\n##breakend_min_reads=%llu\n", p.min_clip, p.max_mismatches, (unsigned long long)p.min_reads);
    fprintf(fp, "##breakend_tallies=records:%llu,one_anchor:%llu,ref_spanning:%llu,supporting:%llu,short:%llu,through:%llu,discordant:%llu,unplaced:%llu,candidates:%llu,reported:%llu\n",
            (unsigned long long)t.records, (unsigned long long)t.one_anchor, (unsigned long long)t.ref_spanning, (unsigned long long)t.supporting,
            (unsigned long long)t.short_, (unsigned long long)t.through, (unsigned long long)t.discordant, (unsigned long long)t.unplaced,
            (unsigned long long)t.candidates, (unsigned long long)t.reported);
    fputs("chrom\tpos\tside\tfwd\trev\treads\tsite_reads\tspan\tfreq\tterminus\ttag\n", fp);
    std::sort(events.begin(), events.end(), [](const BreakendEvent& x, const BreakendEvent& y) {
        return std::make_tuple(x.cell, x.side, tag_letters(x.tag)) < std::make_tuple(y.cell, y.side, tag_letters(y.tag));
    });
    const FileMeta& fm = ix.files[(size_t)file];
    for (const BreakendEvent& e : events) {
        const int64_t c = (int64_t)e.cell - g.cell0;
        if (c < 0 || c >= (int64_t)g.text.size() || e.side > 1 || !is_acgt(g.text[(size_t)c])) throw std::runtime_error("write_breakends_tsv: an event outside the genome file's sequences");
        size_t s = 0;
        while (s + 2 < g.first.size() && g.first[s + 1] <= c) s++;
        const bool terminus = e.side ? c == g.first[s] : c == g.first[s + 1] - 1;
        const uint64_t reads = (uint64_t)e.fwd + e.rev;
        const uint64_t f = 10000ull * reads / std::max<uint64_t>(1, reads + e.span);
        fprintf(fp, "%s\t%lld\t%c\t%u\t%u\t%llu\t%u\t%u\t%llu.%04llu\t%d\t%s\n", chrom_of(fm.sequences[s].name).c_str(), (long long)(c - g.first[s] + 1), e.side ? 'R' : 'L',
                e.fwd, e.rev, (unsigned long long)reads, e.site_reads, e.span, (unsigned long long)(f / 10000), (unsigned long long)(f % 10000), terminus ? 1 : 0,
                tag_letters(e.tag).c_str());
    }
    if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write breakends file " + out_path);
}

}  // namespace bronko
