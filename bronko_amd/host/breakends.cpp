// breakends.cpp -- the host twin of bk_breakends.hip and the .breakends.tsv writer (breakends.hpp).
#include "breakends.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <tuple>

#include "../../include/bronko_hip.h"
#include "event_twin.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

struct Tables {
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (cell, side, tag) -> fwd, rev
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> site;                                     // (cell, side) -> supporting records
    SpanCount span;
    BreakendCounters n;
    explicit Tables(const FileCells& g) : span(g) {}
};

int code_of(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : 3; }

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
    const EndAnchors ends = end_anchors(g, rec);
    const int f = ends.f_off, b = ends.b_off;
    const uint32_t cf = ends.f_cell, cb = ends.b_cell;
    const bool f_ag = ends.f_ag, b_ag = ends.b_ag;
    if (f < 0 && b < 0) return;
    if (ends.both()) {                               // both ends anchored: on one strand, what the span needs
        if (f_ag != b_ag) return;
        const Oriented o = orient(rec, k, ends);
        if (o.a + k <= o.b && t.span.place(g, o, M) == Placed::spanning) t.n.ref_spanning++;
        return;
    }
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
    Tables t(g);
    for_each_record(reads, g.k, [&](const std::string& rec) { add_record(g, rec, min_clip, max_mismatches, t); });
    BreakendResult out;
    out.n = t.n;
    const std::vector<uint32_t> sums = t.span.sums(ix, g, &out.span);
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
    const OutFile fp("breakends", out_path);
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
        const size_t s = (size_t)g.seq_of(c);
        const bool terminus = e.side ? c == g.first[s] : c == g.first[s + 1] - 1;
        const uint64_t reads = (uint64_t)e.fwd + e.rev;
        fprintf(fp, "%s\t%lld\t%c\t%u\t%u\t%llu\t%u\t%u\t%s\t%d\t%s\n", chrom_of(fm.sequences[s].name).c_str(), (long long)(c - g.first[s] + 1), e.side ? 'R' : 'L',
                e.fwd, e.rev, (unsigned long long)reads, e.site_reads, e.span, freq_text(reads, e.span).c_str(), terminus ? 1 : 0, tag_letters(e.tag).c_str());
    }
    fp.finish();
}

}  // namespace bronko
