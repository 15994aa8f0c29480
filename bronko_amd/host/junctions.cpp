// junctions.cpp -- the host twin of bk_junctions.hip and the .junctions.tsv writer (junctions.hpp).
#include "junctions.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <tuple>

#include "event_twin.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

struct Tables {
    std::map<std::pair<uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (cell, D) -> fwd, rev
    SpanCount span;
    JunctionCounters n;
    explicit Tables(const FileCells& g) : span(g) {}
};

void add_record(const AnchorGenome& g, const std::string& rec, int64_t L, int M, Tables& t) {
    const int k = g.k, n = (int)rec.size();
    t.n.records++;
    if (n < 2 * k) return;
    const EndAnchors ends = end_anchors(g, rec);
    if (!ends.both() || ends.f_ag != ends.b_ag) return;
    const Oriented o = orient(rec, k, ends);
    const std::string& r = o.r;
    const int64_t a = o.a, b = o.b;
    if (a + k > b) return;
    t.n.anchored++;
    switch (t.span.place(g, o, M)) {
        case Placed::outside: return;
        case Placed::discordant: t.n.discordant++; return;
        case Placed::spanning: t.n.ref_spanning++; return;
        case Placed::shifted: break;
    }
    const int64_t dL = o.ca - a, dR = o.cb - b, delta = dR - dL;
    const int s = g.seq_of(o.ca);
    if (!g.holds_acgt((size_t)s, std::min(dL, dR), std::max(dL, dR) + n)) return;
    const std::string& ref = g.text;
    auto mm = [&](int64_t j, int64_t d) { return r[(size_t)j] != ref[(size_t)(d + j)] ? 1 : 0; };
    if (delta < L && -delta < L) { t.n.short_++; return; }
    if (delta < 0) { t.n.backward++; return; }
    const int64_t D = delta, p0 = a + k, p1 = b;     // the breakpoint's range
    // m(p0), then one comparison exchanged per step
    int64_t m = 0;
    for (int64_t j = 0; j < p0; j++) m += mm(j, dL);
    for (int64_t j = p0; j < n; j++) m += mm(j, dR);
    int64_t best = m, best_p = p0;
    for (int64_t p = p0; p < p1; p++) {
        m += mm(p, dL) - mm(p, dR);
        if (m < best) { best = m; best_p = p + 1; }
    }
    if (best > M) { t.n.discordant++; return; }
    int64_t pos = dL + best_p;
    int64_t F = pos - 1;                             // first cell of the stretch of ACGT letters of the sequence that holds pos - 1
    while (F - 1 >= g.first[(size_t)s] && is_acgt(ref[(size_t)(F - 1)])) F--;
    while (pos - 1 > F && ref[(size_t)(pos - 1)] == ref[(size_t)(pos + D - 1)]) pos--;
    t.n.supporting++;
    auto& e = t.events[std::make_pair((uint32_t)(g.cell0 + pos), (uint32_t)D)];
    (o.against ? e.second : e.first)++;
}

}  // namespace

JunctionResult junction_events(const Index& ix, int file, const std::vector<std::string>& reads, uint32_t min_len, int max_mismatches) {
    if (min_len < 1 || min_len > kJunctionMaxLen) throw std::runtime_error("junction_events: min_len must be 1..2^27 - 1");
    if (max_mismatches < 0 || max_mismatches > kJunctionMaxMismatches) throw std::runtime_error("junction_events: max_mismatches must be 0..8");
    const AnchorGenome g(ix, file);
    Tables t(g);
    for_each_record(reads, g.k, [&](const std::string& rec) { add_record(g, rec, (int64_t)min_len, max_mismatches, t); });
    JunctionResult out;
    out.n = t.n;
    const std::vector<uint32_t> sums = t.span.sums(ix, g, &out.span);
    for (const auto& kv : t.events) {               // (the map's order is (cell, len))
        JunctionEvent e;
        e.cell = kv.first.first; e.len = kv.first.second;
        e.fwd = kv.second.first; e.rev = kv.second.second;
        e.span_donor = sums[(size_t)(e.cell - g.cell0)]; e.span_acceptor = sums[(size_t)(e.cell - g.cell0) + e.len];
        out.events.push_back(e);
    }
    return out;
}

void write_junctions_tsv(const std::string& out_path, const Index& ix, int file, std::vector<JunctionEvent> events, const JunctionParams& p) {
    const FileCells g(ix, file);
    const OutFile fp("junctions", out_path);
    fprintf(fp, "##junction_min_len=%u\n##junction_max_mismatches=%u\n##junction_min_reads=%llu\n", p.min_len, p.max_mismatches, (unsigned long long)p.min_reads);
    fputs("chrom\tdonor\tacceptor\tlength\tfwd\trev\treads\tspan_donor\tspan_acceptor\tfreq\thomology\n", fp);
    std::sort(events.begin(), events.end(), [](const JunctionEvent& x, const JunctionEvent& y) { return std::tie(x.cell, x.len) < std::tie(y.cell, y.len); });
    const FileMeta& fm = ix.files[(size_t)file];
    for (const JunctionEvent& e : events) {
        const int64_t pos = (int64_t)e.cell - g.cell0, D = e.len;
        const size_t s = (size_t)g.seq_of(pos);
        if (pos <= g.first[s] || pos + D >= g.first[s + 1]) throw std::runtime_error("write_junctions_tsv: an event outside the genome file's sequences");
        int64_t h = 0;                               // how far the junction could slide to the right
        while (h < D && pos + D + h < g.first[s + 1] && is_acgt(g.text[(size_t)(pos + h)]) && g.text[(size_t)(pos + h)] == g.text[(size_t)(pos + D + h)]) h++;
        const uint64_t reads = (uint64_t)e.fwd + e.rev, donor = (uint64_t)(pos - g.first[s]);
        fprintf(fp, "%s\t%llu\t%llu\t%u\t%u\t%u\t%llu\t%u\t%u\t%s\t%lld\n", chrom_of(fm.sequences[s].name).c_str(), (unsigned long long)donor,
                (unsigned long long)(donor + (uint64_t)D + 1), e.len, e.fwd, e.rev, (unsigned long long)reads, e.span_donor, e.span_acceptor,
                freq_text(reads, e.span_donor).c_str(), (long long)h);
    }
    fp.finish();
}

}  // namespace bronko
