// duplications.cpp -- the host twin of bk_duplications.hip and the .duplications.tsv writer (duplications.hpp).
#include "duplications.hpp"

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
    std::map<std::pair<uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (cell, E) -> fwd, rev
    SpanCount span;
    DuplicationCounters n;
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
    const int64_t lo = g.first[(size_t)s], hi = g.first[(size_t)s + 1];
    const std::string& ref = g.text;
    auto acgt = [&](int64_t c0, int64_t c1) { for (int64_t c = c0; c < c1; c++) if (!is_acgt(ref[(size_t)c])) return false; return true; };
    auto mm = [&](int64_t j, int64_t d) { return r[(size_t)j] != ref[(size_t)(d + j)] ? 1 : 0; };
    if (delta > 0) { t.n.forward++; return; }
    if (-delta < L) { t.n.short_++; return; }
    const int64_t E = -delta;
    if (dL < lo || dR + n > hi) return;
    const int64_t p0 = std::max<int64_t>(a + k, lo - dR), p1 = std::min<int64_t>(b, hi - dL);   // the breakpoint's range, clipped to the sequence
    if (p0 > p1) return;
    if (!acgt(dL, dL + p1) || !acgt(dR + p0, dR + n)) return;   // the two arms; what overhangs the sequence is never read
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
    int64_t FL = pos - 1, FR = pos - E;              // first cells of the stretches of ACGT letters of the sequence that hold pos - 1 and pos - E
    while (FL - 1 >= lo && is_acgt(ref[(size_t)(FL - 1)])) FL--;
    while (FR - 1 >= lo && is_acgt(ref[(size_t)(FR - 1)])) FR--;
    while (pos - 1 > FL && pos - E - 1 >= FR && ref[(size_t)(pos - 1)] == ref[(size_t)(pos - E - 1)]) pos--;
    t.n.supporting++;
    auto& e = t.events[std::make_pair((uint32_t)(g.cell0 + pos), (uint32_t)E)];
    (o.against ? e.second : e.first)++;
}

}  // namespace

DuplicationResult duplication_events(const Index& ix, int file, const std::vector<std::string>& reads, uint32_t min_len, int max_mismatches) {
    if (min_len < 1 || min_len > kDuplicationMaxLen) throw std::runtime_error("duplication_events: min_len must be 1..2^27 - 1");
    if (max_mismatches < 0 || max_mismatches > kDuplicationMaxMismatches) throw std::runtime_error("duplication_events: max_mismatches must be 0..8");
    const AnchorGenome g(ix, file);
    Tables t(g);
    for_each_record(reads, g.k, [&](const std::string& rec) { add_record(g, rec, (int64_t)min_len, max_mismatches, t); });
    DuplicationResult out;
    out.n = t.n;
    const std::vector<uint32_t> sums = t.span.sums(ix, g, &out.span);
    for (const auto& kv : t.events) {               // (the map's order is (cell, len))
        DuplicationEvent e;
        e.cell = kv.first.first; e.len = kv.first.second;
        e.fwd = kv.second.first; e.rev = kv.second.second;
        e.span_start = sums[(size_t)(e.cell - g.cell0) - e.len]; e.span_end = sums[(size_t)(e.cell - g.cell0)];
        out.events.push_back(e);
    }
    return out;
}

void write_duplications_tsv(const std::string& out_path, const Index& ix, int file, std::vector<DuplicationEvent> events, const DuplicationParams& p) {
    const FileCells g(ix, file);
    const OutFile fp("duplications", out_path);
    fprintf(fp, "##duplication_min_len=%u\n##duplication_max_mismatches=%u\n##duplication_min_reads=%llu\n", p.min_len, p.max_mismatches, (unsigned long long)p.min_reads);
    fputs("chrom\tstart\tend\tlength\tfwd\trev\treads\tspan_start\tspan_end\tfreq\thomology\twhole\n", fp);
    // by sequence, start, end: start = cell - len ascends with the sequence, end with the cell
    std::sort(events.begin(), events.end(), [](const DuplicationEvent& x, const DuplicationEvent& y) {
        return std::make_tuple(x.cell - x.len, x.cell) < std::make_tuple(y.cell - y.len, y.cell);
    });
    const FileMeta& fm = ix.files[(size_t)file];
    for (const DuplicationEvent& e : events) {
        const int64_t pos = (int64_t)e.cell - g.cell0, E = e.len;
        const size_t s = (size_t)g.seq_of(pos - E);  // the sequence of the first duplicated cell (pos itself may be the next one's first)
        const int64_t lo = g.first[s], hi = g.first[s + 1];
        if (E < 1 || pos - E < lo || pos > hi) throw std::runtime_error("write_duplications_tsv: an event outside the genome file's sequences");
        int64_t h = 0;                               // how far the event could slide to the right
        while (h < E && pos + h < hi && is_acgt(g.text[(size_t)(pos + h)]) && is_acgt(g.text[(size_t)(pos - E + h)]) &&
               g.text[(size_t)(pos + h)] == g.text[(size_t)(pos - E + h)]) h++;
        const uint64_t reads = (uint64_t)e.fwd + e.rev;
        fprintf(fp, "%s\t%lld\t%lld\t%u\t%u\t%u\t%llu\t%u\t%u\t%s\t%lld\t%d\n", chrom_of(fm.sequences[s].name).c_str(), (long long)(pos - E - lo + 1),
                (long long)(pos - lo), e.len, e.fwd, e.rev, (unsigned long long)reads, e.span_start, e.span_end,
                freq_text(reads, std::max(e.span_start, e.span_end)).c_str(), (long long)h, E == hi - lo ? 1 : 0);
    }
    fp.finish();
}

}  // namespace bronko
