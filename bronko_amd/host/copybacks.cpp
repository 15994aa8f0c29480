// copybacks.cpp -- the host twin of bk_copybacks.hip and the .copybacks.tsv writer (copybacks.hpp).
#include "copybacks.hpp"

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
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (lo, hi, kind) -> lo_first, hi_first
    SpanCount span;
    CopybackCounters n;
    explicit Tables(const FileCells& g) : span(g) {}
};

// the pairs (x + t, y - t), t0 <= t <= t1, that the reference cannot tell from (x, y): both cells of each inside sequence s and ACGT
void slide_run(const FileCells& g, size_t s, int kind, int64_t x, int64_t y, int64_t* t0, int64_t* t1) {
    const std::string& ref = g.text;
    auto ok = [&](int64_t c) { return c >= g.first[s] && c < g.first[s + 1] && is_acgt(ref[(size_t)c]); };
    auto up = [&](int64_t u, int64_t v) {            // from the pair (u, v) to (u + 1, v - 1)
        if (!ok(u + 1) || !ok(v - 1)) return false;
        return kind == 0 ? ref[(size_t)(u + 1)] == comp(ref[(size_t)v]) : comp(ref[(size_t)u]) == ref[(size_t)(v - 1)];
    };
    *t1 = 0;
    while (up(x + *t1, y - *t1)) ++*t1;
    *t0 = 0;
    while (ok(x + *t0 - 1) && ok(y - *t0 + 1) && up(x + *t0 - 1, y - *t0 + 1)) --*t0;
}

void add_record(const AnchorGenome& g, const std::string& rec, int M, Tables& t) {
    const int k = g.k, n = (int)rec.size();
    t.n.records++;
    if (n < 2 * k) return;
    const EndAnchors ends = end_anchors(g, rec);
    const int f = ends.f_off, b = ends.b_off;
    const uint32_t cf = ends.f_cell, cg = ends.b_cell;
    const bool f_ag = ends.f_ag, b_ag = ends.b_ag;
    if (f < 0 || b < 0) return;
    if (f_ag == b_ag) {                              // both anchors on one strand: what the span needs
        const Oriented o = orient(rec, k, ends);
        if (o.a + k > o.b) return;
        t.n.same_strand++;
        if (t.span.place(g, o, M) == Placed::spanning) t.n.ref_spanning++;
        return;
    }
    if (f + k > b) return;
    t.n.switched++;
    const int kind = f_ag ? 1 : 0;                   // H: front along, back against; T: front against, back along
    const std::string& ref = g.text;
    // the arms' cells: A(j) = a0 + sa * j, B(j) = b0 + sb * j; an arm that runs down the reference reads its complement
    const int64_t sa = kind == 0 ? 1 : -1, sb = -sa;
    const int64_t a0 = kind == 0 ? (int64_t)cf - f : (int64_t)cf + k - 1 + f, b0 = kind == 0 ? (int64_t)cg + k - 1 + b : (int64_t)cg - b;
    const int s = g.seq_of(cf);
    if (g.seq_of(cg) != s) return;
    auto inside = [&](int64_t c) { return c >= g.first[(size_t)s] && c < g.first[(size_t)s + 1] && is_acgt(ref[(size_t)c]); };
    for (int j = 0; j < b; j++) if (!inside(a0 + sa * j)) return;
    for (int j = f + k; j < n; j++) if (!inside(b0 + sb * j)) return;
    auto mm_a = [&](int j) { const char c = ref[(size_t)(a0 + sa * j)]; return rec[(size_t)j] != (sa > 0 ? c : comp(c)) ? 1 : 0; };
    auto mm_b = [&](int j) { const char c = ref[(size_t)(b0 + sb * j)]; return rec[(size_t)j] != (sb > 0 ? c : comp(c)) ? 1 : 0; };
    // m(f + k), then one comparison exchanged per step
    const int p0 = f + k;
    int64_t m = 0;
    for (int j = 0; j < p0; j++) m += mm_a(j);
    for (int j = p0; j < n; j++) m += mm_b(j);
    auto low = [&](int p) { return std::min(a0 + sa * (p - 1), b0 + sb * p); };
    int64_t best = m, best_low = low(p0);
    int best_p = p0;
    for (int p = p0; p < b; p++) {
        m += mm_a(p) - mm_b(p);
        const int64_t lw = low(p + 1);
        if (m < best || (m == best && lw < best_low)) { best = m; best_low = lw; best_p = p + 1; }
    }
    if (best > M) { t.n.discordant++; return; }
    t.n.supporting++;
    const int64_t x = a0 + sa * (best_p - 1), y = b0 + sb * best_p;
    int64_t t0, t1;
    slide_run(g, (size_t)s, kind, x, y, &t0, &t1);
    int64_t lo, hi;
    if (x + t0 <= y - t1) { lo = x + t0; hi = y - t0; } else { lo = y - t1; hi = x + t1; }
    auto& e = t.events[std::make_tuple((uint32_t)(g.cell0 + lo), (uint32_t)(g.cell0 + hi), (uint32_t)kind)];
    (x <= y ? e.first : e.second)++;
}

}  // namespace

CopybackResult copyback_events(const Index& ix, int file, const std::vector<std::string>& reads, int max_mismatches) {
    if (max_mismatches < 0 || max_mismatches > kCopybackMaxMismatches) throw std::runtime_error("copyback_events: max_mismatches must be 0..8");
    const AnchorGenome g(ix, file);
    Tables t(g);
    for_each_record(reads, g.k, [&](const std::string& rec) { add_record(g, rec, max_mismatches, t); });
    CopybackResult out;
    out.n = t.n;
    const std::vector<uint32_t> sums = t.span.sums(ix, g, &out.span);
    for (const auto& kv : t.events) {               // (the map's order is (lo, hi, kind))
        CopybackEvent e;
        std::tie(e.lo, e.hi, e.kind) = kv.first;
        e.lo_first = kv.second.first; e.hi_first = kv.second.second;
        const size_t off = e.kind == 0 ? 1 : 0;
        e.span_lo = sums[(size_t)(e.lo - g.cell0) + off]; e.span_hi = sums[(size_t)(e.hi - g.cell0) + off];
        out.events.push_back(e);
    }
    return out;
}

void write_copybacks_tsv(const std::string& out_path, const Index& ix, int file, std::vector<CopybackEvent> events, const CopybackParams& p) {
    const FileCells g(ix, file);
    const OutFile fp("copybacks", out_path);
    fprintf(fp, "##copyback_max_mismatches=%u\n##copyback_min_reads=%llu\n##copyback_min_dist=%u\n", p.max_mismatches, (unsigned long long)p.min_reads, p.min_dist);
    fputs("chrom\tkind\tlo\thi\tdistance\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology\n", fp);
    // (one sequence holds both cells, and the sequences' cells ascend: ordered by sequence, kind, lo, hi)
    std::sort(events.begin(), events.end(), [&](const CopybackEvent& x, const CopybackEvent& y) {
        return std::make_tuple(g.seq_of((int64_t)x.lo - g.cell0), x.kind, x.lo, x.hi) < std::make_tuple(g.seq_of((int64_t)y.lo - g.cell0), y.kind, y.lo, y.hi);
    });
    const FileMeta& fm = ix.files[(size_t)file];
    for (const CopybackEvent& e : events) {
        const int64_t lo = (int64_t)e.lo - g.cell0, hi = (int64_t)e.hi - g.cell0;
        if (lo < 0 || hi < lo || hi >= (int64_t)g.text.size() || e.kind > 1) throw std::runtime_error("write_copybacks_tsv: an event outside the genome file's sequences");
        const size_t s = (size_t)g.seq_of(lo);
        if (hi >= g.first[s + 1] || !is_acgt(g.text[(size_t)lo]) || !is_acgt(g.text[(size_t)hi]))
            throw std::runtime_error("write_copybacks_tsv: an event outside the genome file's sequences");
        int64_t t0, t1;
        slide_run(g, s, (int)e.kind, lo, hi, &t0, &t1);
        const uint64_t reads = (uint64_t)e.lo_first + e.hi_first;
        fprintf(fp, "%s\t%c\t%lld\t%lld\t%lld\t%u\t%u\t%llu\t%u\t%u\t%s\t%lld\n", chrom_of(fm.sequences[s].name).c_str(), e.kind == 0 ? 'H' : 'T',
                (long long)(lo - g.first[s] + 1), (long long)(hi - g.first[s] + 1), (long long)(hi - lo), e.lo_first, e.hi_first, (unsigned long long)reads,
                e.span_lo, e.span_hi, freq_text(reads, std::max(e.span_lo, e.span_hi)).c_str(), (long long)(t1 - t0));
    }
    fp.finish();
}

}  // namespace bronko
