// chimeras.cpp -- the host twin of bk_chimeras.hip and the .chimeras.tsv writer (chimeras.hpp).
#include "chimeras.hpp"

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
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (lo, hi, sides) -> lo_first, hi_first
    SpanCount span;
    ChimeraCounters n;
    explicit Tables(const FileCells& g) : span(g) {}
};

// One arm: the cell of offset j is c0 + d * j, in sequence s; along the reference (d = +1) the read shows the cell's letter, against
// it (d = -1) the complement
struct Arm {
    const FileCells& g;
    int64_t c0, d;
    size_t s;
    int64_t cell(int64_t j) const { return c0 + d * j; }
    bool holds(int64_t c) const { return c >= g.first[s] && c < g.first[s + 1] && is_acgt(g.text[(size_t)c]); }
    char base(int64_t c) const { return d > 0 ? g.text[(size_t)c] : comp(g.text[(size_t)c]); }
};

// the pairs (x + dA t, y + dB t), t0 <= t <= t1, that the reference cannot tell from (x, y): each cell inside its arm's sequence, ACGT
void slide_run(const Arm& a, const Arm& b, int64_t x, int64_t y, int64_t* t0, int64_t* t1) {
    auto up = [&](int64_t t) {                       // from the pair of t to the pair of t + 1
        const int64_t u = x + a.d * (t + 1), v = y + b.d * (t + 1);
        return a.holds(u) && b.holds(v) && a.base(u) == b.base(y + b.d * t);
    };
    *t1 = 0;
    while (up(*t1)) ++*t1;
    *t0 = 0;
    while (a.holds(x + a.d * (*t0 - 1)) && b.holds(y + b.d * (*t0 - 1)) && up(*t0 - 1)) --*t0;
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
    const size_t sx = (size_t)g.seq_of(cf), sy = (size_t)g.seq_of(cg);
    if (sx == sy) {                                  // both anchors in one sequence: on one strand, what the span needs
        if (f_ag != b_ag) return;
        const Oriented o = orient(rec, k, ends);
        if (o.a + k > o.b) return;
        t.n.same_strand++;
        if (t.span.place(g, o, M) == Placed::spanning) t.n.ref_spanning++;
        return;
    }
    if (f + k > b) return;
    t.n.crossed++;
    const Arm A{g, f_ag ? (int64_t)cf + k - 1 + f : (int64_t)cf - f, f_ag ? -1 : 1, sx};
    const Arm B{g, b_ag ? (int64_t)cg + k - 1 + b : (int64_t)cg - b, b_ag ? -1 : 1, sy};
    for (int j = 0; j < b; j++) if (!A.holds(A.cell(j))) return;
    for (int j = f + k; j < n; j++) if (!B.holds(B.cell(j))) return;
    auto mm_a = [&](int j) { return rec[(size_t)j] != A.base(A.cell(j)) ? 1 : 0; };
    auto mm_b = [&](int j) { return rec[(size_t)j] != B.base(B.cell(j)) ? 1 : 0; };
    // m(f + k), then one comparison exchanged per step
    const int p0 = f + k;
    int64_t m = 0;
    for (int j = 0; j < p0; j++) m += mm_a(j);
    for (int j = p0; j < n; j++) m += mm_b(j);
    auto low = [&](int p) { return std::min(A.cell(p - 1), B.cell(p)); };
    int64_t best = m, best_low = low(p0);
    int best_p = p0;
    for (int p = p0; p < b; p++) {
        m += mm_a(p) - mm_b(p);
        const int64_t lw = low(p + 1);
        if (m < best || (m == best && lw < best_low)) { best = m; best_low = lw; best_p = p + 1; }
    }
    if (best > M) { t.n.discordant++; return; }
    t.n.supporting++;
    const int64_t x = A.cell(best_p - 1), y = B.cell(best_p);
    int64_t t0, t1;
    slide_run(A, B, x, y, &t0, &t1);
    // the extreme pair whose smaller cell is smaller: the cell of the lower sequence decides
    const bool a_low = x < y;
    const int64_t te = (a_low ? A.d : B.d) > 0 ? t0 : t1;
    const int64_t ex = x + A.d * te, ey = y + B.d * te;
    const uint32_t side_x = f_ag ? 1u : 0u, side_y = b_ag ? 0u : 1u;
    const uint32_t lo = (uint32_t)(g.cell0 + (a_low ? ex : ey)), hi = (uint32_t)(g.cell0 + (a_low ? ey : ex));
    const uint32_t sides = a_low ? side_x | (side_y << 1) : side_y | (side_x << 1);
    auto& e = t.events[std::make_tuple(lo, hi, sides)];
    (a_low ? e.first : e.second)++;
}

}  // namespace

ChimeraResult chimera_events(const Index& ix, int file, const std::vector<std::string>& reads, int max_mismatches) {
    if (max_mismatches < 0 || max_mismatches > kChimeraMaxMismatches) throw std::runtime_error("chimera_events: max_mismatches must be 0..8");
    const AnchorGenome g(ix, file);
    Tables t(g);
    for_each_record(reads, g.k, [&](const std::string& rec) { add_record(g, rec, max_mismatches, t); });
    ChimeraResult out;
    out.n = t.n;
    const std::vector<uint32_t> sums = t.span.sums(ix, g, &out.span);
    for (const auto& kv : t.events) {               // (the map's order is (lo, hi, sides))
        ChimeraEvent e;
        std::tie(e.lo, e.hi, e.sides) = kv.first;
        e.lo_first = kv.second.first; e.hi_first = kv.second.second;
        e.span_lo = sums[(size_t)(e.lo - g.cell0) + ((e.sides & 1u) ? 0 : 1)]; e.span_hi = sums[(size_t)(e.hi - g.cell0) + ((e.sides & 2u) ? 0 : 1)];
        out.events.push_back(e);
    }
    return out;
}

void write_chimeras_tsv(const std::string& out_path, const Index& ix, int file, std::vector<ChimeraEvent> events, const ChimeraParams& p,
                        uint64_t supporting, uint64_t ref_spanning) {
    const FileCells g(ix, file);
    const OutFile fp("chimeras", out_path);
    fprintf(fp, "##chimera_max_mismatches=%u\n##chimera_min_reads=%llu\n##chimera_supporting=%llu\n##chimera_ref_spanning=%llu\n", p.max_mismatches,
            (unsigned long long)p.min_reads, (unsigned long long)supporting, (unsigned long long)ref_spanning);
    fputs("chrom_lo\tpos_lo\tside_lo\tchrom_hi\tpos_hi\tside_hi\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology\n", fp);
    std::sort(events.begin(), events.end(), [](const ChimeraEvent& x, const ChimeraEvent& y) {
        return std::make_tuple(x.lo, x.sides & 1u, x.hi, x.sides >> 1) < std::make_tuple(y.lo, y.sides & 1u, y.hi, y.sides >> 1);
    });
    const FileMeta& fm = ix.files[(size_t)file];
    for (const ChimeraEvent& e : events) {
        const int64_t lo = (int64_t)e.lo - g.cell0, hi = (int64_t)e.hi - g.cell0;
        if (lo < 0 || hi <= lo || hi >= (int64_t)g.text.size() || e.sides > 3) throw std::runtime_error("write_chimeras_tsv: an event outside the genome file's sequences");
        const size_t sx = (size_t)g.seq_of(lo), sy = (size_t)g.seq_of(hi);
        if (sx == sy || !is_acgt(g.text[(size_t)lo]) || !is_acgt(g.text[(size_t)hi]))
            throw std::runtime_error("write_chimeras_tsv: an event that does not join two sequences of the genome file");
        // the arm at lo taken as arm A: side L runs up to its cell, side R down to it; the arm at hi as arm B: side R goes on upward
        const Arm A{g, 0, (e.sides & 1u) ? -1 : 1, sx}, B{g, 0, (e.sides & 2u) ? 1 : -1, sy};
        int64_t t0, t1;
        slide_run(A, B, lo, hi, &t0, &t1);
        const uint64_t reads = (uint64_t)e.lo_first + e.hi_first;
        fprintf(fp, "%s\t%lld\t%c\t%s\t%lld\t%c\t%u\t%u\t%llu\t%u\t%u\t%s\t%lld\n", chrom_of(fm.sequences[sx].name).c_str(), (long long)(lo - g.first[sx] + 1),
                (e.sides & 1u) ? 'R' : 'L', chrom_of(fm.sequences[sy].name).c_str(), (long long)(hi - g.first[sy] + 1), (e.sides & 2u) ? 'R' : 'L', e.lo_first,
                e.hi_first, (unsigned long long)reads, e.span_lo, e.span_hi, freq_text(reads, std::max(e.span_lo, e.span_hi)).c_str(), (long long)(t1 - t0));
    }
    fp.finish();
}

}  // namespace bronko
