// copybacks.cpp -- the host twin of bk_copybacks.hip and the .copybacks.tsv writer (copybacks.hpp).
#include "copybacks.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <tuple>

#include "anchor_genome.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

struct Tables {
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::pair<uint32_t, uint32_t>> events;   // (lo, hi, kind) -> lo_first, hi_first
    std::vector<int64_t> span;                       // difference array over the file's cells (+ 2)
    CopybackCounters n;
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

// both anchors on one strand: what the span needs, as junctions.cpp has it
void same_strand(const AnchorGenome& g, const std::string& rec, int f_off, uint32_t f_cell, int b_off, uint32_t b_cell, bool against, int M, Tables& t) {
    const int k = g.k, n = (int)rec.size();
    std::string r = rec;                             // r': the record along the reference
    int64_t a, b, ca, cb;
    if (against) {
        for (int j = 0; j < n; j++) r[(size_t)j] = comp(rec[(size_t)(n - 1 - j)]);
        a = n - k - b_off; ca = b_cell; b = n - k - f_off; cb = f_cell;
    } else { a = f_off; ca = f_cell; b = b_off; cb = b_cell; }
    if (a + k > b) return;
    t.n.same_strand++;
    const int64_t dL = ca - a, dR = cb - b;
    const int s = g.seq_of(ca);
    if (g.seq_of(cb) != s) return;
    const int64_t lo = std::min(dL, dR), hi = std::max(dL, dR) + n;
    if (lo < g.first[(size_t)s] || hi > g.first[(size_t)s + 1]) return;
    for (int64_t c = lo; c < hi; c++) if (!is_acgt(g.text[(size_t)c])) return;
    if (dL != dR) return;
    int m = 0;
    for (int64_t j = 0; j < n; j++) m += r[(size_t)j] != g.text[(size_t)(dL + j)] ? 1 : 0;
    if (m > M) return;
    t.n.ref_spanning++;
    t.span[(size_t)(dL + a + k)] += 1; t.span[(size_t)(dL + b + 1)] -= 1;
}

void add_record(const AnchorGenome& g, const std::string& rec, int M, Tables& t) {
    const int k = g.k, n = (int)rec.size();
    t.n.records++;
    if (n < 2 * k) return;
    int f = -1, b = -1;
    uint32_t cf = 0, cg = 0;
    bool f_ag = false, b_ag = false;
    for (int o = 0; o <= 24 && o + k <= n; o += 8)
        if (g.anchor(rec.data() + o, &cf, &f_ag)) { f = o; break; }
    for (int o = n - k; o >= n - k - 24 && o >= 0; o -= 8)
        if (g.anchor(rec.data() + o, &cg, &b_ag)) { b = o; break; }
    if (f < 0 || b < 0) return;
    if (f_ag == b_ag) { same_strand(g, rec, f, cf, b, cg, f_ag, M, t); return; }
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
    Tables t;
    t.span.assign(g.text.size() + 2, 0);
    std::string run;
    for (const std::string& read : reads) {
        run.clear();
        for (size_t i = 0; i <= read.size(); i++) {
            const char c = i < read.size() ? (char)(read[i] >= 'a' && read[i] <= 'z' ? read[i] - 32 : read[i]) : 'N';
            if (is_acgt(c)) { run.push_back(c); continue; }
            if ((int)run.size() >= g.k) add_record(g, run, max_mismatches, t);
            run.clear();
        }
    }
    CopybackResult out;
    out.n = t.n;
    out.span.assign((size_t)ix.total_cells(), 0u);
    int64_t acc = 0;
    std::vector<uint32_t> sums(g.text.size() + 1);
    for (size_t c = 0; c <= g.text.size(); c++) {
        acc += t.span[c]; sums[c] = (uint32_t)acc;
        if (c < g.text.size()) out.span[(size_t)g.cell0 + c] = (uint32_t)acc;
    }
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
    FILE* fp = fopen(out_path.c_str(), "w");
    if (!fp) throw std::runtime_error("Failed to create copybacks output file " + out_path);
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{fp};
    fprintf(fp, "##copyback_max_mismatches=%u\n##copyback_min_reads=%llu\n##copyback_min_dist=%u\n", p.max_mismatches, (unsigned long long)p.min_reads, p.min_dist);
    fputs("chrom\tkind\tlo\thi\tdistance\tlo_first\thi_first\treads\tspan_lo\tspan_hi\tfreq\thomology\n", fp);
    // (one sequence holds both cells, and the sequences' cells ascend: ordered by sequence, kind, lo, hi)
    auto seq_of = [&](int64_t c) { size_t s = 0; while (s + 2 < g.first.size() && g.first[s + 1] <= c) s++; return s; };
    std::sort(events.begin(), events.end(), [&](const CopybackEvent& x, const CopybackEvent& y) {
        return std::make_tuple(seq_of((int64_t)x.lo - g.cell0), x.kind, x.lo, x.hi) < std::make_tuple(seq_of((int64_t)y.lo - g.cell0), y.kind, y.lo, y.hi);
    });
    const FileMeta& fm = ix.files[(size_t)file];
    for (const CopybackEvent& e : events) {
        const int64_t lo = (int64_t)e.lo - g.cell0, hi = (int64_t)e.hi - g.cell0;
        if (lo < 0 || hi < lo || hi >= (int64_t)g.text.size() || e.kind > 1) throw std::runtime_error("write_copybacks_tsv: an event outside the genome file's sequences");
        const size_t s = seq_of(lo);
        if (hi >= g.first[s + 1] || !is_acgt(g.text[(size_t)lo]) || !is_acgt(g.text[(size_t)hi]))
            throw std::runtime_error("write_copybacks_tsv: an event outside the genome file's sequences");
        int64_t t0, t1;
        slide_run(g, s, (int)e.kind, lo, hi, &t0, &t1);
        const uint64_t reads = (uint64_t)e.lo_first + e.hi_first;
        const uint64_t t = 10000ull * reads / std::max<uint64_t>(1, reads + std::max(e.span_lo, e.span_hi));
        fprintf(fp, "%s\t%c\t%lld\t%lld\t%lld\t%u\t%u\t%llu\t%u\t%u\t%llu.%04llu\t%lld\n", chrom_of(fm.sequences[s].name).c_str(), e.kind == 0 ? 'H' : 'T',
                (long long)(lo - g.first[s] + 1), (long long)(hi - g.first[s] + 1), (long long)(hi - lo), e.lo_first, e.hi_first, (unsigned long long)reads,
                e.span_lo, e.span_hi, (unsigned long long)(t / 10000), (unsigned long long)(t % 10000), (long long)(t1 - t0));
    }
    if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write copybacks file " + out_path);
}

}  // namespace bronko
