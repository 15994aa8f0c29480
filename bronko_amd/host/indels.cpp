// indels.cpp -- the host twin of bk_indels.hip and the .indels.vcf writer (indels.hpp).
#include "indels.hpp"

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
    std::map<std::tuple<uint32_t, int, int, uint64_t>, std::pair<uint32_t, uint32_t>> events;   // (cell, kind, length, seq) -> fwd, rev
    SpanCount span;
    IndelCounters n;
    explicit Tables(const FileCells& g) : span(g) {}
};

void add_record(const AnchorGenome& g, const std::string& rec, int L, int M, Tables& t) {
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
    const int64_t dL = o.ca - a, dR = o.cb - b, delta = dR - dL;
    if (delta > L || -delta > L) { t.n.discordant++; return; }
    switch (t.span.place(g, o, M)) {
        case Placed::outside: return;
        case Placed::discordant: t.n.discordant++; return;
        case Placed::spanning: t.n.ref_spanning++; return;
        case Placed::shifted: break;
    }
    const int s = g.seq_of(o.ca);
    if (!g.holds_acgt((size_t)s, std::min(dL, dR), std::max(dL, dR) + n)) return;
    const std::string& ref = g.text;
    auto mm = [&](int64_t j, int64_t d) { return r[(size_t)j] != ref[(size_t)(d + j)] ? 1 : 0; };
    auto floor_of = [&](int64_t pos) {               // first cell of the stretch of ACGT letters of the sequence that holds pos - 1
        int64_t f = pos - 1;
        while (f - 1 >= g.first[(size_t)s] && is_acgt(ref[(size_t)(f - 1)])) f--;
        return f;
    };
    const int64_t I = delta < 0 ? -delta : 0, D = delta > 0 ? delta : 0;
    const int64_t p0 = a + k, p1 = b - I;            // the breakpoint's range
    if (p0 > p1) { t.n.discordant++; return; }
    // m(p0), then one comparison exchanged per step
    int64_t m = 0;
    for (int64_t j = 0; j < p0; j++) m += mm(j, dL);
    for (int64_t j = p0 + I; j < n; j++) m += mm(j, dR);
    int64_t best = m, best_p = p0;
    for (int64_t p = p0; p < p1; p++) {
        m += mm(p, dL) - mm(p + I, dR);
        if (m < best) { best = m; best_p = p + 1; }
    }
    if (best > M) { t.n.discordant++; return; }
    int64_t pos = dL + best_p;
    const int64_t F = floor_of(pos);
    uint64_t seq = 0;
    if (D) {
        while (pos - 1 > F && ref[(size_t)(pos - 1)] == ref[(size_t)(pos + D - 1)]) pos--;
    } else {
        std::string S = r.substr((size_t)best_p, (size_t)I);
        while (pos - 1 > F && ref[(size_t)(pos - 1)] == S.back()) { S.insert(S.begin(), S.back()); S.pop_back(); pos--; }
        for (size_t i = 0; i < S.size(); i++) seq |= (uint64_t)nt_to_bits((uint8_t)S[i]) << (2 * i);
    }
    t.n.supporting++;
    auto& e = t.events[std::make_tuple((uint32_t)(g.cell0 + pos), D ? 0 : 1, (int)(D ? D : I), seq)];
    (o.against ? e.second : e.first)++;
}

}  // namespace

bool indel_event_less(const IndelEvent& x, const IndelEvent& y) {
    const int kx = x.len < 0, ky = y.len < 0;
    const int32_t lx = x.len < 0 ? -x.len : x.len, ly = y.len < 0 ? -y.len : y.len;
    return std::tie(x.cell, kx, lx, x.seq) < std::tie(y.cell, ky, ly, y.seq);
}

IndelResult indel_events(const Index& ix, int file, const std::vector<std::string>& reads, int max_len, int max_mismatches) {
    if (max_len < 1 || max_len > kIndelMaxLen) throw std::runtime_error("indel_events: max_len must be 1..32");
    if (max_mismatches < 0 || max_mismatches > kIndelMaxMismatches) throw std::runtime_error("indel_events: max_mismatches must be 0..8");
    const AnchorGenome g(ix, file);
    Tables t(g);
    for_each_record(reads, g.k, [&](const std::string& rec) { add_record(g, rec, max_len, max_mismatches, t); });
    IndelResult out;
    out.n = t.n;
    const std::vector<uint32_t> sums = t.span.sums(ix, g, &out.span);
    for (const auto& kv : t.events) {
        IndelEvent e;
        e.cell = std::get<0>(kv.first);
        e.len = std::get<1>(kv.first) == 0 ? std::get<2>(kv.first) : -std::get<2>(kv.first);
        e.seq = std::get<3>(kv.first);
        e.fwd = kv.second.first; e.rev = kv.second.second;
        e.ref_span = sums[(size_t)(e.cell - g.cell0)];
        out.events.push_back(e);
    }
    std::sort(out.events.begin(), out.events.end(), indel_event_less);
    return out;
}

bool indel_reported(const IndelEvent& e, uint64_t min_reads, uint32_t min_af_ppm) {
    const uint64_t support = (uint64_t)e.fwd + e.rev;
    return support >= min_reads && support * 1000000ull >= (uint64_t)min_af_ppm * (support + e.ref_span);
}

void write_indels_vcf(const std::string& out_path, const std::string& reads_path, const Index& ix, int file, std::vector<IndelEvent> events,
                      const IndelParams& p) {
    if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("write_indels_vcf: no such genome file");
    const OutFile fp("indel vcf", out_path);
    const FileMeta& fm = ix.files[(size_t)file];
    fprintf(fp, "##fileformat=VCFv4.5\n##source=bronko-v0.1.0\n##reference=file://%s\n", reads_path.c_str());
    for (const auto& s : fm.sequences) fprintf(fp, "##contig=<ID=%s,length=%llu>\n", chrom_of(s.name).c_str(), (unsigned long long)s.len);
    fputs("##INFO=<ID=TYPE,Number=1,Type=String,Description=\"DEL or INS\">\n"
          "##INFO=<ID=LEN,Number=1,Type=Integer,Description=\"Bases deleted or inserted\">\n"
          "##INFO=<ID=SF,Number=1,Type=Integer,Description=\"Supporting records along the reference\">\n"
          "##INFO=<ID=SR,Number=1,Type=Integer,Description=\"Supporting records against the reference\">\n"
          "##INFO=<ID=RS,Number=1,Type=Integer,Description=\"Records that span the site without an indel\">\n"
          "##INFO=<ID=AF,Number=1,Type=Float,Description=\"(SF + SR) / (SF + SR + RS)\">\n", fp);
    fprintf(fp, "##indel_max_len=%u\n##indel_max_mismatches=%u\n##indel_min_reads=%llu\n##indel_min_af=%u.%06u\n", p.max_len, p.max_mismatches,
            (unsigned long long)p.min_reads, p.min_af_ppm / 1000000u, p.min_af_ppm % 1000000u);
    fputs("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", fp);
    uint64_t cell0 = 0;
    for (int f = 0; f < file; f++) cell0 += ix.genome_len((size_t)f);
    std::sort(events.begin(), events.end(), indel_event_less);
    for (const IndelEvent& e : events) {
        uint64_t at = cell0;
        const SeqMeta* sm = nullptr;
        for (const auto& s : fm.sequences) { if (e.cell >= at && e.cell < at + s.len) { sm = &s; break; } at += s.len; }
        const uint64_t len = (uint64_t)(e.len < 0 ? -e.len : e.len);
        if (!sm || e.cell == at || (e.len > 0 && e.cell + len > at + sm->len)) throw std::runtime_error("write_indels_vcf: an event outside the genome file's sequences");
        auto up = [](uint8_t c) { return (char)(c >= 'a' && c <= 'z' ? c - 32 : c); };
        const uint64_t i = e.cell - at;              // offset in the sequence; the base before the event is i - 1, 1-based position i
        std::string ref_a(1, up(sm->seq[i - 1])), alt_a(ref_a);
        if (e.len > 0) for (uint64_t j = 0; j < len; j++) ref_a.push_back(up(sm->seq[i + j]));
        else for (uint64_t j = 0; j < len; j++) alt_a.push_back("ACGT"[(e.seq >> (2 * j)) & 3u]);
        fprintf(fp, "%s\t%llu\t.\t%s\t%s\t.\tPASS\tTYPE=%s;LEN=%llu;SF=%u;SR=%u;RS=%u;AF=%s\n", chrom_of(sm->name).c_str(), (unsigned long long)i,
                ref_a.c_str(), alt_a.c_str(), e.len > 0 ? "DEL" : "INS", (unsigned long long)len, e.fwd, e.rev, e.ref_span,
                freq_text((uint64_t)e.fwd + e.rev, e.ref_span).c_str());
    }
    fp.finish();
}

}  // namespace bronko
