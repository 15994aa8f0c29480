// consensus_indels.cpp -- the host twin of bk_consensus_indels.hip and the writers of --consensus-indels (consensus_indels.hpp).
#include "consensus_indels.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <tuple>

#include "event_twin.hpp"

namespace bronko {

namespace {

uint32_t length_of(const ConsensusIndel& e) { return (uint32_t)(e.len < 0 ? -e.len : e.len); }

// the sequence of genome file `file` that holds `cell` with a base in front of it, and that sequence's first cell
const SeqMeta& sequence_of(const Index& ix, int file, const ConsensusIndel& e, uint64_t* first) {
    uint64_t at = 0;
    for (int f = 0; f < file; f++) at += ix.genome_len((size_t)f);
    for (const SeqMeta& s : ix.files[(size_t)file].sequences) {
        if (e.cell > at && e.cell < at + s.len && (e.len < 0 || e.cell + length_of(e) <= at + s.len)) { *first = at; return s; }
        at += s.len;
    }
    throw std::runtime_error("consensus indels: an event outside the genome file's sequences");
}

std::string inserted(const ConsensusIndel& e) {
    std::string s;
    for (uint32_t t = 0; t < length_of(e); t++) s.push_back("ACGT"[(e.seq >> (2 * t)) & 3u]);
    return s;
}

}  // namespace

bool consensus_indel_less(const ConsensusIndel& x, const ConsensusIndel& y) {
    const int kx = x.len < 0, ky = y.len < 0;
    const uint32_t lx = length_of(x), ly = length_of(y);
    return std::tie(x.cell, kx, lx, x.seq) < std::tie(y.cell, ky, ly, y.seq);
}

ConsensusIndels consensus_indels(const Index& ix, int file, const std::vector<IndelEvent>& events, const std::vector<uint32_t>& span, uint64_t min_depth,
                                 double min_freq, uint8_t* letters, uint64_t n_letters) {
    if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("consensus_indels: no such genome file");
    if (span.size() < ix.total_cells()) throw std::runtime_error("consensus_indels: the span array is not the index's length");
    if (n_letters != ix.genome_len((size_t)file)) throw std::runtime_error("consensus_indels: the letters are not the genome's length");
    uint64_t cell0 = 0;
    for (int f = 0; f < file; f++) cell0 += ix.genome_len((size_t)f);
    ConsensusIndels out;
    // the accepted events, and on every boundary the supports of the accepted events that occupy it
    std::map<uint64_t, std::vector<uint64_t>> on;
    auto boundaries = [](const ConsensusIndel& e) { return std::make_pair((uint64_t)e.cell, (uint64_t)e.cell + (e.len > 0 ? (uint64_t)e.len : 0)); };
    for (const IndelEvent& ev : events) {
        out.n.candidates++;
        if ((uint64_t)ev.cell >= span.size()) throw std::runtime_error("consensus_indels: an event outside the index's cells");
        const uint64_t s = (uint64_t)ev.fwd + ev.rev, r = span[ev.cell], n = s + r;
        if (!(n >= min_depth && (double)s >= min_freq * (double)n)) continue;
        ConsensusIndel e;
        e.cell = ev.cell; e.len = ev.len; e.seq = ev.seq; e.support = (uint32_t)s; e.ref_span = (uint32_t)r;
        out.events.push_back(e);
        const auto b = boundaries(e);
        for (uint64_t at = b.first; at <= b.second; at++) on[at].push_back(s);
    }
    std::sort(out.events.begin(), out.events.end(), consensus_indel_less);
    out.n.accepted = out.events.size();
    for (ConsensusIndel& e : out.events) {
        const auto b = boundaries(e);
        bool alone = true;   // on each boundary no other accepted event has as much support: the events with at least e's are e alone
        for (uint64_t at = b.first; at <= b.second && alone; at++) {
            const std::vector<uint64_t>& there = on[at];
            alone = std::count_if(there.begin(), there.end(), [&](uint64_t s) { return s >= e.support; }) == 1;
        }
        e.applied = alone ? 1u : 0u;
        if (!alone) { out.n.contested++; continue; }
        out.n.applied++;
        const uint32_t len = length_of(e);
        if (len % 3 != 0) out.n.frameshifts++;
        if (e.len > 0) {
            out.n.deletions++; out.n.deleted_bases += len;
            if (e.cell < cell0 || e.cell - cell0 + len > n_letters) throw std::runtime_error("consensus_indels: a deletion outside the genome file's letters");
            for (uint32_t j = 0; j < len; j++) letters[e.cell - cell0 + j] = '-';
        } else {
            out.n.insertions++; out.n.inserted_bases += len;
        }
    }
    return out;
}

void write_consensus_indels_fasta(const std::string& out_path, const std::string& stem, const Index& ix, int file, const uint8_t* letters, uint64_t n,
                                  const std::vector<ConsensusIndel>& events) {
    if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("write_consensus_indels_fasta: no such genome file");
    if (n != ix.genome_len((size_t)file)) throw std::runtime_error("write_consensus_indels_fasta: the letters are not the genome's length");
    std::map<uint64_t, std::string> put;             // the applied insertions by cell (one a cell: two would have collided)
    for (const ConsensusIndel& e : events)
        if (e.applied && e.len < 0) {
            uint64_t first;
            sequence_of(ix, file, e, &first);
            put[e.cell] = inserted(e);
        }
    const OutFile fp("consensus fasta", out_path);
    uint64_t cell = 0, at = 0;
    for (int f = 0; f < file; f++) cell += ix.genome_len((size_t)f);
    for (const SeqMeta& sm : ix.files[(size_t)file].sequences) {
        fprintf(fp, ">%s|%s\n", stem.c_str(), chrom_of(sm.name).c_str());
        std::string text;
        for (uint64_t i = 0; i < sm.len; i++, cell++, at++) {
            const auto ins = put.find(cell);
            if (ins != put.end()) text += ins->second;
            if (letters[at] != '-') text.push_back((char)letters[at]);
        }
        for (size_t i = 0; i < text.size(); i += 60) {
            fwrite(text.data() + i, 1, std::min<size_t>(60, text.size() - i), fp);
            fputc('\n', fp);
        }
    }
    fp.finish();
}

void write_consensus_indels_tsv(const std::string& out_path, const Index& ix, int file, std::vector<ConsensusIndel> events, uint64_t min_depth, double min_freq) {
    if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("write_consensus_indels_tsv: no such genome file");
    const OutFile fp("consensus indel", out_path);
    fprintf(fp, "##consensus_min_depth=%llu\n##consensus_min_freq=%g\n", (unsigned long long)min_depth, min_freq);
    fputs("chrom\tpos\ttype\tlen\tseq\tsupport\tref_span\taf\tstatus\tcons_pos\n", fp);
    std::sort(events.begin(), events.end(), consensus_indel_less);
    for (const ConsensusIndel& e : events) {
        uint64_t first;
        const SeqMeta& sm = sequence_of(ix, file, e, &first);
        const uint64_t pos = e.cell - first;         // the base in front of the event: offset pos - 1, 1-based position pos
        std::string cons_pos = ".";
        if (e.applied) {
            // that base in the edited sequence: the applied deletions that end at or before it are gone, the applied insertions at
            // smaller cells stand in front of it
            uint64_t gone = 0, more = 0;
            for (const ConsensusIndel& o : events) {
                if (!o.applied || o.cell <= first || o.cell >= first + sm.len) continue;
                if (o.len > 0 && (uint64_t)o.cell + length_of(o) <= e.cell) gone += length_of(o);
                if (o.len < 0 && o.cell < e.cell) more += length_of(o);
            }
            cons_pos = std::to_string(pos - gone + more);
        }
        fprintf(fp, "%s\t%llu\t%s\t%u\t%s\t%u\t%u\t%s\t%s\t%s\n", chrom_of(sm.name).c_str(), (unsigned long long)pos, e.len > 0 ? "DEL" : "INS", length_of(e),
                e.len > 0 ? "." : inserted(e).c_str(), e.support, e.ref_span, freq_text(e.support, e.ref_span).c_str(), e.applied ? "applied" : "contested",
                cons_pos.c_str());
    }
    fp.finish();
}

}  // namespace bronko
