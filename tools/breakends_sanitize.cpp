// breakends_sanitize.cpp -- a stand-alone program over the host twin of the breakend pass (bronko_amd/host/breakends.cpp), meant to be
// built with -fsanitize=address,undefined (make -C bronko_amd/host sanitize-breakends) and run on the CPU: tools/breakends_sanitize.py
// writes the crafted records of tests/breakend_cases.py and runs it.
//   breakends_sanitize K GENOME.fa READS.txt OUT.tsv     (one read per line)
// It counts every record at (min_clip, max_mismatches) = (20, 2), (16, 0) and (40, 8), writes the TSV of each table, and prints what it
// counted.  Then the twins of the other five event passes (indels, junctions, copybacks, duplications, chimeras) read the same genome
// and records with their default parameters and write their reports, so that the code the six share (anchor_genome.hpp,
// event_twin.hpp) runs under every pass's rule.  Exit status 0 unless a twin throws or the sanitizers find something.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bronko_amd/host/breakends.hpp"
#include "../bronko_amd/host/chimeras.hpp"
#include "../bronko_amd/host/copybacks.hpp"
#include "../bronko_amd/host/duplications.hpp"
#include "../bronko_amd/host/indels.hpp"
#include "../bronko_amd/host/index.hpp"
#include "../bronko_amd/host/junctions.hpp"

namespace {
// what a twin counted: its events, its reference-spanning records, the sum of its span array
template <class Result>
void report(const char* pass, const Result& r) {
    unsigned long long sum = 0;
    for (uint32_t v : r.span) sum += v;
    printf("%s records=%llu ref_spanning=%llu supporting=%llu events=%zu span_sum=%llu\n", pass, (unsigned long long)r.n.records, (unsigned long long)r.n.ref_spanning,
           (unsigned long long)r.n.supporting, r.events.size(), sum);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: breakends_sanitize K GENOME.fa READS.txt OUT.tsv\n"); return 2; }
    try {
        const int k = atoi(argv[1]);
        const bronko::Index ix = bronko::build_indexes(k, {argv[2]}, 2);
        std::vector<std::string> reads;
        std::string line;
        for (std::ifstream in(argv[3]); std::getline(in, line);) reads.push_back(line);
        const int settings[3][2] = {{20, 2}, {16, 0}, {40, 8}};
        for (const auto& cm : settings) {
            const bronko::BreakendResult r = bronko::breakend_events(ix, 0, reads, cm[0], cm[1]);
            bronko::BreakendParams prm;
            prm.min_clip = (uint32_t)cm[0]; prm.max_mismatches = (uint32_t)cm[1]; prm.min_reads = 1;
            bronko::BreakendTallies t;
            t.records = r.n.records; t.one_anchor = r.n.one_anchor; t.ref_spanning = r.n.ref_spanning; t.supporting = r.n.supporting; t.short_ = r.n.short_;
            t.through = r.n.through; t.discordant = r.n.discordant; t.unplaced = r.n.unplaced; t.candidates = t.reported = r.events.size();
            bronko::write_breakends_tsv(argv[4], ix, 0, r.events, prm, t);
            printf("C=%d M=%d records=%llu one_anchor=%llu ref_spanning=%llu supporting=%llu short=%llu through=%llu discordant=%llu unplaced=%llu events=%zu\n", cm[0],
                   cm[1], (unsigned long long)r.n.records, (unsigned long long)r.n.one_anchor, (unsigned long long)r.n.ref_spanning, (unsigned long long)r.n.supporting,
                   (unsigned long long)r.n.short_, (unsigned long long)r.n.through, (unsigned long long)r.n.discordant, (unsigned long long)r.n.unplaced, r.events.size());
        }
        try { (void)bronko::breakend_events(ix, 0, reads, 15, 2); return 1; } catch (const std::runtime_error&) {}   // (the refusals as well)
        try { (void)bronko::breakend_events(ix, 0, reads, 20, 9); return 1; } catch (const std::runtime_error&) {}
        const std::string out = argv[4];
        const bronko::IndelParams ip;
        const bronko::IndelResult ir = bronko::indel_events(ix, 0, reads, (int)ip.max_len, (int)ip.max_mismatches);
        bronko::write_indels_vcf(out, argv[3], ix, 0, ir.events, ip);
        report("indels", ir);
        const bronko::JunctionParams jp;
        const bronko::JunctionResult jr = bronko::junction_events(ix, 0, reads, jp.min_len, (int)jp.max_mismatches);
        bronko::write_junctions_tsv(out, ix, 0, jr.events, jp);
        report("junctions", jr);
        const bronko::CopybackParams cp;
        const bronko::CopybackResult cr = bronko::copyback_events(ix, 0, reads, (int)cp.max_mismatches);
        bronko::write_copybacks_tsv(out, ix, 0, cr.events, cp);
        report("copybacks", cr);
        const bronko::DuplicationParams dp;
        const bronko::DuplicationResult dr = bronko::duplication_events(ix, 0, reads, dp.min_len, (int)dp.max_mismatches);
        bronko::write_duplications_tsv(out, ix, 0, dr.events, dp);
        report("duplications", dr);
        const bronko::ChimeraParams hp;
        const bronko::ChimeraResult hr = bronko::chimera_events(ix, 0, reads, (int)hp.max_mismatches);
        bronko::write_chimeras_tsv(out, ix, 0, hr.events, hp, hr.n.supporting, hr.n.ref_spanning);
        report("chimeras", hr);
    } catch (const std::exception& e) { fprintf(stderr, "breakends_sanitize: %s\n", e.what()); return 1; }
    return 0;
}
