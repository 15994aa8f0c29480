// breakends_sanitize.cpp -- a stand-alone program over the host twin of the breakend pass (bronko_amd/host/breakends.cpp), meant to be
// built with -fsanitize=address,undefined (make -C bronko_amd/host sanitize-breakends) and run on the CPU: tools/breakends_sanitize.py
// writes the crafted records of tests/breakend_cases.py and runs it.
//   breakends_sanitize K GENOME.fa READS.txt OUT.tsv     (one read per line)
// It counts every record at (min_clip, max_mismatches) = (20, 2), (16, 0) and (40, 8), writes the TSV of each table, and prints what it
// counted.  Exit status 0 unless the twin throws or the sanitizers find something.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bronko_amd/host/breakends.hpp"
#include "../bronko_amd/host/index.hpp"

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
    } catch (const std::exception& e) { fprintf(stderr, "breakends_sanitize: %s\n", e.what()); return 1; }
    return 0;
}
