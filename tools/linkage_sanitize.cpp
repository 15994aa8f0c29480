// linkage_sanitize.cpp -- a stand-alone program over the host twin of the linkage passes (bronko_amd/host/linkage.cpp), meant to be
// built with -fsanitize=address,undefined (make -C bronko_amd/host sanitize-linkage) and run on the CPU: tools/linkage_sanitize.py
// writes the crafted records and sites of tests/linkage_cases.py and runs it.
//   linkage_sanitize K GENOME.fa READS.txt SITES.txt OUT.tsv     (one read / one cell per line)
// It places every record at max_mismatches 0, 2 and 8, counts the pairs at three distances, writes the TSV with one made-up record
// per site, and prints what it counted.  Exit status 0 unless the twin throws or the sanitizers find something.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bronko_amd/host/index.hpp"
#include "../bronko_amd/host/lcb.hpp"
#include "../bronko_amd/host/linkage.hpp"

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: linkage_sanitize K GENOME.fa READS.txt SITES.txt OUT.tsv\n"); return 2; }
    try {
        const int k = atoi(argv[1]);
        const bronko::Index ix = bronko::build_indexes(k, {argv[2]}, 2);
        std::vector<std::string> reads;
        std::vector<uint32_t> sites;
        std::string line;
        for (std::ifstream in(argv[3]); std::getline(in, line);) reads.push_back(line);
        for (std::ifstream in(argv[4]); std::getline(in, line);) if (!line.empty()) sites.push_back((uint32_t)strtoul(line.c_str(), nullptr, 10));
        std::string text;                             // the genome file's cells
        for (const auto& s : ix.files[0].sequences) text.append(s.seq.begin(), s.seq.end());
        for (int M : {0, 2, 8}) {
            const bronko::LinkResult r = bronko::link_rows(ix, 0, reads, M);
            printf("M=%d records=%llu placed=%llu unplaced=%llu discordant=%llu\n", M, (unsigned long long)r.n.records, (unsigned long long)r.n.placed,
                   (unsigned long long)r.n.unplaced, (unsigned long long)r.n.discordant);
            for (uint32_t dist : {2u, 1000u, 65519u}) {
                const std::vector<bronko::LinkPair> pairs = bronko::link_count(ix, 0, r.rows, sites, dist);
                unsigned long long sum = 0;
                for (const auto& p : pairs) for (uint32_t c : p.count) sum += c;
                std::vector<bronko::LinkSite> recs;
                for (uint32_t c : sites) {
                    bronko::LinkSite s;
                    s.cell = c; s.ref_base = bronko::nt_to_bits((uint8_t)text[c]); s.alt_base = (uint8_t)((s.ref_base + 1) & 3);
                    recs.push_back(s);
                }
                bronko::LinkParams prm;
                prm.max_mismatches = (uint32_t)M; prm.max_dist = dist; prm.min_reads = 1;
                const uint64_t lines = bronko::write_linkage_tsv(argv[5], ix, 0, recs, pairs, prm);
                printf("  dist=%u pairs=%zu adds=%llu lines=%llu\n", dist, pairs.size(), sum, (unsigned long long)lines);
            }
        }
        try { (void)bronko::link_count(ix, 0, {}, {5, 5}, 10); return 1; } catch (const std::runtime_error&) {}   // (the refusals as well)
        try { (void)bronko::link_rows(ix, 0, reads, 9); return 1; } catch (const std::runtime_error&) {}
    } catch (const std::exception& e) { fprintf(stderr, "linkage_sanitize: %s\n", e.what()); return 1; }
    return 0;
}
