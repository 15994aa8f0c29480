// pack_cat -- what fastq_pack.hpp makes of a FASTQ(.gz) file, as text: pack_cat FILE K THREADS [quiet] [--min-qual=Q] [--ends] writes
// every packed record's bases, one per line, in the order they come, then "reads N records M"; exit code 1 and a message on stderr
// for a damaged file.  --min-qual=Q: bases whose quality byte is below '!' + Q are N (FastqPacker's min_qual; 0 is off).
// --ends: the reader is asked for the records' end flags (--primers) and every line ends in a tab and the record's flags, 0..3.
// tests/test_fastq_pack.py compares the parallel reader (THREADS > 1) with the line loop (THREADS = 1).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fastq_pack.hpp"

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: pack_cat FILE K THREADS [quiet] [--min-qual=Q]\n"); return 2; }
    const int k = atoi(argv[2]);
    const unsigned threads = (unsigned)atoi(argv[3]);
    bool quiet = false;   // (another argument: only the counts -- timing the reader, not the printing)
    int min_qual = 0;
    bool ends = false;
    for (int i = 4; i < argc; i++) {
        if (strncmp(argv[i], "--min-qual=", 11) == 0) {
            char* end = nullptr;
            const long v = strtol(argv[i] + 11, &end, 10);
            if (end == argv[i] + 11 || *end || v < 0 || v > 93) { fprintf(stderr, "pack_cat: --min-qual must be 0..93\n"); return 2; }
            min_qual = (int)v;
        }
        else if (strcmp(argv[i], "--ends") == 0) ends = true;
        else quiet = true;
    }
    try {
        bronko::FastqPacker in(argv[1], k, threads, min_qual, ends);
        bronko::PackedBatch b;
        uint64_t reads = 0, records = 0;
        std::string line;
        while (in.next(b)) {
            reads += b.n_reads; records += b.n_records;
            for (uint64_t r = 0; r < b.n_records && !quiet; r++) {
                line.clear();
                const uint32_t* w = b.words.data() + r * b.stride;
                for (uint32_t i = 0; i < b.lens[r]; i++) line.push_back("ACGT"[(w[i >> 4] >> (2 * (i & 15))) & 3u]);
                if (ends) { line.push_back('\t'); line.push_back((char)('0' + (r < b.ends.size() ? b.ends[r] : 9))); }
                line.push_back('\n');
                fwrite(line.data(), 1, line.size(), stdout);
            }
        }
        printf("reads %llu records %llu\n", (unsigned long long)reads, (unsigned long long)records);
    } catch (const std::exception& e) {
        fflush(stdout);
        fprintf(stderr, "pack_cat: %s\n", e.what());
        return 1;
    }
    return 0;
}
