// event_twin.hpp -- what the host twins and writers of the six read-level event passes share beyond anchor_genome.hpp (indels.cpp,
// junctions.cpp, copybacks.cpp, duplications.cpp, chimeras.cpp, breakends.cpp): where a record lies whose anchors stand on one
// strand, the count of the records that span each cell, the report file and its freq column.  Nothing of any one pass's rule: what
// a pass tallies for an outcome, and all that follows once the anchors are known, is in its own file.
#pragma once
#include <cstdio>

#include "anchor_genome.hpp"

namespace bronko {

// Where a record with both anchors on one strand lies on the reference
enum class Placed {
    outside,      // the anchors in two sequences; or on one diagonal, the record over an end of its sequence or a letter that is not ACGT
    shifted,      // the anchors in one sequence on two diagonals (dL != dR): nothing else has been looked at
    discordant,   // on one diagonal, more than M mismatches
    spanning      // on one diagonal, at most M mismatches: a reference-spanning record
};

// The reference-spanning records of one genome file.  Each adds one to the cells dL + a + k .. dL + b, from behind its first anchor
// to the first cell of its second: a difference array over the file's cells while the records are read, its prefix sums at the end
class SpanCount {
    std::vector<int64_t> diff;                       // the file's cells + 2
public:
    explicit SpanCount(const FileCells& g) : diff(g.text.size() + 2, 0) {}
    // places the record (a + k <= b) and counts it where it is spanning
    Placed place(const AnchorGenome& g, const Oriented& o, int M) {
        const int64_t n = (int64_t)o.r.size(), dL = o.ca - o.a, dR = o.cb - o.b;
        const size_t s = (size_t)g.seq_of(o.ca);
        if ((size_t)g.seq_of(o.cb) != s) return Placed::outside;
        if (dL != dR) return Placed::shifted;
        if (!g.holds_acgt(s, dL, dL + n)) return Placed::outside;
        int m = 0;
        for (int64_t j = 0; j < n; j++) m += o.r[(size_t)j] != g.text[(size_t)(dL + j)] ? 1 : 0;
        if (m > M) return Placed::discordant;
        diff[(size_t)(dL + o.a + g.k)] += 1; diff[(size_t)(dL + o.b + 1)] -= 1;
        return Placed::spanning;
    }
    // the prefix sums of the file's cells and of the cell behind them (cells + 1 entries), which the events read; span: the same over
    // all cells of the index, zero outside the file
    std::vector<uint32_t> sums(const Index& ix, const FileCells& g, std::vector<uint32_t>* span) const {
        span->assign((size_t)ix.total_cells(), 0u);
        std::vector<uint32_t> sums(g.text.size() + 1);
        int64_t acc = 0;
        for (size_t c = 0; c <= g.text.size(); c++) {
            acc += diff[c]; sums[c] = (uint32_t)acc;
            if (c < g.text.size()) (*span)[(size_t)g.cell0 + c] = (uint32_t)acc;
        }
        return sums;
    }
};

// A report file: opened or "Failed to create WHAT output file PATH", closed on every path
class OutFile {
    std::string what, path;
    FILE* fp;
public:
    OutFile(const std::string& what_, const std::string& path_) : what(what_), path(path_), fp(fopen(path_.c_str(), "w")) {
        if (!fp) throw std::runtime_error("Failed to create " + what + " output file " + path);
    }
    ~OutFile() { fclose(fp); }
    OutFile(const OutFile&) = delete;
    OutFile& operator=(const OutFile&) = delete;
    operator FILE*() const { return fp; }
    // after the last line: all of it has reached the file, or "Failed to write WHAT file PATH"
    void finish() const {
        if (fflush(fp) != 0 || ferror(fp)) throw std::runtime_error("Failed to write " + what + " file " + path);
    }
};

// the freq column: reads / (reads + span) in four decimals, truncated; computed in integers so that every platform prints the same
inline std::string freq_text(uint64_t reads, uint64_t span) {
    const uint64_t t = 10000ull * reads / std::max<uint64_t>(1, reads + span);
    char buf[32];
    snprintf(buf, sizeof buf, "%llu.%04llu", (unsigned long long)(t / 10000), (unsigned long long)(t % 10000));
    return buf;
}

}  // namespace bronko
