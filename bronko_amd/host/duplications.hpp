// duplications.hpp -- `bronko call --duplications`: the host twin of the engine's duplication pass (bk_duplications.hip) and the
// writer of OUT/<stem>.duplications.tsv.  The rule is stated in include/bronko_hip.h (bk_duplications_enable) and DESIGN.md section
// V; this file restates it in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the
// Python restatement (tests/duplications_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr uint32_t kDuplicationMaxLen = (1u << 27) - 1;   // BK_DUPLICATION_MAX_LEN
constexpr int kDuplicationMaxMismatches = 8;

// One event, as bk_duplication_record: cell = pos, the cell behind the last one read twice (left-normalised), len = E; the cells
// [cell - len, cell) are read twice
struct DuplicationEvent {
    uint32_t cell = 0, len = 0;
    uint32_t fwd = 0, rev = 0, span_start = 0, span_end = 0;
};
struct DuplicationCounters { uint64_t records = 0, anchored = 0, ref_spanning = 0, supporting = 0, short_ = 0, forward = 0, discordant = 0; };
struct DuplicationResult {
    std::vector<DuplicationEvent> events; // every event, sorted by (cell, len), the two spans filled in
    std::vector<uint32_t> span;           // [total_cells] the prefix-summed span array
    DuplicationCounters n;
};
struct DuplicationParams {
    uint32_t min_len = 33, max_mismatches = 2;
    uint64_t min_reads = 5;
};

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
DuplicationResult duplication_events(const Index& ix, int file, const std::vector<std::string>& reads, uint32_t min_len, int max_mismatches);

// OUT/<stem>.duplications.tsv: the three ##duplication_* lines, the column line, one line per event of `events` (sorted here by
// sequence, start, end); homology and whole are computed here from the reference
void write_duplications_tsv(const std::string& out_path, const Index& ix, int file, std::vector<DuplicationEvent> events, const DuplicationParams& p);

}  // namespace bronko
