// junctions.hpp -- `bronko call --junctions`: the host twin of the engine's junction pass (bk_junctions.hip) and the writer of
// OUT/<stem>.junctions.tsv.  The rule is stated in include/bronko_hip.h (bk_junctions_enable) and DESIGN.md section J; this file
// restates it in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the Python
// restatement (tests/junctions_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr uint32_t kJunctionMaxLen = (1u << 27) - 1;   // BK_JUNCTION_MAX_LEN
constexpr int kJunctionMaxMismatches = 8;

// One event, as bk_junction_record: cell = the first cell left out (left-normalised), len = D; the read continues at cell + len
struct JunctionEvent {
    uint32_t cell = 0, len = 0;
    uint32_t fwd = 0, rev = 0, span_donor = 0, span_acceptor = 0;
};
struct JunctionCounters { uint64_t records = 0, anchored = 0, ref_spanning = 0, supporting = 0, short_ = 0, backward = 0, discordant = 0; };
struct JunctionResult {
    std::vector<JunctionEvent> events;    // every event, sorted by (cell, len), the two spans filled in
    std::vector<uint32_t> span;           // [total_cells] the prefix-summed span array
    JunctionCounters n;
};
struct JunctionParams {
    uint32_t min_len = 33, max_mismatches = 2;
    uint64_t min_reads = 5;
};

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
JunctionResult junction_events(const Index& ix, int file, const std::vector<std::string>& reads, uint32_t min_len, int max_mismatches);

// OUT/<stem>.junctions.tsv: the three ##junction_* lines, the column line, one line per event of `events` (sorted here by
// sequence, donor, acceptor); homology is computed here from the reference
void write_junctions_tsv(const std::string& out_path, const Index& ix, int file, std::vector<JunctionEvent> events, const JunctionParams& p);

}  // namespace bronko
