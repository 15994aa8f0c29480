// chimeras.hpp -- `bronko call --chimeras`: the host twin of the engine's chimera pass (bk_chimeras.hip) and the writer of
// OUT/<stem>.chimeras.tsv.  The rule is stated in include/bronko_hip.h (bk_chimeras_enable) and DESIGN.md section X; this file
// restates it in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the Python
// restatement (tests/chimeras_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr int kChimeraMaxMismatches = 8;

// One event, as bk_chimera_record: the read joins the cells lo < hi of two sequences; sides bit 0 the side of lo, bit 1 the side of
// hi; 0 = L (the read holds the cell and the cells below it), 1 = R (the cell and the cells above it)
struct ChimeraEvent {
    uint32_t lo = 0, hi = 0, sides = 0;
    uint32_t lo_first = 0, hi_first = 0, span_lo = 0, span_hi = 0, pad = 0;
};
struct ChimeraCounters { uint64_t records = 0, same_strand = 0, ref_spanning = 0, crossed = 0, supporting = 0, discordant = 0; };
struct ChimeraResult {
    std::vector<ChimeraEvent> events;     // every event, sorted by (lo, hi, sides), the two spans filled in
    std::vector<uint32_t> span;           // [total_cells] the prefix-summed span array
    ChimeraCounters n;
};
struct ChimeraParams {
    uint32_t max_mismatches = 2;
    uint64_t min_reads = 5;
};

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
ChimeraResult chimera_events(const Index& ix, int file, const std::vector<std::string>& reads, int max_mismatches);

// OUT/<stem>.chimeras.tsv: the two ##chimera_* lines of the parameters, the two of the sample's tallies `supporting` and
// `ref_spanning`, the column line, one line per event of `events` (sorted here by lo, side_lo, hi, side_hi); homology is computed
// here from the reference
void write_chimeras_tsv(const std::string& out_path, const Index& ix, int file, std::vector<ChimeraEvent> events, const ChimeraParams& p,
                        uint64_t supporting, uint64_t ref_spanning);

}  // namespace bronko
