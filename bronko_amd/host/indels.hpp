// indels.hpp -- `bronko call --indels`: the host twin of the engine's indel pass (bk_indels.hip) and the writer of
// OUT/<stem>.indels.vcf.  The rule is stated in include/bronko_hip.h (bk_indels_enable) and DESIGN.md section I; this file restates
// it in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the Python restatement
// (tests/indels_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr int kIndelMaxLen = 32;          // BK_INDEL_MAX_LEN
constexpr int kIndelMaxMismatches = 8;

// One event, as bk_indel_record: cell = the first deleted cell / the cell the insertion stands in front of (left-normalised),
// len > 0 a deletion, < 0 an insertion; seq = the inserted bases, base t at bits [2t, 2t + 2), A C G T = 0 1 2 3 (0 for a deletion)
struct IndelEvent {
    uint32_t cell = 0;
    int32_t len = 0;
    uint32_t fwd = 0, rev = 0, ref_span = 0;
    uint64_t seq = 0;
};
struct IndelCounters { uint64_t records = 0, anchored = 0, ref_spanning = 0, supporting = 0, discordant = 0; };
struct IndelResult {
    std::vector<IndelEvent> events;       // every event, sorted by (cell, kind, length, seq), ref_span filled in
    std::vector<uint32_t> span;           // [total_cells] the prefix-summed span array
    IndelCounters n;
};
struct IndelParams {
    uint32_t max_len = 32, max_mismatches = 2;
    uint64_t min_reads = 5;
    uint32_t min_af_ppm = 30000;
};

// (cell, kind, length, seq): deletions before insertions at one cell
bool indel_event_less(const IndelEvent& x, const IndelEvent& y);

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
IndelResult indel_events(const Index& ix, int file, const std::vector<std::string>& reads, int max_len, int max_mismatches);

// support >= min_reads and support * 1e6 >= min_af_ppm * (support + ref_span)
bool indel_reported(const IndelEvent& e, uint64_t min_reads, uint32_t min_af_ppm);

// OUT/<stem>.indels.vcf: the main VCF's header lines, the INFO and ##indel_* lines, one line per event of `events` (sorted here)
void write_indels_vcf(const std::string& out_path, const std::string& reads_path, const Index& ix, int file, std::vector<IndelEvent> events,
                      const IndelParams& p);

}  // namespace bronko
