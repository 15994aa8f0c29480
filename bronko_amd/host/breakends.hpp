// breakends.hpp -- `bronko call --breakends`: the host twin of the engine's breakend pass (bk_breakends.hip) and the writer of
// OUT/<stem>.breakends.tsv.  The rule is stated in include/bronko_hip.h (bk_breakends_enable) and DESIGN.md section E; this file
// restates it in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the Python
// restatement (tests/breakends_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr int kBreakendMaxMismatches = 8;
constexpr long kBreakendMinClipLo = 16, kBreakendMinClipHi = 65519;

// One event, as bk_breakend_record: the read holds `cell` and, side 0 = L, the cells below it, side 1 = R, the cells above it, and
// leaves the reference beyond it; tag: the 16 clipped bases next to the breakpoint along the reference, base t at bits [2t, 2t + 2)
struct BreakendEvent {
    uint32_t cell = 0, tag = 0, side = 0;
    uint32_t fwd = 0, rev = 0, site_reads = 0, span = 0, pad = 0;
};
struct BreakendCounters { uint64_t records = 0, one_anchor = 0, ref_spanning = 0, supporting = 0, short_ = 0, through = 0, discordant = 0, unplaced = 0; };
struct BreakendResult {
    std::vector<BreakendEvent> events;    // every event, sorted by (cell, side, tag), site_reads and span filled in
    std::vector<uint32_t> span;           // [total_cells] the prefix-summed span array
    BreakendCounters n;
};
struct BreakendParams {
    uint32_t min_clip = 20;
    uint32_t max_mismatches = 2;
    uint64_t min_reads = 5;
};
// the tallies the ##breakend_tallies line prints (bk_breakend_summary without overflow)
struct BreakendTallies { uint64_t records = 0, one_anchor = 0, ref_spanning = 0, supporting = 0, short_ = 0, through = 0, discordant = 0, unplaced = 0, candidates = 0, reported = 0; };

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
BreakendResult breakend_events(const Index& ix, int file, const std::vector<std::string>& reads, int min_clip, int max_mismatches);

// OUT/<stem>.breakends.tsv: the three ##breakend_* lines of the parameters, the ##breakend_tallies line, the column line, one line
// per event of `events` (sorted here by cell, side, tag's letters)
void write_breakends_tsv(const std::string& out_path, const Index& ix, int file, std::vector<BreakendEvent> events, const BreakendParams& p,
                         const BreakendTallies& t);

}  // namespace bronko
