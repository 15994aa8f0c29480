// copybacks.hpp -- `bronko call --copybacks`: the host twin of the engine's copy-back pass (bk_copybacks.hip) and the writer of
// OUT/<stem>.copybacks.tsv.  The rule is stated in include/bronko_hip.h (bk_copybacks_enable) and DESIGN.md section B; this file
// restates it in plain C++ over ASCII reads and the index's sequences, so that the CPU tests can hold it against the Python
// restatement (tests/copybacks_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"

namespace bronko {

constexpr int kCopybackMaxMismatches = 8;

// One event, as bk_copyback_record: the read turns between the cells lo <= hi; kind 0 = H (both arms at and below their cells),
// 1 = T (both at and above)
struct CopybackEvent {
    uint32_t lo = 0, hi = 0, kind = 0;
    uint32_t lo_first = 0, hi_first = 0, span_lo = 0, span_hi = 0, pad = 0;
};
struct CopybackCounters { uint64_t records = 0, same_strand = 0, ref_spanning = 0, switched = 0, supporting = 0, discordant = 0; };
struct CopybackResult {
    std::vector<CopybackEvent> events;    // every event, sorted by (lo, hi, kind), the two spans filled in
    std::vector<uint32_t> span;           // [total_cells] the prefix-summed span array
    CopybackCounters n;
};
struct CopybackParams {
    uint32_t max_mismatches = 2;
    uint64_t min_reads = 5;
    uint32_t min_dist = 0;
};

// Every record (run of ACGT letters of at least k bases) of every read against genome file `file` of the index.
CopybackResult copyback_events(const Index& ix, int file, const std::vector<std::string>& reads, int max_mismatches);

// OUT/<stem>.copybacks.tsv: the three ##copyback_* lines, the column line, one line per event of `events` (sorted here by
// sequence, kind, lo, hi); homology is computed here from the reference
void write_copybacks_tsv(const std::string& out_path, const Index& ix, int file, std::vector<CopybackEvent> events, const CopybackParams& p);

}  // namespace bronko
