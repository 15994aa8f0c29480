// read_pileup.hpp -- `bronko call --read-pileup`: the host twin of the engine's read pileup (bk_read_pileup.hip) and the writer of
// OUT/<stem>.read_pileup.tsv.  The rule is stated in include/bronko_hip.h (bk_sample_read_pileup) and DESIGN.md section U;
// read_pileup_count restates it in plain C++ over the rows of linkage.hpp, so that the CPU tests can hold it against the Python
// restatement (tests/read_pileup_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "index.hpp"
#include "linkage.hpp"

namespace bronko {

constexpr uint32_t kReadPileupMaxEnd = 255;   // BK_READ_PILEUP_MAX_END

// bk_read_pileup_cell: the rows over one cell by the base they carry there (A C G T = 0 1 2 3): strand 0, strand 1, and of both the
// rows that have the cell within end_dist positions of one of their ends
struct ReadPileupCell {
    uint32_t fwd[4] = {}, rev[4] = {}, near[4] = {};
};
static_assert(sizeof(ReadPileupCell) == 48, "ReadPileupCell is bk_read_pileup_cell");
struct ReadPileupParams {
    uint32_t max_mismatches = 8, end_dist = 10;
};
struct ReadPileupStats {
    uint64_t covered = 0, bases = 0;     // cells with at least one row, the sum of all fwd and rev counters
};

// One cell per position of genome file `file`, in the order of its sequences.  Throws for end_dist above kReadPileupMaxEnd and for a
// row that does not lie inside the file's cells.
std::vector<ReadPileupCell> read_pileup_count(const Index& ix, int file, const std::vector<LinkRow>& rows, uint32_t end_dist);

// OUT/<stem>.read_pileup.tsv: two ##read_pileup_* lines, the column line -- write_pileup_tsv's eleven columns, then near_A .. near_T --
// and one line per position of every sequence, zero-cover positions included.  cells: read_pileup_count's or the engine's.
ReadPileupStats write_read_pileup_tsv(const std::string& out_path, const Index& ix, int file, const std::vector<ReadPileupCell>& cells, const ReadPileupParams& p);

}  // namespace bronko
