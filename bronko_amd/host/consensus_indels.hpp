// consensus_indels.hpp -- `bronko call --consensus-indels`: the host twin of the engine's step that applies a sample's indels to its
// consensus (bk_consensus_indels.hip), and the writers of OUT/<stem>.consensus.fa with the indels in it and of
// OUT/<stem>.consensus_indels.tsv.  The rule is stated in include/bronko_hip.h (bk_sample_consensus_indels) and DESIGN.md section
// CI; this file restates it in plain C++ over the host indel twin's events and span array, so that the CPU tests can hold it against
// the Python restatement (tests/consensus_indels_ref.py) and the GPU tests the engine against both.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "indels.hpp"

namespace bronko {

// One accepted event, as bk_consensus_indel_record: cell, len and seq as IndelEvent has them, support = fwd + rev, ref_span =
// span[cell], applied = 1, or 0 for a contested one
struct ConsensusIndel {
    uint32_t cell = 0;
    int32_t len = 0;
    uint32_t support = 0, ref_span = 0;
    uint64_t seq = 0;
    uint32_t applied = 0, pad = 0;
};
// bk_consensus_indel_summary's tallies
struct ConsensusIndelTallies {
    uint64_t candidates = 0, accepted = 0, applied = 0, contested = 0, deletions = 0, insertions = 0, deleted_bases = 0, inserted_bases = 0, frameshifts = 0;
};
struct ConsensusIndels {
    std::vector<ConsensusIndel> events;   // the accepted events, sorted by (cell, deletion before insertion, length, seq)
    ConsensusIndelTallies n;
};

// (cell, kind, length, seq): indel_event_less's order
bool consensus_indel_less(const ConsensusIndel& x, const ConsensusIndel& y);

// The events of genome file `file` (cells of the whole index, as indel_events gives them) against `span` (the prefix-summed span
// array of all cells) at min_depth and min_freq; `letters` (the genome file's n_letters consensus letters) get '-' at the applied
// deletions.
ConsensusIndels consensus_indels(const Index& ix, int file, const std::vector<IndelEvent>& events, const std::vector<uint32_t>& span, uint64_t min_depth,
                                 double min_freq, uint8_t* letters, uint64_t n_letters);

// OUT/<stem>.consensus.fa of the edited letters: write_consensus_fasta's headers; per sequence its letters without the '-' and every
// applied insertion's S in front of its cell, in lines of 60 after the edit
void write_consensus_indels_fasta(const std::string& out_path, const std::string& stem, const Index& ix, int file, const uint8_t* letters, uint64_t n,
                                  const std::vector<ConsensusIndel>& events);

// OUT/<stem>.consensus_indels.tsv: the two parameter lines, the column line, one line per accepted event (sorted here)
void write_consensus_indels_tsv(const std::string& out_path, const Index& ix, int file, std::vector<ConsensusIndel> events, uint64_t min_depth, double min_freq);

}  // namespace bronko
