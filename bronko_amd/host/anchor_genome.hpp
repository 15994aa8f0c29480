// anchor_genome.hpp -- one genome file as the host twins of the engine's anchor passes see it (indels.cpp, linkage.cpp): its letters,
// where its sequences start, its anchor k-mers.  The rule is include/bronko_hip.h's (bk_indels_enable).
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "file_cells.hpp"
#include "lcb.hpp"

namespace bronko {

// One genome file as the rule sees it: its cells and where its sequences start (FileCells), its anchor k-mers
struct AnchorGenome : FileCells {
    int k = 0;
    struct Anchor { uint64_t kmer; uint32_t cell; bool rc; };
    std::vector<Anchor> anchors;                     // canonical k-mers that start at exactly one cell, sorted

    AnchorGenome(const Index& ix, int file) : FileCells(ix, file), k(ix.k) {
        std::vector<Anchor> all;
        const std::vector<SeqMeta>& seqs = ix.files[(size_t)file].sequences;
        for (size_t q = 0; q < seqs.size(); q++)    // the genome's k-mers as the index reads them: every letter that is not ACGT stands for A (nt_to_bits)
            for (uint64_t i = 0; i + (uint64_t)k <= seqs[q].seq.size(); i++) {
                const Canon cn = canonical_kmer(seqs[q].seq.data() + i, k);
                all.push_back(Anchor{cn.kmer, (uint32_t)(first[q] + (int64_t)i), cn.rc});
            }
        std::sort(all.begin(), all.end(), [](const Anchor& x, const Anchor& y) { return x.kmer < y.kmer; });
        for (size_t i = 0; i < all.size();) {
            size_t j = i + 1;
            while (j < all.size() && all[j].kmer == all[i].kmer) j++;
            if (j == i + 1) anchors.push_back(all[i]);
            i = j;
        }
    }
    bool anchor(const char* kmer, uint32_t* cell, bool* against) const {
        const Canon cn = canonical_kmer(reinterpret_cast<const uint8_t*>(kmer), k);
        const auto it = std::lower_bound(anchors.begin(), anchors.end(), cn.kmer, [](const Anchor& a, uint64_t v) { return a.kmer < v; });
        if (it == anchors.end() || it->kmer != cn.kmer) return false;
        *cell = it->cell; *against = cn.rc != it->rc;
        return true;
    }
    int seq_of(int64_t cell) const {
        int s = 0;
        while (s + 2 < (int)first.size() && first[(size_t)s + 1] <= cell) s++;
        return s;
    }
};

inline bool is_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
inline char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

}  // namespace bronko
