// anchor_genome.hpp -- one genome file as the host twins of the engine's anchor passes see it (indels.cpp, linkage.cpp): its letters,
// where its sequences start, its anchor k-mers.  The rule is include/bronko_hip.h's (bk_indels_enable).
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "index.hpp"
#include "lcb.hpp"

namespace bronko {

// One genome file as the rule sees it: its letters upper-cased, where its sequences start, its anchor k-mers
struct AnchorGenome {
    int k = 0;
    int64_t cell0 = 0;                               // first cell of the file among all cells of the index
    std::string text;                                // the file's cells (upper-cased FASTA letters)
    std::vector<int64_t> first;                      // first cell of each sequence, relative to cell0; one more entry: the end
    struct Anchor { uint64_t kmer; uint32_t cell; bool rc; };
    std::vector<Anchor> anchors;                     // canonical k-mers that start at exactly one cell, sorted

    AnchorGenome(const Index& ix, int file) : k(ix.k) {
        if (file < 0 || (size_t)file >= ix.files.size()) throw std::runtime_error("no such genome file");
        for (int f = 0; f < file; f++) cell0 += (int64_t)ix.genome_len((size_t)f);
        std::vector<Anchor> all;
        for (const SeqMeta& s : ix.files[(size_t)file].sequences) {
            const int64_t c0 = (int64_t)text.size();
            first.push_back(c0);
            for (uint8_t c : s.seq) text.push_back((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
            // the genome's k-mers as the index reads them: every letter that is not ACGT stands for A (nt_to_bits)
            for (uint64_t i = 0; i + (uint64_t)k <= s.seq.size(); i++) {
                const Canon cn = canonical_kmer(s.seq.data() + i, k);
                all.push_back(Anchor{cn.kmer, (uint32_t)(c0 + (int64_t)i), cn.rc});
            }
        }
        first.push_back((int64_t)text.size());
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
