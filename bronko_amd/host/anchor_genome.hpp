// anchor_genome.hpp -- one genome file as the host twins of the engine's anchor passes see it, and how they all read a record: the
// file's letters, where its sequences start, its anchor k-mers; the records of the reads; the anchors at a record's two ends; the
// record turned along the reference.  Used by linkage.cpp and, with event_twin.hpp, by the twins of the six event passes (indels.cpp,
// junctions.cpp, copybacks.cpp, duplications.cpp, chimeras.cpp, breakends.cpp).  The rule is include/bronko_hip.h's (bk_indels_enable).
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "file_cells.hpp"
#include "lcb.hpp"

namespace bronko {

inline bool is_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
inline char comp(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }

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
    // the cells [lo, hi) lie in sequence s and hold letters ACGT
    bool holds_acgt(size_t s, int64_t lo, int64_t hi) const {
        if (lo < first[s] || hi > first[s + 1]) return false;
        for (int64_t c = lo; c < hi; c++) if (!is_acgt(text[(size_t)c])) return false;
        return true;
    }
};

// The records of the reads, in their order: a read upper-cased and cut at every letter that is not ACGT, the runs of at least k letters
template <class F>
void for_each_record(const std::vector<std::string>& reads, int k, F each) {
    std::string run;
    for (const std::string& read : reads) {
        run.clear();
        for (size_t i = 0; i <= read.size(); i++) {
            const char c = i < read.size() ? (char)(read[i] >= 'a' && read[i] <= 'z' ? read[i] - 32 : read[i]) : 'N';
            if (is_acgt(c)) { run.push_back(c); continue; }
            if ((int)run.size() >= k) each(run);
            run.clear();
        }
    }
}

// The anchors at a record's two ends (n >= k): the first anchor k-mer at the offsets 0, 8, 16, 24 and at n - k, n - k - 8, ..
struct EndAnchors {
    int f_off = -1, b_off = -1;                      // the offsets; -1: none
    uint32_t f_cell = 0, b_cell = 0;                 // the cells the k-mers start at
    bool f_ag = false, b_ag = false;                 // read against the reference
    bool both() const { return f_off >= 0 && b_off >= 0; }
};
inline EndAnchors end_anchors(const AnchorGenome& g, const std::string& rec) {
    const int k = g.k, n = (int)rec.size();
    EndAnchors e;
    for (int o = 0; o <= 24 && o + k <= n; o += 8)
        if (g.anchor(rec.data() + o, &e.f_cell, &e.f_ag)) { e.f_off = o; break; }
    for (int o = n - k; o >= n - k - 24 && o >= 0; o -= 8)
        if (g.anchor(rec.data() + o, &e.b_cell, &e.b_ag)) { e.b_off = o; break; }
    return e;
}

// r': the record along the reference
inline std::string along_reference(const std::string& rec, bool against) {
    if (!against) return rec;
    std::string r(rec.size(), 'A');
    for (size_t j = 0; j < rec.size(); j++) r[j] = comp(rec[rec.size() - 1 - j]);
    return r;
}

// A record with both anchors on one strand, along the reference: r', its anchors' offsets a and b (the lower cell's first) and their
// cells ca and cb.  Whether the anchors are apart (a + k <= b) is the pass's to ask.
struct Oriented {
    bool against;
    std::string r;
    int64_t a, b, ca, cb;
};
inline Oriented orient(const std::string& rec, int k, const EndAnchors& e) {
    const int64_t n = (int64_t)rec.size();
    if (e.f_ag) return Oriented{true, along_reference(rec, true), n - k - e.b_off, n - k - e.f_off, e.b_cell, e.f_cell};
    return Oriented{false, rec, e.f_off, e.b_off, e.f_cell, e.b_cell};
}

}  // namespace bronko
