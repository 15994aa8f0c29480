// contamination_sanitize.cpp -- the host side of --contamination under AddressSanitizer and UBSan, as a program of its own
// (tools/contamination_sanitize.py builds and runs it): minor_mask_host over a pileup made of the masks, cohort_explained_host on 1 and
// 16 threads and in row blocks, the scanner fed blocks of BLOCK rows, and the three writers, over a cohort read from two files.
//   contamination_sanitize LETTERS MASKS N POSITIONS BLOCK MIN_SITES MIN_SHARE OUT_PREFIX     LETTERS, MASKS: N rows of POSITIONS bytes
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bronko_amd/host/cohort.hpp"

using namespace bronko;

static void fail(const std::string& what) { fprintf(stderr, "contamination_sanitize: %s\n", what.c_str()); exit(1); }

static std::vector<uint8_t> read_rows(const char* path, size_t bytes) {
    std::vector<uint8_t> v(bytes);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), 1, v.size(), f) != v.size()) fail(std::string("cannot read ") + path);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 9) fail("usage: contamination_sanitize LETTERS MASKS N POSITIONS BLOCK MIN_SITES MIN_SHARE OUT_PREFIX");
    const uint64_t n = strtoull(argv[3], nullptr, 10), positions = strtoull(argv[4], nullptr, 10), block = std::max<uint64_t>(1, strtoull(argv[5], nullptr, 10));
    ContaminationParams prm;
    prm.min_sites = (uint32_t)strtoull(argv[6], nullptr, 10);
    prm.min_share = strtod(argv[7], nullptr);
    const std::vector<uint8_t> letters = read_rows(argv[1], (size_t)(n * positions)), masks = read_rows(argv[2], (size_t)(n * positions));
    try {
        // a pileup whose present masks at R = 10, F = 0 are the low four bits of the first sample's bytes: the twin gives them back
        std::vector<uint64_t> fwd((size_t)(positions * 4)), rev((size_t)(positions * 4));
        for (uint64_t p = 0; p < positions; p++)
            for (int b = 0; b < 4; b++) { fwd[p * 4 + b] = masks[p] >> b & 1 ? 6 : 5; rev[p * 4 + b] = 4; }
        std::vector<uint8_t> back((size_t)positions);
        const MinorSummary ms = minor_mask_host(fwd.data(), rev.data(), positions, 10, 0.0, back.data());
        uint64_t present = 0;
        for (uint64_t p = 0; p < positions; p++) {
            if (back[p] != (masks[p] & 15)) fail("minor_mask_host does not give the masks back");
            present += (uint64_t)__builtin_popcount(back[p]);
        }
        if (ms.positions != positions || ms.present != present) fail("minor_mask_host: the tallies");

        std::vector<uint32_t> diff((size_t)(n * n)), cmp((size_t)(n * n)), ex((size_t)(n * n)), ex1((size_t)(n * n)), sites((size_t)n), sites1((size_t)n);
        cohort_distances_host(letters.data(), n, positions, 0, n, diff.data(), cmp.data(), 16);
        cohort_explained_host(letters.data(), masks.data(), n, positions, 0, n, ex.data(), sites.data(), 16);
        cohort_explained_host(letters.data(), masks.data(), n, positions, 0, n, ex1.data(), sites1.data(), 1);
        if (ex != ex1 || sites != sites1) fail("1 and 16 threads disagree");
        ContaminationScanner sc(n, prm.min_sites, prm.min_share);
        std::vector<uint32_t> bex((size_t)(block * n)), bsites((size_t)block);
        for (uint64_t r = 0; r < n; r += block) {   // (the blocks on their own, against the whole)
            const uint64_t rows = std::min(block, n - r);
            cohort_explained_host(letters.data(), masks.data(), n, positions, r, rows, bex.data(), bsites.data(), 3);
            if (!std::equal(bex.begin(), bex.begin() + (ptrdiff_t)(rows * n), ex.begin() + (ptrdiff_t)(r * n)) || !std::equal(bsites.begin(), bsites.begin() + (ptrdiff_t)rows, sites.begin() + (ptrdiff_t)r))
                fail("a row block differs from the whole");
            cohort_explained_host(letters.data(), masks.data(), n, positions, r, rows, nullptr, bsites.data(), 2);
            cohort_explained_host(letters.data(), masks.data(), n, positions, r, rows, bex.data(), nullptr, 2);
            sc.add_rows(r, rows, diff.data() + r * n, cmp.data() + r * n, bex.data());
        }
        const Contamination c = sc.finish();
        for (uint64_t i = 0; i < n; i++)
            for (uint64_t j = 0; j < n; j++)
                if (ex[i * n + j] > diff[i * n + j] || ex[i * n + j] > sites[i] || (i == j && ex[i * n + j])) fail("explained beyond diff or minor_sites, or on the diagonal");
        for (const auto& x : c.flagged)
            if (x.recipient == x.source || x.explained < prm.min_sites || !((double)x.explained >= prm.min_share * (double)x.diff)) fail("a flagged pair that is none");
        std::vector<std::string> names;
        for (uint64_t i = 0; i < n; i++) names.push_back("s" + std::to_string(i));
        const std::string out = argv[8];
        write_cohort_explained_tsv(out + ".explained.tsv", names, ex.data());
        write_contamination_tsv(out + ".contamination.tsv", names, c, sites, prm);
        write_mixture_tsv(out + ".mixture.tsv", names, c, sites, prm);
    } catch (const std::exception& e) { fail(e.what()); }
    return 0;
}
