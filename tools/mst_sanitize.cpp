// mst_sanitize.cpp -- the host side of --mst under AddressSanitizer and UBSan, as a program of its own (tools/mst_sanitize.py
// builds and runs it): cohort_pack_host, cohort_mst_host on 1 and 16 threads, root_forest and write_cohort_mst_tsv over a cohort
// read from a file, and an independent check of what they return: the edges ascend in the edge order, join what they should and
// leave no admissible pair between two components.
//   mst_sanitize LETTERS N POSITIONS MIN_COMPARED OUT.tsv      LETTERS: N rows of POSITIONS bytes
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "../bronko_amd/host/cohort.hpp"

using namespace bronko;

static void fail(const std::string& what) { fprintf(stderr, "mst_sanitize: %s\n", what.c_str()); exit(1); }

int main(int argc, char** argv) {
    if (argc != 6) fail("usage: mst_sanitize LETTERS N POSITIONS MIN_COMPARED OUT.tsv");
    const uint64_t n = strtoull(argv[2], nullptr, 10), positions = strtoull(argv[3], nullptr, 10);
    const uint32_t min_compared = (uint32_t)strtoull(argv[4], nullptr, 10);
    std::vector<uint8_t> letters((size_t)(n * positions));
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(letters.data(), 1, letters.size(), f) != letters.size()) fail("cannot read the letters");
    fclose(f);
    try {
        const CohortPlanes p = cohort_pack_host(letters.data(), n, positions, 3);
        const CohortMst one = cohort_mst_host(p, min_compared, 1), m = cohort_mst_host(p, min_compared, 16);
        if (one.edges.size() != m.edges.size() || one.nearest.size() != n || m.nearest.size() != n) fail("1 and 16 threads disagree on the sizes");
        for (size_t k = 0; k < m.edges.size(); k++)
            if (one.edges[k].lo != m.edges[k].lo || one.edges[k].hi != m.edges[k].hi || one.edges[k].diff != m.edges[k].diff || one.edges[k].compared != m.edges[k].compared)
                fail("1 and 16 threads disagree on an edge");
        for (size_t i = 0; i < n; i++)
            if (one.nearest[i].sample != m.nearest[i].sample || one.nearest[i].diff != m.nearest[i].diff || one.nearest[i].compared != m.nearest[i].compared)
                fail("1 and 16 threads disagree on a nearest neighbour");
        const CohortForest forest = root_forest(n, m.edges);
        // the matrix, for the check only
        std::vector<uint32_t> diff((size_t)(n * n)), cmp((size_t)(n * n));
        cohort_distances_host(p, 0, n, diff.data(), cmp.data(), 16);
        const uint32_t need = min_compared > 1 ? min_compared : 1;
        for (size_t k = 0; k < m.edges.size(); k++) {
            const CohortMstEdge& e = m.edges[k];
            if (e.lo >= e.hi || e.hi >= n || e.diff != diff[e.lo * n + e.hi] || e.compared != cmp[e.lo * n + e.hi] || e.compared < need) fail("an edge that is none");
            if (forest.component[e.lo] != forest.component[e.hi]) fail("an edge across two components");
            if (k > 0) {
                const CohortMstEdge& b = m.edges[k - 1];
                if (!(b.diff < e.diff || (b.diff == e.diff && (b.lo < e.lo || (b.lo == e.lo && b.hi < e.hi))))) fail("the edges do not ascend");
            }
        }
        uint64_t roots = 0;
        for (uint64_t i = 0; i < n; i++) {
            roots += forest.parent[i] == kCohortNone;
            for (uint64_t j = 0; j < n; j++) {
                const bool adm = i != j && cmp[i * n + j] >= need;
                if (adm && forest.component[i] != forest.component[j]) fail("an admissible pair between two components");
                if (adm && (m.nearest[i].sample == kCohortNone || diff[i * n + j] < m.nearest[i].diff || (diff[i * n + j] == m.nearest[i].diff && j < m.nearest[i].sample)))
                    fail("a nearer neighbour than the nearest");
            }
        }
        if (roots != forest.n_components || m.edges.size() + roots != n) fail("edges + components != samples");
        std::vector<std::string> names;
        for (uint64_t i = 0; i < n; i++) names.push_back("s" + std::to_string(i));
        write_cohort_mst_tsv(argv[5], names, forest, m.nearest, 0.5, min_compared);
        bool threw = false;
        try { root_forest(2, {CohortMstEdge{1, 2, 0, 1}}); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) fail("root_forest took an edge beyond the samples");
        printf("mst_sanitize: n = %llu, positions = %llu, min_compared = %u: %zu edges, %u components, longest edge %u\n", (unsigned long long)n,
               (unsigned long long)positions, min_compared, m.edges.size(), forest.n_components, forest.longest);
    } catch (const std::exception& ex) { fail(ex.what()); }
    return 0;
}
