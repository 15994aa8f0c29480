// cohort.cpp -- see cohort.hpp
#include "cohort.hpp"

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <thread>

namespace bronko {
namespace {

// fn(begin, end) over [0, n) on up to `threads` threads
template <class F>
void over_threads(uint64_t n, unsigned threads, F fn) {
    const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::max(1u, threads), n));
    if (nt == 1) { fn((uint64_t)0, n); return; }
    std::vector<std::thread> th;
    const uint64_t per = (n + nt - 1) / nt;
    for (unsigned i = 0; i < nt; i++) {
        const uint64_t b = std::min(n, i * per), e = std::min(n, b + per);
        if (b < e) th.emplace_back([&fn, b, e] { fn(b, e); });
    }
    for (auto& t : th) t.join();
}

// one row against the columns [0, n): the hardware's population count where the target has one
#if defined(__x86_64__)
__attribute__((target("popcnt")))
#endif
void row_against_all(const CohortPlanes& p, uint64_t i, uint32_t* diff, uint32_t* compared) {
    const uint64_t W = p.W;
    const uint64_t *vi = p.valid.data() + i * W, *b0i = p.b0.data() + i * W, *b1i = p.b1.data() + i * W;
    for (uint64_t j = 0; j < p.n; j++) {
        const uint64_t *vj = p.valid.data() + j * W, *b0j = p.b0.data() + j * W, *b1j = p.b1.data() + j * W;
        uint64_t cmp = 0, dif = 0;
        for (uint64_t w = 0; w < W; w++) {
            const uint64_t c = vi[w] & vj[w];
            const uint64_t d = c & ((b0i[w] ^ b0j[w]) | (b1i[w] ^ b1j[w]));
            cmp += (uint64_t)__builtin_popcountll(c);
            dif += (uint64_t)__builtin_popcountll(d);
        }
        if (compared) compared[j] = (uint32_t)cmp;
        if (diff) diff[j] = (uint32_t)dif;
    }
}

}  // namespace

CohortPlanes cohort_pack_host(const uint8_t* letters, uint64_t n, uint64_t positions, unsigned threads) {
    CohortPlanes p;
    p.n = n; p.positions = positions; p.W = (positions + 63) / 64;
    p.valid.assign((size_t)(n * p.W), 0); p.b0.assign((size_t)(n * p.W), 0); p.b1.assign((size_t)(n * p.W), 0);
    over_threads(n, threads, [&](uint64_t s0, uint64_t s1) {
        for (uint64_t s = s0; s < s1; s++) {
            const uint8_t* row = letters + s * positions;
            for (uint64_t pos = 0; pos < positions; pos++) {
                const uint8_t ch = row[pos];
                const uint64_t code = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
                if (code > 3) continue;
                const size_t at = (size_t)(s * p.W + pos / 64);
                const uint64_t bit = 1ull << (pos % 64);
                p.valid[at] |= bit;
                if (code & 1) p.b0[at] |= bit;
                if (code & 2) p.b1[at] |= bit;
            }
        }
    });
    return p;
}

void cohort_distances_host(const CohortPlanes& p, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared, unsigned threads) {
    if (row0 > p.n || n_rows > p.n - row0) throw std::runtime_error("cohort_distances_host: the rows lie beyond the cohort");
    over_threads(n_rows, threads, [&](uint64_t r0, uint64_t r1) {
        for (uint64_t r = r0; r < r1; r++) row_against_all(p, row0 + r, diff ? diff + r * p.n : nullptr, compared ? compared + r * p.n : nullptr);
    });
}

void cohort_distances_host(const uint8_t* letters, uint64_t n, uint64_t positions, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared,
                           unsigned threads) {
    cohort_distances_host(cohort_pack_host(letters, n, positions, threads), row0, n_rows, diff, compared, threads);
}

// ---- clusters -------------------------------------------------------------------------------------------------------------------
CohortClusterer::CohortClusterer(uint64_t n, uint64_t positions, uint64_t threshold, double min_breadth)
    : n_(n), positions_(positions), threshold_(threshold), min_breadth_(min_breadth), parent_((size_t)n) {
    std::iota(parent_.begin(), parent_.end(), 0u);
}

uint32_t CohortClusterer::find(uint32_t x) {
    while (parent_[x] != x) { parent_[x] = parent_[parent_[x]]; x = parent_[x]; }
    return x;
}

void CohortClusterer::add_rows(uint64_t row0, uint64_t n_rows, const uint32_t* diff, const uint32_t* compared) {
    const double need = min_breadth_ * (double)positions_;
    for (uint64_t r = 0; r < n_rows; r++) {
        const uint64_t i = row0 + r;
        for (uint64_t j = 0; j < n_; j++) {
            if (j == i || (uint64_t)diff[r * n_ + j] > threshold_ || !((double)compared[r * n_ + j] >= need)) continue;
            const uint32_t a = find((uint32_t)i), b = find((uint32_t)j);
            if (a != b) parent_[std::max(a, b)] = std::min(a, b);   // (the root is the component's first sample)
        }
    }
}

CohortClusters CohortClusterer::finish() {
    CohortClusters c;
    c.cluster.assign((size_t)n_, 0); c.size.assign((size_t)n_, 0);
    std::vector<uint32_t> number((size_t)n_, 0), count((size_t)n_, 0);
    for (uint64_t i = 0; i < n_; i++) {   // (in input order: a component is numbered when its first sample, its root, comes by)
        const uint32_t r = find((uint32_t)i);
        if (r == i) number[r] = ++c.n_clusters;
        count[r]++;
    }
    for (uint64_t i = 0; i < n_; i++) {
        const uint32_t r = find((uint32_t)i);
        c.cluster[i] = number[r]; c.size[i] = count[r];
        c.largest = std::max(c.largest, count[r]);
    }
    return c;
}

// ---- writers --------------------------------------------------------------------------------------------------------------------
CohortMatrixWriter::CohortMatrixWriter(const std::string& path, const std::vector<std::string>& names) : path_(path), names_(names) {
    f_ = fopen(path.c_str(), "wb");
    if (!f_) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to create distance matrix file " + path);
    std::string head = "sample";
    for (const auto& s : names_) { head += '\t'; head += s; }
    head += '\n';
    fwrite(head.data(), 1, head.size(), f_);
}

CohortMatrixWriter::~CohortMatrixWriter() { if (f_) fclose(f_); }

void CohortMatrixWriter::add_rows(uint64_t row0, uint64_t n_rows, const uint32_t* values) {
    if (!f_ || row0 != next_ || n_rows > names_.size() - row0) throw std::runtime_error("CohortMatrixWriter: rows out of order for " + path_);
    const size_t n = names_.size();
    std::string line;
    for (uint64_t r = 0; r < n_rows; r++) {
        line = names_[(size_t)(row0 + r)];
        char buf[16];
        for (size_t j = 0; j < n; j++) {
            const int len = snprintf(buf, sizeof buf, "\t%u", values[r * n + j]);
            line.append(buf, (size_t)len);
        }
        line += '\n';
        if (fwrite(line.data(), 1, line.size(), f_) != line.size()) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to write " + path_);
    }
    next_ = row0 + n_rows;
}

void CohortMatrixWriter::close() {
    if (!f_) return;
    FILE* f = f_;
    f_ = nullptr;
    if (fclose(f) != 0) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to write " + path_);
    if (next_ != names_.size()) throw std::runtime_error("CohortMatrixWriter: " + path_ + " was closed before its last row");
}

void write_cohort_distances_tsv(const std::string& path, const std::vector<std::string>& names, const uint32_t* diff) {
    CohortMatrixWriter w(path, names);
    if (!names.empty()) w.add_rows(0, names.size(), diff);
    w.close();
}

void write_cohort_compared_tsv(const std::string& path, const std::vector<std::string>& names, const uint32_t* compared) {
    write_cohort_distances_tsv(path, names, compared);
}

void write_cohort_clusters_tsv(const std::string& path, const std::vector<std::string>& names, const CohortClusters& c, uint64_t threshold, double min_breadth) {
    if (c.cluster.size() != names.size() || c.size.size() != names.size()) throw std::runtime_error("write_cohort_clusters_tsv: one cluster per sample");
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to create clusters file " + path);
    fprintf(f, "##cluster_threshold=%llu\n##cluster_min_breadth=%g\nsample\tcluster\tsize\n", (unsigned long long)threshold, min_breadth);
    for (size_t i = 0; i < names.size(); i++) fprintf(f, "%s\t%u\t%u\n", names[i].c_str(), c.cluster[i], c.size[i]);
    if (fclose(f) != 0) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to write " + path);
}

}  // namespace bronko
