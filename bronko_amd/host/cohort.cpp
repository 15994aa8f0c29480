// cohort.cpp -- see cohort.hpp
#include "cohort.hpp"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
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

// The same split of [0, n) run again and again on threads that stay: a step of cohort_mst_host is one row, too short to start
// threads for.  run(fn) returns when fn(begin, end) has returned for every part; the caller's thread takes the first part.
class RangePool {
public:
    RangePool(uint64_t n, unsigned threads) {
        const unsigned nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::max(1u, threads), n));
        const uint64_t per = nt ? (n + nt - 1) / nt : 0;
        for (unsigned i = 0; i < nt; i++) {
            const uint64_t b = std::min(n, i * per), e = std::min(n, b + per);
            if (i == 0) { b0_ = b; e0_ = e; }
            else if (b < e) workers_.emplace_back([this, b, e] { work(b, e); });
        }
    }
    ~RangePool() {
        { std::lock_guard<std::mutex> g(m_); stop_ = true; }
        start_.notify_all();
        for (auto& t : workers_) t.join();
    }
    RangePool(const RangePool&) = delete;
    RangePool& operator=(const RangePool&) = delete;
    void run(const std::function<void(uint64_t, uint64_t)>& fn) {
        { std::lock_guard<std::mutex> g(m_); fn_ = &fn; pending_ = workers_.size(); generation_++; }
        start_.notify_all();
        if (b0_ < e0_) fn(b0_, e0_);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
    }
private:
    void work(uint64_t b, uint64_t e) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(uint64_t, uint64_t)>* fn;
            {
                std::unique_lock<std::mutex> g(m_);
                start_.wait(g, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_; fn = fn_;
            }
            (*fn)(b, e);
            { std::lock_guard<std::mutex> g(m_); pending_--; }
            done_.notify_one();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable start_, done_;
    const std::function<void(uint64_t, uint64_t)>* fn_ = nullptr;
    uint64_t generation_ = 0, b0_ = 0, e0_ = 0;
    size_t pending_ = 0;
    bool stop_ = false;
};

// one row against the columns [j0, j1): the hardware's population count where the target has one
#if defined(__x86_64__)
__attribute__((target("popcnt")))
#endif
void row_against_columns(const CohortPlanes& p, uint64_t i, uint64_t j0, uint64_t j1, uint32_t* diff, uint32_t* compared) {
    const uint64_t W = p.W;
    const uint64_t *vi = p.valid.data() + i * W, *b0i = p.b0.data() + i * W, *b1i = p.b1.data() + i * W;
    for (uint64_t j = j0; j < j1; j++) {
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
void row_against_all(const CohortPlanes& p, uint64_t i, uint32_t* diff, uint32_t* compared) { row_against_columns(p, i, 0, p.n, diff, compared); }

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

// ---- the minimum spanning forest --------------------------------------------------------------------------------------------------
uint32_t cohort_min_compared(double min_breadth, uint64_t positions) {
    const double need = min_breadth * (double)positions;
    if (!(need > 0.0)) return 0;
    if (need >= 4294967295.0) return 0xffffffffu;
    return (uint32_t)std::ceil(need);       // (an integer below 2^32 is exact as a double: (double)c >= need iff c >= ceil(need))
}

CohortMst cohort_mst_host(const CohortPlanes& p, uint32_t min_compared, unsigned threads) {
    const uint64_t n = p.n;
    const uint32_t need = std::max<uint32_t>(1, min_compared);
    CohortMst m;
    m.nearest.assign((size_t)n, CohortMstNearest{kCohortNone, 0, 0});
    std::vector<uint32_t> diff((size_t)n), cmp((size_t)n);
    // per sample outside the tree its least edge into the tree, under (diff, lo, hi); lo = kCohortNone: none yet
    std::vector<CohortMstEdge> best((size_t)n, CohortMstEdge{kCohortNone, kCohortNone, 0, 0});
    std::vector<uint8_t> in_tree((size_t)n, 0);
    auto less = [](const CohortMstEdge& x, const CohortMstEdge& y) {
        return x.diff != y.diff ? x.diff < y.diff : x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi;
    };
    RangePool pool(n, threads);             // (the columns of a row, split once)
    uint64_t u = 0;
    const std::function<void(uint64_t, uint64_t)> row = [&](uint64_t j0, uint64_t j1) { row_against_columns(p, u, j0, j1, diff.data(), cmp.data()); };
    for (uint64_t first = 0; first < n; first++) {
        if (in_tree[first]) continue;
        u = first;                 // (a component's tree grows from its first sample)
        for (;;) {
            in_tree[u] = 1;
            pool.run(row);
            for (uint64_t j = 0; j < n; j++) {
                if (j == u || cmp[j] < need) continue;
                CohortMstNearest& nr = m.nearest[u];
                if (nr.sample == kCohortNone || diff[j] < nr.diff) nr = CohortMstNearest{(uint32_t)j, diff[j], cmp[j]};   // (ascending j: the first of equals stays)
                if (in_tree[j]) continue;
                const CohortMstEdge e{(uint32_t)std::min(u, j), (uint32_t)std::max(u, j), diff[j], cmp[j]};
                if (best[j].lo == kCohortNone || less(e, best[j])) best[j] = e;
            }
            uint64_t next = n;
            for (uint64_t j = 0; j < n; j++)
                if (!in_tree[j] && best[j].lo != kCohortNone && (next == n || less(best[j], best[next]))) next = j;
            if (next == n) break;           // (nothing admissible leaves the tree: the component is whole)
            m.edges.push_back(best[next]);
            u = next;
        }
    }
    std::sort(m.edges.begin(), m.edges.end(), less);
    return m;
}

CohortForest root_forest(uint64_t n, const std::vector<CohortMstEdge>& edges) {
    CohortForest f;
    f.parent.assign((size_t)n, kCohortNone); f.diff.assign((size_t)n, 0); f.compared.assign((size_t)n, 0);
    f.component.assign((size_t)n, 0); f.size.assign((size_t)n, 0);
    std::vector<uint32_t> start((size_t)n + 1, 0), adj(2 * edges.size());   // the neighbours of a sample: the edges' indices
    for (const auto& e : edges) {
        if (e.lo >= e.hi || e.hi >= n) throw std::runtime_error("root_forest: an edge's samples must be lo < hi < n");
        start[e.lo + 1]++; start[e.hi + 1]++;
        f.longest = std::max(f.longest, e.diff);
    }
    for (uint64_t i = 0; i < n; i++) start[i + 1] += start[i];
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (size_t k = 0; k < edges.size(); k++) { adj[fill[edges[k].lo]++] = (uint32_t)k; adj[fill[edges[k].hi]++] = (uint32_t)k; }
    std::vector<uint32_t> todo, members;
    for (uint64_t root = 0; root < n; root++) {
        if (f.component[root]) continue;    // (in input order: an unreached sample is its component's smallest)
        const uint32_t number = ++f.n_components;
        f.component[root] = number;
        todo.assign(1, (uint32_t)root); members.clear();
        while (!todo.empty()) {
            const uint32_t i = todo.back();
            todo.pop_back();
            members.push_back(i);
            for (uint32_t k = start[i]; k < start[i + 1]; k++) {
                const CohortMstEdge& e = edges[adj[k]];
                const uint32_t j = e.lo == i ? e.hi : e.lo;
                if (j == f.parent[i]) continue;
                if (f.component[j]) throw std::runtime_error("root_forest: the edges hold a cycle");
                f.component[j] = number; f.parent[j] = i; f.diff[j] = e.diff; f.compared[j] = e.compared;
                todo.push_back(j);
            }
        }
        for (uint32_t i : members) f.size[i] = (uint32_t)members.size();
        f.largest = std::max<uint32_t>(f.largest, (uint32_t)members.size());
    }
    return f;
}

void write_cohort_mst_tsv(const std::string& path, const std::vector<std::string>& names, const CohortForest& f, const std::vector<CohortMstNearest>& nearest,
                          double min_breadth, uint32_t min_compared) {
    const size_t n = names.size();
    if (f.parent.size() != n || f.diff.size() != n || f.compared.size() != n || f.component.size() != n || f.size.size() != n || nearest.size() != n)
        throw std::runtime_error("write_cohort_mst_tsv: one line per sample");
    FILE* file = fopen(path.c_str(), "wb");
    if (!file) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to create spanning forest file " + path);
    fprintf(file, "##mst_min_breadth=%g\n##mst_min_compared=%u\nsample\tparent\tdiff\tcompared\tcomponent\tsize\tnearest\tnearest_diff\tnearest_compared\n", min_breadth, min_compared);
    for (size_t i = 0; i < n; i++) {
        fprintf(file, "%s\t", names[i].c_str());
        if (f.parent[i] == kCohortNone) fputs(".\t.\t.", file);
        else if (f.parent[i] < n) fprintf(file, "%s\t%u\t%u", names[f.parent[i]].c_str(), f.diff[i], f.compared[i]);
        else { fclose(file); throw std::runtime_error("write_cohort_mst_tsv: a parent beyond the samples"); }
        fprintf(file, "\t%u\t%u\t", f.component[i], f.size[i]);
        if (nearest[i].sample == kCohortNone) fputs(".\t.\t.\n", file);
        else if (nearest[i].sample < n) fprintf(file, "%s\t%u\t%u\n", names[nearest[i].sample].c_str(), nearest[i].diff, nearest[i].compared);
        else { fclose(file); throw std::runtime_error("write_cohort_mst_tsv: a nearest neighbour beyond the samples"); }
    }
    if (fclose(file) != 0) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to write " + path);
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

// ---- --contamination --------------------------------------------------------------------------------------------------------------
MinorSummary minor_mask_host(const uint64_t* fwd, const uint64_t* rev, uint64_t positions, uint64_t min_reads, double min_freq, uint8_t* masks) {
    MinorSummary s;
    s.positions = positions;
    for (uint64_t p = 0; p < positions; p++) {
        uint64_t tot[4], depth = 0;
        for (int b = 0; b < 4; b++) { tot[b] = fwd[p * 4 + b] + rev[p * 4 + b]; depth += tot[b]; }
        const double need = min_freq * (double)depth;
        unsigned mask = 0;
        for (int b = 0; b < 4; b++)
            if (tot[b] >= min_reads && (double)tot[b] >= need) mask |= 1u << b;
        s.mixed += (mask & (mask - 1)) != 0;
        s.present += (uint64_t)__builtin_popcount(mask);
        if (masks) masks[p] = (uint8_t)mask;
    }
    return s;
}

namespace {
// one recipient row against all columns: M_X of the row, C_X of the columns made of their three planes
#if defined(__x86_64__)
__attribute__((target("popcnt")))
#endif
void explained_row(const CohortPlanes& p, const std::vector<uint64_t>& minor, uint64_t i, uint32_t* explained) {
    const uint64_t W = p.W;
    const uint64_t* m = minor.data() + i * 4 * W;   // [A C G T][W]
    for (uint64_t j = 0; j < p.n; j++) {
        const uint64_t *vj = p.valid.data() + j * W, *b0j = p.b0.data() + j * W, *b1j = p.b1.data() + j * W;
        uint64_t ex = 0;
        for (uint64_t w = 0; w < W; w++) {
            const uint64_t v = vj[w], b0 = b0j[w], b1 = b1j[w];
            ex += (uint64_t)__builtin_popcountll((m[w] & v & ~b0 & ~b1) | (m[W + w] & v & b0 & ~b1) | (m[2 * W + w] & v & ~b0 & b1) | (m[3 * W + w] & v & b0 & b1));
        }
        explained[j] = (uint32_t)ex;
    }
}
}  // namespace

void cohort_explained_host(const uint8_t* letters, const uint8_t* masks, uint64_t n, uint64_t positions, uint64_t row0, uint64_t n_rows, uint32_t* explained,
                           uint32_t* minor_sites, unsigned threads) {
    if (row0 > n || n_rows > n - row0) throw std::runtime_error("cohort_explained_host: the rows lie beyond the cohort");
    const CohortPlanes p = cohort_pack_host(letters, n, positions, threads);
    const uint64_t W = p.W;
    std::vector<uint64_t> minor((size_t)(n_rows * 4 * W), 0);   // of the block's rows only
    over_threads(n_rows, threads, [&](uint64_t r0, uint64_t r1) {
        for (uint64_t r = r0; r < r1; r++) {
            const uint64_t s = row0 + r;
            uint64_t sites = 0;
            for (uint64_t pos = 0; pos < positions; pos++) {
                const size_t at = (size_t)(s * W + pos / 64);
                const uint64_t bit = 1ull << (pos % 64);
                if (!(p.valid[at] & bit)) continue;
                const unsigned code = (p.b0[at] & bit ? 1u : 0u) | (p.b1[at] & bit ? 2u : 0u);
                const unsigned m = masks[s * positions + pos] & 15u & ~(1u << code);
                for (unsigned b = 0; b < 4; b++)
                    if (m >> b & 1u) minor[(size_t)((r * 4 + b) * W + pos / 64)] |= bit;
                sites += m != 0;
            }
            if (minor_sites) minor_sites[r] = (uint32_t)sites;
        }
    });
    if (!explained) return;
    over_threads(n_rows, threads, [&](uint64_t r0, uint64_t r1) {
        for (uint64_t r = r0; r < r1; r++) explained_row(p, minor, r, explained + r * n);
    });
}

ContaminationScanner::ContaminationScanner(uint64_t n, uint32_t min_sites, double min_share) : n_(n), min_sites_(min_sites), min_share_(min_share) {
    c_.best.assign((size_t)n, ContaminationBest{});
    c_.n_flagged.assign((size_t)n, 0);
}

void ContaminationScanner::add_rows(uint64_t row0, uint64_t n_rows, const uint32_t* diff, const uint32_t* compared, const uint32_t* explained) {
    if (row0 > n_ || n_rows > n_ - row0) throw std::runtime_error("ContaminationScanner: the rows lie beyond the cohort");
    for (uint64_t r = 0; r < n_rows; r++) {
        const uint64_t i = row0 + r;
        ContaminationBest& best = c_.best[i];
        for (uint64_t j = 0; j < n_; j++) {   // (ascending j: the earlier of equals stays)
            if (j == i) continue;
            const uint32_t ex = explained[r * n_ + j], d = diff[r * n_ + j];
            c_.largest = std::max(c_.largest, ex);
            if (ex >= 1 && (best.source == kCohortNone || ex > best.explained || (ex == best.explained && d < best.diff))) best = ContaminationBest{(uint32_t)j, ex, d};
            if (ex >= min_sites_ && (double)ex >= min_share_ * (double)d) {
                c_.flagged.push_back(ContaminationPair{(uint32_t)i, (uint32_t)j, d, compared[r * n_ + j], ex});
                c_.n_flagged[i]++;
            }
        }
    }
}

Contamination ContaminationScanner::finish() {
    std::sort(c_.flagged.begin(), c_.flagged.end(), [](const ContaminationPair& x, const ContaminationPair& y) {
        return x.recipient != y.recipient ? x.recipient < y.recipient : x.source < y.source;
    });
    c_.recipients = 0;
    for (uint32_t f : c_.n_flagged) c_.recipients += f != 0;
    return c_;
}

void write_cohort_explained_tsv(const std::string& path, const std::vector<std::string>& names, const uint32_t* explained) {
    write_cohort_distances_tsv(path, names, explained);
}

namespace {
// x / y with four decimals, truncated, from the integers (y > 0)
std::string ratio4(uint64_t x, uint64_t y) {
    char buf[48];
    snprintf(buf, sizeof buf, "%llu.%04llu", (unsigned long long)(x / y), (unsigned long long)(x % y * 10000 / y));
    return buf;
}
FILE* open_contamination_file(const std::string& path, const char* what, const ContaminationParams& p) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to create " + what + " file " + path);
    fprintf(f, "##minor_min_reads=%llu\n##minor_min_freq=%g\n##contamination_min_sites=%u\n##contamination_min_share=%g\n", (unsigned long long)p.minor_min_reads,
            p.minor_min_freq, p.min_sites, p.min_share);
    return f;
}
}  // namespace

void write_contamination_tsv(const std::string& path, const std::vector<std::string>& names, const Contamination& c, const std::vector<uint32_t>& minor_sites,
                             const ContaminationParams& p) {
    const size_t n = names.size();
    if (minor_sites.size() != n) throw std::runtime_error("write_contamination_tsv: one minor_sites per sample");
    for (const auto& x : c.flagged)
        if (x.recipient >= n || x.source >= n || x.diff == 0 || minor_sites[x.recipient] == 0)
            throw std::runtime_error("write_contamination_tsv: a flagged pair beyond the samples, or without a difference or a minor site");
    FILE* f = open_contamination_file(path, "contamination", p);
    fputs("recipient\tsource\tdiff\tcompared\texplained\tshare\tminor_sites\tminor_share\n", f);
    for (const auto& x : c.flagged)
        fprintf(f, "%s\t%s\t%u\t%u\t%u\t%s\t%u\t%s\n", names[x.recipient].c_str(), names[x.source].c_str(), x.diff, x.compared, x.explained, ratio4(x.explained, x.diff).c_str(),
                minor_sites[x.recipient], ratio4(x.explained, minor_sites[x.recipient]).c_str());
    if (fclose(f) != 0) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to write " + path);
}

void write_mixture_tsv(const std::string& path, const std::vector<std::string>& names, const Contamination& c, const std::vector<uint32_t>& minor_sites,
                       const ContaminationParams& p) {
    const size_t n = names.size();
    if (minor_sites.size() != n || c.best.size() != n || c.n_flagged.size() != n) throw std::runtime_error("write_mixture_tsv: one line per sample");
    for (const auto& b : c.best)
        if (b.source != kCohortNone && (b.source >= n || b.diff == 0)) throw std::runtime_error("write_mixture_tsv: a best source beyond the samples, or without a difference");
    FILE* f = open_contamination_file(path, "mixture", p);
    fputs("sample\tminor_sites\tflagged\tbest_source\texplained\tdiff\tshare\n", f);
    for (size_t i = 0; i < n; i++) {
        const ContaminationBest& b = c.best[i];
        fprintf(f, "%s\t%u\t%u\t", names[i].c_str(), minor_sites[i], c.n_flagged[i]);
        if (b.source == kCohortNone) fputs(".\t.\t.\t.\n", f);
        else fprintf(f, "%s\t%u\t%u\t%s\n", names[b.source].c_str(), b.explained, b.diff, ratio4(b.explained, b.diff).c_str());
    }
    if (fclose(f) != 0) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to write " + path);
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
