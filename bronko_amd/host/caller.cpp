// caller.cpp -- see caller.hpp.
#include "caller.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>

#include "fastx.hpp"
#include "file_cells.hpp"
#include "lcb.hpp"

namespace bronko {

namespace {

// Student-t quantile StudentsT(0,1,n-2).inverse_cdf(1 - 0.001/n) for n = 3..300 (call.rs:922-925).  statrs
// is not vendored with the reference; the window never holds more than 300 values (call.rs:802,813), so the
// quantile is tabulated (oracle/gen_tcrit.py, exact to the last bit of the mathematical value).
const double kTCrit[298] = {
#include "tcrit_table.inc"
};

double thompson_tau(uint64_t n) {
    if (n <= 2) return INFINITY;                                   // call.rs:927-929
    const double t = (n <= 300) ? kTCrit[n - 3] : NAN;
    const double dn = (double)n;
    return (t * (dn - 1.0)) / (std::sqrt(dn) * std::sqrt(dn - 2.0 + t * t));   // call.rs:926
}

char base_char(unsigned b) { return b < 4 ? "ACGT"[b] : 'N'; }   // lcb.rs:57-65

// Rust `{:.N}` of an f64: correctly rounded decimal; "NaN" / "inf" / "-inf" for the specials.
std::string fixed(double v, int prec) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[512];
    snprintf(buf, sizeof buf, "%.*f", prec, v);
    return buf;
}

struct File {
    FILE* fp;
    explicit File(const std::string& path) : fp(fopen(path.c_str(), "w")) {}
    ~File() { if (fp) fclose(fp); }
};

}  // namespace

int pick_best_genome(const Index& ix, const std::vector<uint64_t>& stats, const std::vector<uint8_t>& present) {
    int best = -1;
    double best_score = 0.0;
    for (size_t f = 0; f < ix.files.size(); f++) {
        if (!present[f]) continue;                                  // no key in the mapping data
        const double score = (double)stats[f * 3] / (double)ix.genome_len(f) / 2.0;   // call.rs:435
        if (score > best_score) { best_score = score; best = (int)f; }                 // strict >, call.rs:443
    }
    return best;
}

std::vector<double> baseline_noise_max(const uint64_t* fwd4, const uint64_t* rev4, uint64_t len) {
    constexpr int kWindow = 100, kTop = kWindow / 10, kHalf = kWindow / 2;   // call.rs:802-804,824
    std::vector<double> out(len, 0.0);
    std::array<double, kWindow * 3> ring{};      // minor-allele frequencies currently in the window
    std::array<uint8_t, kWindow * 3> flagged{};  // "in_max" flag of each ring slot
    std::array<double, kTop> top{};              // the largest values, descending
    uint64_t n = 0;
    double s = 0.0, s2 = 0.0;

    for (uint64_t i = 0; i < len + kHalf; i++) {
        std::array<double, 4> freq{0.0, 0.0, 0.0, 0.0};
        if (i < len) {                                              // call.rs:831-845
            std::array<uint64_t, 4> cnt;
            for (int b = 0; b < 4; b++) cnt[b] = fwd4[i * 4 + b] + rev4[i * 4 + b];
            std::sort(cnt.begin(), cnt.end(), [](uint64_t a, uint64_t b) { return a > b; });
            const uint64_t depth = cnt[0] + cnt[1] + cnt[2] + cnt[3];
            if (depth != 0) for (int b = 0; b < 4; b++) freq[b] = (double)cnt[b] / (double)depth;
        }
        const size_t slot0 = (size_t)(i % kWindow) * 3;
        for (int r = 1; r < 4; r++) {                               // minor ranks 1..3, call.rs:848
            const size_t slot = slot0 + (size_t)(r - 1);
            const double old = ring[slot];
            if (old > 0.0) {                                        // evict, call.rs:853-870
                n -= 1; s -= old; s2 -= old * old;
                if (flagged[slot]) {
                    for (int q = 0; q < kTop; q++) {
                        if (std::fabs(top[q] - old) < 1e-12) {
                            for (int z = q; z + 1 < kTop; z++) top[z] = top[z + 1];
                            top[kTop - 1] = 0.0;
                            break;
                        }
                    }
                    flagged[slot] = 0;
                }
            }
            const double maf = freq[r];
            if (maf > 0.0) {                                        // insert, call.rs:873-890
                n += 1; s += maf; s2 += maf * maf;
                for (int q = kTop - 1; q >= 0; q--) {
                    if (!(maf > top[q])) break;
                    if (q + 1 < kTop) top[q + 1] = top[q];
                    top[q] = maf;
                }
                flagged[slot] = 1;                                  // set whether or not it entered the table
            } else {
                flagged[slot] = 0;
            }
            ring[slot] = maf;
        }

        double mu = 0.0, var = 0.0;
        if (n != 0) { mu = s / (double)n; var = s2 / (double)n - mu * mu; }   // population variance, call.rs:901-907
        int idx = 0;
        uint64_t cn = n;
        double cs = s, cs2 = s2;
        while (idx < kTop && top[idx] != 0.0) {                     // strip outliers, call.rs:917-950
            const double cand = top[idx];
            if (!(std::fabs(cand - mu) > thompson_tau(cn) * std::sqrt(var))) break;
            cs -= cand;
            cs2 -= cand;                                            // sic (call.rs:936): the value, not its square
            cn -= 1;
            if (cn > 0) { mu = cs / (double)cn; var = cs2 / (double)cn - mu * mu; }
            else { mu = 0.0; var = 0.0; }
            idx++;
        }
        if (i >= (uint64_t)kHalf && i - kHalf < len)                // call.rs:953-962
            out[i - kHalf] = idx < kTop ? top[idx] : 0.0;           // idx == kTop would index out of bounds upstream
    }
    return out;
}

double strand_odds(uint64_t fwd_ref, uint64_t rev_ref, uint64_t fwd_alt, uint64_t rev_alt, const CallParams& prm, bool* tested) {
    if (tested) *tested = false;
    double sor = prm.strand_odds_max + 1.0;
    if (!prm.no_strand_filter) {                                        // call.rs:1059-1096
        const double a = (double)fwd_ref + 1.0, b = (double)rev_ref + 1.0;
        const double c = (double)fwd_alt + 1.0, d = (double)rev_alt + 1.0;
        const double min_strand = std::fmin(a + c, b + d) / (a + b + c + d);
        if (!prm.no_strand_balance_filter || min_strand >= prm.strand_balance_ratio) {
            const double r = (a * d) / (b * c);
            sor = std::log(r + 1.0 / r) + std::log(std::fmin(a, b) / std::fmax(a, b))
                  - std::log(std::fmin(c, d) / std::fmax(c, d));
            if (tested) *tested = true;
        } else {
            sor = -1.0;
        }
    }
    return sor;
}

CallSummary call_variants(const Index& ix, int file_id, const Pileup& p, const CallParams& prm) {
    CallSummary out;
    uint64_t covered = 0, positions = 0, coverage = 0;
    uint64_t cell = 0;
    for (int f = 0; f < file_id; f++) cell += ix.genome_len(f);
    const FileMeta& fm = ix.files[file_id];
    for (size_t sid = 0; sid < fm.sequences.size(); sid++) {        // metadata order (upstream: DashMap order)
        const SeqMeta& sm = fm.sequences[sid];
        const uint64_t len = sm.len;
        const uint64_t* fd = p.fwd_depth.data() + cell * 4;
        const uint64_t* rd = p.rev_depth.data() + cell * 4;
        const uint64_t* fk = p.fwd_nk.data() + cell * 4;
        const uint64_t* rk = p.rev_nk.data() + cell * 4;
        const std::vector<double> noise = baseline_noise_max(fd, rd, len);          // call.rs:1002
        int64_t start = 0, end = (int64_t)len;
        if (!prm.no_end_filter) { start = prm.k; end = (int64_t)len - prm.k; }      // call.rs:1013-1016
        positions += len;
        for (int64_t i = start; i < end; i++) {
            const uint64_t* row = fd + i * 4;
            const uint64_t* rrow = rd + i * 4;
            const unsigned ref = nt_to_bits(sm.seq[i]);                             // non-ACGT counts as A
            uint64_t tot[4], depth = 0;
            for (int b = 0; b < 4; b++) { tot[b] = row[b] + rrow[b]; depth += tot[b]; }
            if (depth == 0) continue;
            covered += 1;
            coverage += depth;
            for (unsigned alt = 0; alt < 4; alt++) {
                if (alt == ref || tot[alt] == 0) continue;
                bool tested = false;
                const double sor = strand_odds(row[ref], rrow[ref], row[alt], rrow[alt], prm, &tested);
                if (tested) {
                    if (sor > prm.strand_odds_max) continue;
                    if (fk[i * 4 + alt] < prm.n_per_strand && rk[i * 4 + alt] < prm.n_per_strand) continue;
                }
                const double af = (double)tot[alt] / (double)depth;
                const double y0 = prm.variant_multiplier;
                const double factor = y0 + 0.5 * std::pow(0.03, 100.0 * af);        // call.rs:1102-1105
                if (af < prm.min_af || af < std::fmax(factor, y0) * noise[i]) continue;
                if (af >= 0.5) {
                    out.n_major += 1;
                } else {
                    if (depth < prm.min_depth) continue;
                    if (tot[alt] < prm.min_variant_depth) continue;
                    out.n_minor += 1;
                }
                out.records.push_back(VcfRecord{(int)sid, (uint64_t)i + 1, (uint8_t)ref, (uint8_t)alt, row[ref], rrow[ref],
                                                row[alt], rrow[alt], depth, af, sor});
            }
        }
        cell += len;
    }
    out.breadth = (double)covered / (double)positions;              // call.rs:1144
    out.depth = (double)coverage / (double)covered;                 // call.rs:1145 (NaN when nothing is covered)
    return out;
}

Consensus consensus(const Index& ix, int file_id, const Pileup& p, const ConsensusParams& prm) {
    static const char kLetter[] = "-ACMGRSVTWYHKDBN";              // by bit mask A = 1, C = 2, G = 4, T = 8
    Consensus out;
    uint64_t cell = 0;
    for (int f = 0; f < file_id; f++) cell += ix.genome_len(f);
    for (const SeqMeta& sm : ix.files[file_id].sequences) {
        for (uint64_t i = 0; i < sm.len; i++, cell++) {
            const uint64_t* fd = p.fwd_depth.data() + cell * 4;
            const uint64_t* rd = p.rev_depth.data() + cell * 4;
            std::array<std::pair<uint64_t, unsigned>, 4> by;        // (count, base code)
            uint64_t depth = 0;
            for (unsigned b = 0; b < 4; b++) { by[b] = {fd[b] + rd[b], b}; depth += by[b].first; }
            out.positions += 1;
            if (depth < prm.min_depth) { out.letters.push_back('N'); out.masked += 1; continue; }
            std::sort(by.begin(), by.end(), [](const auto& x, const auto& y) { return x.first != y.first ? x.first > y.first : x.second < y.second; });
            const double need = prm.min_freq * (double)depth;
            unsigned mask = 0;
            uint64_t cum = 0;
            size_t j = 0;
            do {                                                    // at least one base; a count of 0 is never taken
                mask |= 1u << by[j].second;
                cum += by[j].first;
                j++;
            } while (j < 4 && by[j].first != 0 && !((double)cum >= need));
            for (; j < 4 && by[j].first != 0 && by[j].first == by[j - 1].first; j++) mask |= 1u << by[j].second;   // ties with the last one taken
            out.letters.push_back(kLetter[mask]);
            if ((mask & (mask - 1)) == 0) {
                out.called += 1;
                if (mask != 1u << nt_to_bits(sm.seq[i])) out.substitutions += 1;   // non-ACGT counts as A
            } else {
                out.ambiguous += 1;
            }
        }
    }
    return out;
}

void write_consensus_fasta(const std::string& out_path, const std::string& stem, const Index& ix, int file_id, const uint8_t* letters, uint64_t n) {
    if (n != ix.genome_len((size_t)file_id)) throw std::runtime_error("write_consensus_fasta: the letters are not the genome's length");
    File f(out_path);
    if (!f.fp) throw std::runtime_error("Failed to create consensus fasta file " + out_path);
    uint64_t at = 0;
    for (const SeqMeta& sm : ix.files[file_id].sequences) {
        fprintf(f.fp, ">%s|%s\n", stem.c_str(), chrom_of(sm.name).c_str());
        for (uint64_t i = 0; i < sm.len; i += 60) {
            const size_t m = (size_t)std::min<uint64_t>(60, sm.len - i);
            if (fwrite(letters + at + i, 1, m, f.fp) != m || fputc('\n', f.fp) == EOF) throw std::runtime_error("Failed to write consensus fasta file " + out_path);
        }
        at += sm.len;
    }
}

// ---- --regions / --region-window -------------------------------------------------------------------------------------------
std::vector<BedLine> read_bed(const std::string& path) {
    std::vector<BedLine> out;
    GzLineReader in(path);
    std::string line;
    size_t no = 0;
    // a column that is a number: digits only, below 2^63
    auto number = [](const std::string& v, uint64_t* x) {
        if (v.empty() || v.size() > 18) return false;
        *x = 0;
        for (char c : v) { if (c < '0' || c > '9') return false; *x = *x * 10 + (uint64_t)(c - '0'); }
        return true;
    };
    while (in.next(line)) {
        no++;
        if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        const std::string where = path + ": line " + std::to_string(no);
        std::vector<std::string> col;
        for (size_t a = 0; col.size() < 6;) {
            const size_t b = line.find('\t', a);
            col.push_back(line.substr(a, b == std::string::npos ? b : b - a));
            if (b == std::string::npos) break;
            a = b + 1;
        }
        if (col.size() < 3) throw std::runtime_error(where + ": " + std::to_string(col.size()) + " tab-separated column(s), a BED line has at least chrom, start and end");
        BedLine r;
        r.chrom = col[0]; r.line = no;
        r.name = col.size() > 3 && !col[3].empty() ? col[3] : ".";
        if (col.size() > 5) r.strand = col[5];
        if (r.chrom.empty()) throw std::runtime_error(where + ": empty chrom column");
        if (!number(col[1], &r.start)) throw std::runtime_error(where + ": start '" + col[1] + "' is not a non-negative integer");
        if (!number(col[2], &r.end)) throw std::runtime_error(where + ": end '" + col[2] + "' is not a non-negative integer");
        if (r.start >= r.end) throw std::runtime_error(where + ": start " + col[1] + " is not below end " + col[2] + " (BED ranges are half-open and not empty)");
        if (out.size() == kMaxBedRegions) throw std::runtime_error(path + ": more than " + std::to_string(kMaxBedRegions) + " regions");
        out.push_back(std::move(r));
    }
    return out;
}

std::vector<Region> resolve_bed(const Index& ix, const std::vector<BedLine>& bed, const std::string& path) {
    std::map<std::string, std::vector<std::pair<int, uint32_t>>> where;   // CHROM token -> (file, sequence) in index order
    for (size_t f = 0; f < ix.files.size(); f++)
        for (size_t q = 0; q < ix.files[f].sequences.size(); q++) where[chrom_of(ix.files[f].sequences[q].name)].push_back({(int)f, (uint32_t)q});
    std::vector<Region> out;
    for (const BedLine& b : bed) {
        const std::string at = path + ": line " + std::to_string(b.line);
        const auto it = where.find(b.chrom);
        if (it == where.end()) throw std::runtime_error(at + ": chrom '" + b.chrom + "' is no sequence of any genome");
        for (const auto& fq : it->second) {
            const SeqMeta& sm = ix.files[(size_t)fq.first].sequences[fq.second];
            if (b.end > sm.len)
                throw std::runtime_error(at + ": end " + std::to_string(b.end) + " lies beyond sequence '" + b.chrom + "' of " + ix.files[(size_t)fq.first].name +
                                         " (length " + std::to_string(sm.len) + ")");
            Region r;
            r.file_id = fq.first; r.seq = fq.second; r.start = (uint32_t)b.start; r.end = (uint32_t)b.end; r.name = b.name;
            out.push_back(std::move(r));
        }
        if (out.size() > kMaxRegions) throw std::runtime_error(path + ": more than " + std::to_string(kMaxRegions) + " regions over all genomes");
    }
    return out;
}

std::vector<Region> window_regions(const Index& ix, uint64_t window) {
    if (window < 1) throw std::runtime_error("the region window must be at least 1");
    uint64_t n = 0;
    for (const FileMeta& fm : ix.files)
        for (const SeqMeta& sm : fm.sequences) n += (sm.len + window - 1) / window;
    if (n > kMaxRegions)
        throw std::runtime_error("--region-window " + std::to_string(window) + " makes " + std::to_string(n) + " windows, at most " + std::to_string(kMaxRegions) +
                                 " are supported: raise the window");
    std::vector<Region> out;
    out.reserve((size_t)n);
    for (size_t f = 0; f < ix.files.size(); f++)
        for (size_t q = 0; q < ix.files[f].sequences.size(); q++) {
            const uint64_t len = ix.files[f].sequences[q].len;
            for (uint64_t s = 0; s < len; s += window) {
                Region r;
                r.file_id = (int)f; r.seq = (uint32_t)q; r.start = (uint32_t)s; r.end = (uint32_t)std::min(s + window, len); r.name = ".";
                out.push_back(std::move(r));
            }
        }
    return out;
}

RegionReport region_depths(const Index& ix, int file_id, const Pileup& p, const std::vector<Region>& regions, uint64_t min_depth) {
    RegionReport out;
    if (file_id < 0) return out;
    uint64_t file_cell = 0;
    for (int f = 0; f < file_id; f++) file_cell += ix.genome_len((size_t)f);
    for (const Region& r : regions) {
        if (r.file_id != file_id) continue;
        uint64_t cell = file_cell;
        for (uint32_t q = 0; q < r.seq; q++) cell += ix.files[(size_t)file_id].sequences[q].len;
        std::vector<uint64_t> d;
        for (uint64_t i = r.start; i < r.end; i++) {
            uint64_t depth = 0;
            for (unsigned b = 0; b < 4; b++) depth += p.fwd_depth[(cell + i) * 4 + b] + p.rev_depth[(cell + i) * 4 + b];
            d.push_back(depth);
        }
        const uint64_t L = d.size();
        RegionDepth o;
        for (uint64_t v : d) { o.sum += v; if (v >= min_depth) o.covered += 1; }
        std::sort(d.begin(), d.end());
        o.min = d.front(); o.max = d.back(); o.median = d[(size_t)((L - 1) / 2)];
        out.rows.push_back(o);
        if (o.covered == L) out.full += 1; else if (o.covered == 0) out.empty += 1; else out.partial += 1;
    }
    return out;
}

void write_regions_tsv(const std::string& out_path, const Index& ix, int file_id, const std::vector<Region>& regions,
                       const RegionDepth* rows, uint64_t n_rows, uint64_t min_depth) {
    File f(out_path);
    if (!f.fp) throw std::runtime_error("Failed to create regions file " + out_path);
    fprintf(f.fp, "##min_depth=%llu\nchrom\tstart\tend\tname\tlength\tmean\tmin\tmedian\tmax\tcovered\n", (unsigned long long)min_depth);
    uint64_t at = 0;
    for (const Region& r : regions) {
        if (file_id < 0 || r.file_id != file_id) continue;
        if (at == n_rows) throw std::runtime_error("write_regions_tsv: fewer rows than the genome has regions");
        const RegionDepth& o = rows[at++];
        const uint64_t L = (uint64_t)r.end - r.start;
        const unsigned __int128 m = (unsigned __int128)o.sum * 100u / L;   // (100 * sum leaves u64 above 1.8e17)
        fprintf(f.fp, "%s\t%u\t%u\t%s\t%llu\t%llu.%02u\t%llu\t%llu\t%llu\t%llu\n", chrom_of(ix.files[(size_t)file_id].sequences[r.seq].name).c_str(), r.start, r.end,
                r.name.c_str(), (unsigned long long)L, (unsigned long long)(m / 100u), (unsigned)(m % 100u), (unsigned long long)o.min,
                (unsigned long long)o.median, (unsigned long long)o.max, (unsigned long long)o.covered);
    }
    if (at != n_rows) throw std::runtime_error("write_regions_tsv: more rows than the genome has regions");
    if (fflush(f.fp) != 0 || ferror(f.fp)) throw std::runtime_error("Failed to write regions file " + out_path);
}

std::string clean_sample_id(const std::string& path) {
    static const char* const kSuffixes[] = {".fastq.gz", ".fasta.gz", "fna.gz", "fnq.gz", ".fq.gz", ".fastq",
                                            ".fasta", ".fnq", ".fna", ".fa", ".fq"};
    const size_t slash = path.find_last_of('/');
    std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    auto ends_with = [](const std::string& s, const std::string& suf) {
        return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
    };
    for (const char* suf : kSuffixes) {
        if (ends_with(name, suf)) {
            const std::string sfx(suf);
            while (ends_with(name, sfx)) name.resize(name.size() - sfx.size());    // trim_end_matches
            return name;
        }
    }
    const size_t dot = name.find_last_of('.');
    if (dot != std::string::npos && dot != 0) name.resize(dot);
    return name;
}

// --keep-kmer-info (call.rs:1202-1211): one "KMER\tCOUNT\n" line per entry, in the order given (the engine's: ascending k-mer).
// Pieces of the table are formatted on `threads` threads, a piece at a time per thread, and written in order.
void write_kmer_counts(const std::string& out_path, int k, const uint64_t* kmers, const uint64_t* counts, uint64_t n, int threads) {
    if (k < 1 || k > 32) throw std::runtime_error("write_kmer_counts: k out of range");
    File f(out_path);
    if (!f.fp) throw std::runtime_error("Failed to create k-mer count file " + out_path);
    const unsigned nt = (unsigned)std::max(1, threads);
    const uint64_t piece = 1u << 16;   // entries per piece (about 2 MB of text at k = 21)
    const uint64_t n_pieces = (n + piece - 1) / piece;
    auto format = [&](uint64_t p, std::string& out) {
        const uint64_t i0 = p * piece, i1 = std::min(n, i0 + piece);
        out.resize((size_t)(i1 - i0) * ((size_t)k + 22));
        char* q = &out[0];
        for (uint64_t i = i0; i < i1; i++) {
            const uint64_t v = kmers[i];
            for (int j = 0; j < k; j++) *q++ = "ACGT"[(v >> (2 * (k - 1 - j))) & 3];
            *q++ = '\t';
            char d[24];
            int nd = 0;
            uint64_t c = counts[i];
            do { d[nd++] = (char)('0' + c % 10); c /= 10; } while (c);
            while (nd) *q++ = d[--nd];
            *q++ = '\n';
        }
        out.resize((size_t)(q - &out[0]));
    };
    // rounds of nt pieces: formatted side by side, written one after the other
    std::vector<std::string> buf(nt);
    for (uint64_t p0 = 0; p0 < n_pieces; p0 += nt) {
        const unsigned m = (unsigned)std::min<uint64_t>(nt, n_pieces - p0);
        if (m == 1) format(p0, buf[0]);
        else {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < m; t++) th.emplace_back([&, t] { format(p0 + t, buf[t]); });
            for (auto& t : th) t.join();
        }
        for (unsigned t = 0; t < m; t++)
            if (fwrite(buf[t].data(), 1, buf[t].size(), f.fp) != buf[t].size()) throw std::runtime_error("Failed to write k-mer count file " + out_path);
    }
}

void write_vcf(const std::string& out_path, const std::string& reads_path, const Index& ix, int file_id, const std::vector<VcfRecord>& recs) {
    File f(out_path);
    if (!f.fp) throw std::runtime_error("Failed to create vcf output file");
    const FileMeta& fm = ix.files[file_id];
    fprintf(f.fp, "##fileformat=VCFv4.5\n##source=bronko-v0.1.0\n##reference=file://%s\n", reads_path.c_str());
    for (const auto& s : fm.sequences)
        fprintf(f.fp, "##contig=<ID=%s,length=%llu>\n", chrom_of(s.name).c_str(), (unsigned long long)s.len);
    fputs("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Total Depth\">\n"
          "##INFO=<ID=AF,Number=1,Type=Float,Description=\"Allele Frequency\">\n"
          "##INFO=<ID=DP4,Number=4,Type=Integer,Description=\"Fwd_ref,Rev_ref,Fwd_alt,Rev_alt\">\n"
          "##INFO=<ID=SOR,Number=4,Type=Float,Description=\"SOR\">\n"
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", f.fp);
    for (const VcfRecord& v : recs)
        fprintf(f.fp, "%s\t%llu\t.\t%c\t%c\t.\tPASS\tDP=%llu;AF=%s;DP4=%llu,%llu,%llu,%llu;SOR=%s\n",
                chrom_of(fm.sequences[v.seq_id].name).c_str(), (unsigned long long)v.pos, base_char(v.ref_base),
                base_char(v.alt_base), (unsigned long long)v.depth, fixed(v.af, 3).c_str(), (unsigned long long)v.fwd_ref,
                (unsigned long long)v.rev_ref, (unsigned long long)v.fwd_alt, (unsigned long long)v.rev_alt, fixed(v.sor, 3).c_str());
}

void write_pileup_tsv(const std::string& out_path, const Index& ix, int file_id, const Pileup& p) {
    File f(out_path);
    if (!f.fp) throw std::runtime_error("Failed to create tsv pileup file");
    fputs("reference\tindex\tref\tA\tC\tG\tT\ta\tc\tg\tt\n", f.fp);
    uint64_t cell = 0;
    for (int g = 0; g < file_id; g++) cell += ix.genome_len(g);
    for (const auto& s : ix.files[file_id].sequences) {
        for (uint64_t i = 0; i < s.len; i++, cell++) {
            const uint64_t* a = p.fwd_depth.data() + cell * 4;
            const uint64_t* b = p.rev_depth.data() + cell * 4;
            fprintf(f.fp, "%s\t%llu\t%c\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", s.name.c_str(),
                    (unsigned long long)(i + 1), (char)s.seq[i], (unsigned long long)a[0], (unsigned long long)a[1],
                    (unsigned long long)a[2], (unsigned long long)a[3], (unsigned long long)b[0], (unsigned long long)b[1],
                    (unsigned long long)b[2], (unsigned long long)b[3]);
        }
    }
}

void write_overview_tsv(const std::string& out_path, const std::vector<OverviewRow>& rows) {
    File f(out_path);
    if (!f.fp) throw std::runtime_error("Failed to create tsv file");
    fputs("filename\tselected_genome\tnum_major_variants\tnum_minor_variants\tbreadth_coverage\tdepth_coverage\t"
          "num_perfect_kmers\tnum_variant_kmers\tnum_unmapped_kmers\n", f.fp);
    for (const auto& r : rows)
        fprintf(f.fp, "%s\t%s\t%llu\t%llu\t%s\t%s\t%llu\t%llu\t%llu\n", r.filename.c_str(), r.selected_genome.c_str(),
                (unsigned long long)r.n_major, (unsigned long long)r.n_minor, fixed(r.breadth, 4).c_str(), fixed(r.depth, 4).c_str(),
                (unsigned long long)r.n_perfect, (unsigned long long)r.n_variant, (unsigned long long)r.n_unmapped);
}

void write_alignments(const std::string& out_dir, const Index& ix, const std::vector<SampleCalls>& samples,
                      void (*note)(const std::string&)) {
    for (size_t g = 0; g < ix.files.size(); g++) {
        const FileMeta& fm = ix.files[g];
        std::vector<const SampleCalls*> group;
        for (const SampleCalls& sc : samples) {
            if (sc.selected_genome != fm.name) continue;
            if (sc.breadth < 0.90) {                                                    // call.rs:520-523
                if (note) note("Skipping " + sc.filename + " (breadth of coverage = " + std::to_string(sc.breadth) + ")");
                continue;
            }
            group.push_back(&sc);
        }
        if (group.empty()) continue;
        if (group.size() < 3) {                                                         // call.rs:540-543
            if (note) note("Skipping " + fm.name + " (only " + std::to_string(group.size()) + " samples)");
            continue;
        }
        if (note) note("Building alignment for genome " + fm.name + " with " + std::to_string(group.size()) + " samples");
        // every (sequence name, position) with a major variant in some sample -> its reference base (call.rs:570-582)
        std::map<std::pair<std::string, uint64_t>, uint8_t> columns;
        std::vector<std::map<std::pair<std::string, uint64_t>, uint8_t>> own(group.size());
        for (size_t i = 0; i < group.size(); i++)
            for (const VcfRecord& r : group[i]->records) {
                if (!(r.af >= 0.5)) continue;
                const std::pair<std::string, uint64_t> key(fm.sequences[(size_t)r.seq_id].name, r.pos);
                columns[key] = r.ref_base;
                own[i][key] = r.alt_base;
            }
        const std::string path = out_dir + "/" + fm.name + ".mfa";
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) throw std::runtime_error(std::string(strerror(errno)) + " | Failed to create mfa alignment file");
        std::string row;
        for (const auto& kv : columns) row.push_back(base_char(kv.second));            // std::map iterates in (name, position) order
        fprintf(f, ">%s\n%s\n", fm.name.c_str(), row.c_str());
        for (size_t i = 0; i < group.size(); i++) {
            row.clear();
            for (const auto& kv : columns) {
                const auto it = own[i].find(kv.first);
                row.push_back(base_char(it != own[i].end() ? it->second : kv.second));
            }
            fprintf(f, ">%s\n%s\n", clean_sample_id(group[i]->filename).c_str(), row.c_str());
        }
        fclose(f);
    }
}

}  // namespace bronko
