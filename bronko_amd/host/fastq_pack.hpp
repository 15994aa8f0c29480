// fastq_pack.hpp -- one FASTQ(.gz) file -> batches of 2-bit packed records (include/bronko_hip.h: the layout bk_push_reads_packed
// takes), parsed and packed on several threads: what `bronko call` feeds an engine from (round 6).
//
// The reference hands its FASTQ files to KMC, which reads them with `-t` threads (call.rs:1166-1181).  Until round 6 a file's text --
// inflated on several threads by pargz.hpp -- went through ONE line loop per file (14 M reads/s) into batches of sequence lines that
// the engine packed on the device (bk_push_reads_ascii: 110 M reads/s over PCIe).  Here the text's pieces (a few MB each, as
// pargz.hpp's waves deliver them, or slices of a mapped plain file) are taken apart where they are:
//   stage A (a thread per piece)   the positions of the piece's line ends
//   in order (one thread)          the number of the piece's first line -- a FASTQ record is four lines, the sequence is line 1
//                                  mod 4 (the rule of the line loop it replaces, fastx.hpp / needletail's FASTQ reader) -- and the
//                                  piece of a line that the pieces before it left over
//   stage B (a thread per piece)   its sequence lines 2-bit packed (bk_pack_reads: KMC's splitting at non-ACGT symbols, runs
//                                  shorter than k dropped) into one PackedBatch
// and delivered in file order.  Inputs that cannot be mapped (a FIFO, /dev/fd/N) or a single thread keep the line loop; the
// batches are the same records either way (tests/test_fastq_pack.py).
#pragma once
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bronko_hip.h"
#include "fastx.hpp"
#include "pargz.hpp"

namespace bronko {

struct PackedBatch {
    std::vector<uint32_t> words;   // [n_records][stride]
    std::vector<uint16_t> lens;    // [n_records]
    std::vector<uint8_t> ends;     // [n_records] end flags (bk_push_reads_packed_ends), filled only for a reader asked for them (--primers, --adapter)
    uint32_t stride = 0;
    uint64_t n_records = 0, n_reads = 0;   // records packed; sequence lines seen (a read with an N is several records, a short one none)
    size_t bytes() const { return words.size() * 4 + lens.size() * 2 + ends.size(); }
    void clear() { words.clear(); lens.clear(); ends.clear(); stride = 0; n_records = 0; n_reads = 0; }
};

// 2-bit code of a sequence symbol (A C G T, either case), 4 = anything else (KMC splits a read there)
struct AcgtLut {
    uint8_t c[256];
    AcgtLut() { memset(c, 4, sizeof c); c['A'] = c['a'] = 0; c['C'] = c['c'] = 1; c['G'] = c['g'] = 2; c['T'] = c['t'] = 3; }
};
inline const AcgtLut& acgt_lut() { static const AcgtLut l; return l; }

// The sequence lines `ptr[i]` (length `len[i]`) packed into `out` (overwritten): the records bk_pack_reads makes of them, in the same
// order (include/bronko_hip.h: one record per maximal ACGT run of at least k symbols, runs longer than a record cut into chunks
// that overlap by k - 1).  A line that is one run and fits a record -- nearly every line -- takes the short way: sixteen table
// look-ups a word, no branch per symbol (the byte-at-a-time packer of the C ABI made 1 us a read of it: with the text inflated
// on 32 threads the packing was the slower half).
// kQual (--min-base-qual): qual[i] is line i's quality line (same length); a symbol whose quality byte is below thr is an N.
// want_ends (--primers): out.ends holds every record's end flags -- bit 0: its run starts the line, bit 1: its run ends the line; the
// chunks of a run that was cut carry neither.
template <bool kQual>
inline void pack_lines_t(const std::vector<const uint8_t*>& ptr, const std::vector<uint64_t>& len, int k, PackedBatch& out,
                         const std::vector<const uint8_t*>* qual, uint8_t thr, bool want_ends = false) {
    out.clear();
    out.n_reads = ptr.size();
    uint64_t longest = (uint64_t)k;
    for (uint64_t l : len) longest = std::max(longest, l);
    const uint32_t stride = (uint32_t)std::min<uint64_t>((longest + 15) / 16, 4095);   // (the engine's own rule for a batch of sequence lines: bk_push_reads_ascii)
    out.stride = stride;
    const uint64_t maxb = std::min<uint64_t>((uint64_t)stride * 16, 65535);
    const uint8_t* const lut = acgt_lut().c;
    out.words.resize((ptr.size() + 16) * (size_t)stride);
    out.lens.resize(ptr.size() + 16);
    if (want_ends) out.ends.resize(out.lens.size());
    uint64_t n = 0;
    auto room = [&]() {
        if (n == out.lens.size()) {
            out.lens.resize(n + n / 2 + 64); out.words.resize(out.lens.size() * (size_t)stride);
            if (want_ends) out.ends.resize(out.lens.size());
        }
    };
    auto emit = [&](const uint8_t* s, uint64_t l, uint8_t flags) {   // one record of l <= maxb ACGT symbols
        room();
        if (want_ends) out.ends[n] = flags;
        uint32_t* w = out.words.data() + n * stride;
        uint64_t i = 0;
        for (uint32_t wi = 0; wi < stride; wi++) {
            uint32_t x = 0;
            const uint64_t e = std::min<uint64_t>(l, i + 16);
            for (uint32_t sh = 0; i < e; i++, sh += 2) x |= (uint32_t)lut[s[i]] << sh;
            w[wi] = x;
        }
        out.lens[n++] = (uint16_t)l;
    };
    for (size_t r = 0; r < ptr.size(); r++) {
        const uint8_t* s = ptr[r];
        const uint8_t* q = kQual ? (*qual)[r] : nullptr;
        const uint64_t l = len[r];
        if (l >= (uint64_t)k && l <= maxb) {
            // the short way: packed as if it were one run, sixteen symbols a word; "anything else" shows in bit 2 of a code
            room();
            uint32_t* w = out.words.data() + n * stride;
            uint32_t bad = 0;
            uint64_t i = 0;
            uint32_t wi = 0;
            for (; i + 16 <= l; i += 16, wi++) {
                uint32_t x = 0, y = 0;
                for (uint32_t j = 0; j < 16; j++) { const uint32_t c = lut[s[i + j]]; y |= c; x |= (c & 3u) << (2 * j); }
                if (kQual) for (uint32_t j = 0; j < 16; j++) y |= (uint32_t)(q[i + j] < thr) << 2;   // (a masked symbol: "anything else")
                w[wi] = x; bad |= y;
            }
            if (i < l) {
                uint32_t x = 0, y = 0;
                for (uint32_t j = 0; i + j < l; j++) { const uint32_t c = lut[s[i + j]]; y |= c; x |= (c & 3u) << (2 * j); }
                if (kQual) for (uint32_t j = 0; i + j < l; j++) y |= (uint32_t)(q[i + j] < thr) << 2;
                w[wi++] = x; bad |= y;
            }
            if (!(bad & 4u)) {
                for (; wi < stride; wi++) w[wi] = 0u;
                if (want_ends) out.ends[n] = 3;
                out.lens[n++] = (uint16_t)l;
                continue;
            }
        }
        // the long way: run by run (what the C ABI's packer does)
        uint64_t start = 0;
        for (uint64_t i = 0; i <= l; i++) {
            if (i == l || lut[s[i]] > 3 || (kQual && q[i] < thr)) {
                const uint64_t rl = i - start;
                if (rl >= (uint64_t)k) {
                    const uint8_t flags = rl <= maxb ? (uint8_t)((start == 0 ? 1 : 0) | (i == l ? 2 : 0)) : (uint8_t)0;
                    uint64_t pos = 0;
                    for (;;) {
                        const uint64_t take = std::min(maxb, rl - pos);
                        emit(s + start + pos, take, flags);
                        if (pos + take >= rl) break;
                        pos += take - (uint64_t)(k - 1);      // next chunk re-reads k-1 bases: no k-mer lost or doubled
                    }
                }
                start = i + 1;
            }
        }
    }
    out.n_records = n;
    out.words.resize((size_t)n * stride);
    out.lens.resize((size_t)n);
    if (want_ends) out.ends.resize((size_t)n);
}

inline void pack_lines(const std::vector<const uint8_t*>& ptr, const std::vector<uint64_t>& len, int k, PackedBatch& out, bool want_ends = false) {
    pack_lines_t<false>(ptr, len, k, out, nullptr, 0, want_ends);
}
// The same with quality lines: min_qual > 0 packs the lines with every symbol whose quality byte is below '!' + min_qual
// (Phred+33) replaced by N; 0 ignores `qual`.
inline void pack_lines(const std::vector<const uint8_t*>& ptr, const std::vector<uint64_t>& len, int k, PackedBatch& out,
                       const std::vector<const uint8_t*>& qual, int min_qual, bool want_ends = false) {
    if (min_qual < 0 || min_qual > 93) throw std::invalid_argument("min_qual must be between 0 and 93 (Phred+33)");
    if (min_qual > 0) pack_lines_t<true>(ptr, len, k, out, &qual, (uint8_t)('!' + min_qual), want_ends);
    else pack_lines_t<false>(ptr, len, k, out, nullptr, 0, want_ends);
}

class FastqPacker {
public:
    // threads: parse / pack threads (and, for gzip input, as many inflate threads again: they take turns); min_qual > 0
    // (--min-base-qual): every base whose quality byte is below '!' + min_qual is packed as an N (pack_lines), and a quality line
    // that is not as long as its sequence line is an error; want_ends (--primers): the batches carry their records' end flags
    FastqPacker(const std::string& path, int k, unsigned threads, int min_qual = 0, bool want_ends = false)
        : path_(path), k_(k), threads_(std::max(1u, threads)), min_qual_(min_qual), want_ends_(want_ends) {
        if (min_qual < 0 || min_qual > 93) throw std::invalid_argument("min_qual must be between 0 and 93 (Phred+33)");
        struct stat st;
        const bool regular = ::stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0;
        if (threads_ > 1 && regular) {
            if (ParallelGunzip::is_gzip(path)) gz_.reset(new ParallelGunzip(path, std::min(threads_, 32u)));   // (a file's inflate gains nothing past 32 threads)
            else if (!looks_gzip(path)) map_plain(st.st_size);
        }
        if (gz_ || plain_) {
            // (taking the text apart and packing it is a tenth of inflating it -- 0.1 us against 1 us a read --: a few workers keep
            // up with any number of inflate threads, and sixty-four of them only queue up at the one lock)
            const unsigned n_workers = gz_ ? std::min(8u, std::max(2u, threads_ / 4)) : std::min(16u, threads_);
            for (unsigned t = 0; t < n_workers; t++) workers_.emplace_back([this] { work(); });
            feeder_ = std::thread([this] { feed(); });
            sequencer_ = std::thread([this] { sequence(); });
        } else {
            lines_.reset(new GzLineReader(path, 1));
        }
    }
    ~FastqPacker() {
        { std::unique_lock<std::mutex> lk(m_); quit_ = true; }
        cv_.notify_all();
        if (feeder_.joinable()) feeder_.join();
        if (sequencer_.joinable()) sequencer_.join();
        for (auto& w : workers_) if (w.joinable()) w.join();
        gz_.reset();
        if (plain_) munmap(const_cast<uint8_t*>(plain_), plain_n_);
        if (fd_ >= 0) ::close(fd_);
    }
    FastqPacker(const FastqPacker&) = delete;
    FastqPacker& operator=(const FastqPacker&) = delete;

    // The file's next batch; false at its end.  Throws std::runtime_error for a damaged or unreadable file.
    bool next(PackedBatch& out) {
        if (lines_) return next_serial(out);
        std::shared_ptr<Job> j;
        {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return !q2_.empty() || seq_done_; });
            if (q2_.empty()) {
                if (!error_.empty()) throw std::runtime_error(error_);
                return false;
            }
            j = q2_.front(); q2_.pop_front();
        }
        cv_.notify_all();
        j->done_b.get_future().wait();
        if (!j->error.empty()) throw std::runtime_error(j->error);
        std::swap(out, j->out);   // (the caller's old buffers stay with the reader)
        { std::unique_lock<std::mutex> lk(m_); spare_.push_back(std::move(j->out)); if (spare_.size() > 64) spare_.pop_front(); }
        return true;
    }

private:
    struct Job {
        pargz::Piece piece;                 // gzip input: the piece's own buffer
        const uint8_t* d = nullptr;         // the piece's text (the buffer above, or a slice of the mapped file)
        size_t n = 0;
        std::vector<uint32_t> nl;           // positions of its '\n'
        uint64_t line_base = 0;             // number of the line that its first '\n' ends
        std::string head;                   // what the pieces before it hold of that line (min_qual > 0: of that line's record, from
                                            // the record's first line on)
        bool last = false;                  // the text's end: what is left behind the last '\n' is a line too
        PackedBatch out;
        std::string error;
        std::promise<void> done_a, done_b;
    };
    static constexpr size_t kSlice = 4u << 20;   // a mapped plain file is taken in slices of this size
    static constexpr size_t kAheadJobs = 2;      // jobs in flight per thread (memory: a piece of a few MB each)

    static bool looks_gzip(const std::string& path) {   // (a file of fewer than three bytes, or unreadable: the line loop says what is wrong)
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return true;
        unsigned char h[2] = {0, 0};
        const ssize_t r = ::pread(fd, h, 2, 0);
        ::close(fd);
        return r < 2 || (h[0] == 0x1f && h[1] == 0x8b);
    }
    void map_plain(off_t size) {
        fd_ = ::open(path_.c_str(), O_RDONLY);
        if (fd_ < 0) return;
        void* m = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fd_, 0);
        if (m == MAP_FAILED) { ::close(fd_); fd_ = -1; return; }
        plain_ = static_cast<const uint8_t*>(m);
        plain_n_ = (size_t)size;
        madvise(m, plain_n_, MADV_SEQUENTIAL);
    }

    // ---- the worker pool -------------------------------------------------------------------------------------------------
    void submit(std::function<void()> f) {
        { std::unique_lock<std::mutex> lk(m_); tasks_.push_back(std::move(f)); }
        cv_.notify_all();
    }
    void work() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || !tasks_.empty(); });
                if (tasks_.empty()) return;   // (quit, nothing left)
                f = std::move(tasks_.front()); tasks_.pop_front();
            }
            f();
        }
    }

    // ---- stage A: the line ends of a piece ----------------------------------------------------------------------------------
    void stage_a(Job& j) {
        try {
            { std::unique_lock<std::mutex> lk(m_); if (!spare_nl_.empty()) { j.nl = std::move(spare_nl_.back()); spare_nl_.pop_back(); } }
            j.nl.clear();
            j.nl.reserve(j.n / 64 + 16);
            const uint8_t* p = j.d;
            const uint8_t* const end = j.d + j.n;
            while (p < end) {
                const uint8_t* q = static_cast<const uint8_t*>(memchr(p, '\n', (size_t)(end - p)));
                if (!q) break;
                j.nl.push_back((uint32_t)(q - j.d));
                p = q + 1;
            }
        } catch (const std::exception& e) { j.error = e.what(); }
        j.done_a.set_value();
    }
    // ---- stage B: the piece's sequence lines, packed ----------------------------------------------------------------------
    void stage_b(Job& j) {
        try {
            if (j.error.empty() && min_qual_ > 0) stage_b_records(j);
            else if (j.error.empty()) {
                static thread_local std::vector<const uint8_t*> ptr;   // (a worker's own: their memory is used again, piece after piece)
                static thread_local std::vector<uint64_t> len;
                ptr.clear(); len.clear();
                ptr.reserve(j.nl.size() / 4 + 2); len.reserve(j.nl.size() / 4 + 2);
                auto add = [&](const uint8_t* s, size_t n) {
                    while (n && s[n - 1] == '\r') n--;   // ("\r\n": the line loop strips it)
                    ptr.push_back(s); len.push_back(n);
                };
                std::string first;   // the line the pieces before this one began, whole
                size_t from = 0;
                for (size_t i = 0; i < j.nl.size(); i++) {
                    const size_t to = j.nl[i];
                    if (((j.line_base + i) & 3u) == 1u) {
                        if (i == 0 && !j.head.empty()) { first = j.head; first.append(reinterpret_cast<const char*>(j.d), to); add(reinterpret_cast<const uint8_t*>(first.data()), first.size()); }
                        else add(j.d + from, to - from);
                    }
                    from = to + 1;
                }
                std::string tail;   // the text's last line has no '\n'
                if (j.last && ((j.line_base + j.nl.size()) & 3u) == 1u) {
                    tail = j.nl.empty() ? j.head : std::string();
                    tail.append(reinterpret_cast<const char*>(j.d + from), j.n - from);
                    if (!tail.empty()) add(reinterpret_cast<const uint8_t*>(tail.data()), tail.size());
                }
                { std::unique_lock<std::mutex> lk(m_); if (!spare_.empty()) { j.out = std::move(spare_.back()); spare_.pop_back(); } }
                pack_lines(ptr, len, k_, j.out, want_ends_);
            }
        } catch (const std::exception& e) { j.error = e.what(); }
        j.piece = pargz::Piece();   // (its buffer goes back to the pool)
        { std::unique_lock<std::mutex> lk(m_); if (spare_nl_.size() < 256) spare_nl_.push_back(std::move(j.nl)); }
        j.done_b.set_value();
    }

    // ---- stage B with qualities (min_qual > 0): the records whose quality line ends in the piece --------------------------------
    // A record is lines 4r .. 4r + 3 (@id / sequence / + / quality).  The piece's head holds its first record's lines up to the
    // piece (sequence(): the carry is the unfinished record); every other record it finishes lies in the piece itself.  The text's
    // last piece also takes a last record that ends without a '\n' or is cut short (no quality line: an empty one).
    static const uint8_t* strip_cr(const uint8_t* s, size_t& n) { while (n && s[n - 1] == '\r') n--; return s; }
    void check_record(uint64_t rec_line, size_t seq_n, size_t qual_n) const {
        if (seq_n != qual_n)
            throw std::runtime_error(path_ + ": record " + std::to_string(rec_line / 4 + 1) + ": quality line of " + std::to_string(qual_n) +
                                     " bytes for a sequence of " + std::to_string(seq_n) + " (--min-base-qual)");
    }
    void stage_b_records(Job& j) {
        static thread_local std::vector<const uint8_t*> ptr, qptr;
        static thread_local std::vector<uint64_t> len;
        ptr.clear(); qptr.clear(); len.clear();
        ptr.reserve(j.nl.size() / 4 + 2); qptr.reserve(j.nl.size() / 4 + 2); len.reserve(j.nl.size() / 4 + 2);
        const uint64_t L = j.line_base, n = j.nl.size();
        // a record from its lines (ls[0..m), m <= 4; an absent quality line is an empty one)
        auto add = [&](uint64_t rec_line, const uint8_t* const* ls, const size_t* ln, size_t m) {
            if (m < 2) return;   // (no sequence line: nothing to pack, as without qualities)
            size_t sn = ln[1], qn = m > 3 ? ln[3] : 0;
            const uint8_t* sq = strip_cr(ls[1], sn);
            const uint8_t* qu = m > 3 ? strip_cr(ls[3], qn) : nullptr;
            check_record(rec_line, sn, qn);
            ptr.push_back(sq); qptr.push_back(qu); len.push_back(sn);
        };
        // text -> its first lines (what follows the last '\n' is a line if `open` -- the text was cut at a '\n' -- or not empty)
        auto split = [](const uint8_t* t, size_t tn, bool open, const uint8_t** ls, size_t* ln) {
            size_t m = 0, from = 0;
            for (size_t i = 0; i < tn && m < 4; i++)
                if (t[i] == '\n') { ls[m] = t + from; ln[m++] = i - from; from = i + 1; }
            if (m < 4 && (open || from < tn)) { ls[m] = t + from; ln[m++] = tn - from; }
            return m;
        };
        const uint8_t* ls[4]; size_t ln[4];
        std::string first, tail;
        uint64_t r = L & ~3ull;   // the first record the piece may finish
        if (r + 3 < L + n) {      // its quality line ends here: the head and the piece's text up to that '\n'
            first = j.head;
            first.append(reinterpret_cast<const char*>(j.d), j.nl[r + 3 - L]);
            add(r, ls, ln, split(reinterpret_cast<const uint8_t*>(first.data()), first.size(), true, ls, ln));   // (four lines)
            r += 4;
            for (; r + 3 < L + n; r += 4) {   // whole in the piece: line x (x > L) is [nl[x - L - 1] + 1, nl[x - L])
                for (size_t t = 0; t < 4; t++) {
                    const size_t i = (size_t)(r + t - L), from = j.nl[i - 1] + 1;
                    ls[t] = j.d + from; ln[t] = j.nl[i] - from;
                }
                add(r, ls, ln, 4);
            }
        }
        if (j.last) {   // what is left: the text's last record, unfinished or without its final '\n'
            const uint8_t* t; size_t tn;
            if (r == (L & ~3ull)) { tail = j.head; tail.append(reinterpret_cast<const char*>(j.d), j.n); t = reinterpret_cast<const uint8_t*>(tail.data()); tn = tail.size(); }
            else { const size_t from = j.nl[r - L - 1] + 1; t = j.d + from; tn = j.n - from; }
            add(r, ls, ln, split(t, tn, false, ls, ln));
        }
        { std::unique_lock<std::mutex> lk(m_); if (!spare_.empty()) { j.out = std::move(spare_.back()); spare_.pop_back(); } }
        pack_lines(ptr, len, k_, j.out, qptr, min_qual_, want_ends_);
    }

    // ---- pieces in, jobs out ------------------------------------------------------------------------------------------------
    void push_job(std::shared_ptr<Job> j) {
        Job* jp = j.get();
        {
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return quit_ || q1_.size() + q2_.size() < (size_t)threads_ * kAheadJobs; });
            if (quit_) return;
            q1_.push_back(std::move(j));
            tasks_.push_back([this, jp] { stage_a(*jp); });
        }
        cv_.notify_all();
    }
    void feed() {
        try {
            if (gz_) {
                pargz::Piece p;
                while (gz_->take(p)) {
                    auto j = std::make_shared<Job>();
                    j->piece = std::move(p); j->d = reinterpret_cast<const uint8_t*>(j->piece.d); j->n = j->piece.n;
                    push_job(std::move(j));
                    { std::unique_lock<std::mutex> lk(m_); if (quit_) return; }
                }
            } else {
                for (size_t at = 0; at < plain_n_; at += kSlice) {
                    auto j = std::make_shared<Job>();
                    j->d = plain_ + at; j->n = std::min(kSlice, plain_n_ - at);
                    push_job(std::move(j));
                    { std::unique_lock<std::mutex> lk(m_); if (quit_) return; }
                }
            }
        } catch (const std::exception& e) {
            std::unique_lock<std::mutex> lk(m_);
            if (error_.empty()) error_ = e.what();
        }
        { std::unique_lock<std::mutex> lk(m_); feed_done_ = true; }
        cv_.notify_all();
    }
    // in order: every piece learns its first line's number and the beginning of that line; then it is packed
    void sequence() {
        uint64_t lines = 0;
        std::string head;
        std::shared_ptr<Job> held;   // the newest piece: it is sent on once it is known whether it is the text's last
        auto send = [&](std::shared_ptr<Job> j, bool last) {
            j->line_base = lines; j->head = head; j->last = last;
            const uint64_t before = lines;
            lines += j->nl.size();
            // the carry: the line in progress, or with qualities the record in progress (from its first line, lines & ~3, on)
            const uint64_t from_line = min_qual_ > 0 ? lines & ~3ull : lines;
            if (from_line <= before) head.append(reinterpret_cast<const char*>(j->d), j->n);
            else {
                const size_t at = j->nl[from_line - 1 - before] + 1;
                head.assign(reinterpret_cast<const char*>(j->d + at), j->n - at);
            }
            Job* jp = j.get();
            {
                std::unique_lock<std::mutex> lk(m_);
                q2_.push_back(std::move(j));
                tasks_.push_back([this, jp] { stage_b(*jp); });
            }
            cv_.notify_all();
        };
        for (;;) {
            std::shared_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || !q1_.empty() || feed_done_; });
                if (quit_) return;
                if (q1_.empty()) break;
                j = q1_.front(); q1_.pop_front();
            }
            cv_.notify_all();
            j->done_a.get_future().wait();
            if (held) send(std::move(held), false);
            held = std::move(j);
        }
        if (held) send(std::move(held), true);
        { std::unique_lock<std::mutex> lk(m_); seq_done_ = true; }
        cv_.notify_all();
    }

    // ---- the line loop (streams, one thread): the same batches, 64 Ki reads at a time ------------------------------------------
    bool next_serial(PackedBatch& out) {
        if (serial_end_) return false;
        constexpr uint64_t kBatchReads = 1u << 16;
        const bool qual = min_qual_ > 0;   // (the quality line, line 3 mod 4, goes into qbuf_ at the sequence line's offset)
        buf_.clear(); off_.assign(1, 0); qbuf_.clear();
        for (; off_.size() <= kBatchReads || (qual && (serial_line_ & 3u) != 0u);) {   // (with qualities: whole records)
            const uint64_t at = serial_line_ & 3u;
            if (at == 3u && qual) {
                const size_t q0 = qbuf_.size();
                const bool got = lines_->append_next(qbuf_);   // (none: a record cut short, an empty quality line)
                check_record(serial_line_ - 3, off_.back() - off_[off_.size() - 2], qbuf_.size() - q0);
                if (!got) { serial_end_ = true; break; }
                serial_line_++; continue;
            }
            if (at != 1u) {
                if (!lines_->skip_next()) {
                    serial_end_ = true;
                    // (a record cut short after its sequence line has no quality line: an empty one)
                    if (qual && at == 2u) check_record(serial_line_ - 2, off_.back() - off_[off_.size() - 2], 0);
                    break;
                }
                serial_line_++; continue;
            }
            if (!lines_->append_next(buf_)) { serial_end_ = true; break; }
            serial_line_++;
            off_.push_back(buf_.size());
        }
        if (off_.size() == 1 && serial_end_) return false;
        std::vector<const uint8_t*> ptr(off_.size() - 1);
        std::vector<uint64_t> len(off_.size() - 1);
        for (size_t i = 0; i + 1 < off_.size(); i++) { ptr[i] = reinterpret_cast<const uint8_t*>(buf_.data()) + off_[i]; len[i] = off_[i + 1] - off_[i]; }
        if (qual) {
            std::vector<const uint8_t*> qptr(off_.size() - 1);
            for (size_t i = 0; i + 1 < off_.size(); i++) qptr[i] = reinterpret_cast<const uint8_t*>(qbuf_.data()) + off_[i];
            pack_lines(ptr, len, k_, out, qptr, min_qual_, want_ends_);
        } else {
            pack_lines(ptr, len, k_, out, want_ends_);
        }
        return true;
    }

    std::string path_;
    int k_;
    unsigned threads_;
    int min_qual_;
    bool want_ends_;
    std::unique_ptr<ParallelGunzip> gz_;
    std::unique_ptr<GzLineReader> lines_;
    int fd_ = -1;
    const uint8_t* plain_ = nullptr;
    size_t plain_n_ = 0;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::function<void()>> tasks_;
    std::deque<std::shared_ptr<Job>> q1_, q2_;   // waiting for their line ends / for their batch, in file order
    std::deque<PackedBatch> spare_;              // batches the caller handed back: their buffers are used again
    std::vector<std::vector<uint32_t>> spare_nl_;   // ... and the jobs' lists of line ends
    std::vector<std::thread> workers_;
    std::thread feeder_, sequencer_;
    bool quit_ = false, feed_done_ = false, seq_done_ = false;
    std::string error_;
    std::string buf_, qbuf_;
    std::vector<uint64_t> off_;
    uint64_t serial_line_ = 0;
    bool serial_end_ = false;
};

}  // namespace bronko
