// reads.cpp -- the reader side of `bronko call` (reads.hpp): the FASTQ(.gz) files of a sample are inflated and parsed into batches by
// reader threads, ahead of the sample's turn where memory allows (ReadAhead), and pushed into the engine(s) by the sample's lane.
#include <atomic>
#include <chrono>
#include <deque>
#include <functional>
#include <stdexcept>

#include <sys/stat.h>

#include "reads.hpp"
#include "fastq_pack.hpp"
#include "fastx.hpp"

namespace bronko {

// The mate files of one sample: FASTQ(.gz) -> batches of sequence lines -> bk_push_reads_ascii (packed on the GPU,
// asynchronous: the next batch is parsed while the previous ones are copied, packed and scanned).  Every mate file is
// inflated and parsed by its own host thread (upstream runs the two KMC processes of a pair concurrently too,
// call.rs:301-307); the engine is only ever called from this thread.  Returns reads seen.
struct FastqBatch {
    std::string buf; std::vector<uint64_t> off{0};   // sequence lines back to back (the line loop: streams, one thread) ...
    std::string qual;                                // (--min-base-qual) ... and their quality lines, at the same offsets
    PackedBatch packed; bool is_packed = false;      // ... or 2-bit records, parsed and packed on several threads (fastq_pack.hpp;
                                                     // --primers, --adapter: with their end flags)
    bool last = false; std::string error;
    size_t bytes() const { return is_packed ? packed.bytes() : buf.size() + qual.size(); }
};
struct BatchQueue {
    std::mutex m;
    std::condition_variable cv;
    std::deque<FastqBatch> q;
    std::vector<FastqBatch> spare;   // consumed batches, handed back: their 40 MB buffers are reused instead of being unmapped and
                                     // mapped again (with dozens of lanes the page faults of fresh buffers cost more than the parsing)
    static constexpr size_t kDepth = 3;
    // A sample read ahead of its turn (ReadAhead below): the whole file may wait here as long as the gate has room.  Once a lane has
    // claimed the sample the queue is an ordinary one again (kDepth batches ahead of the lane) and no longer waits for the gate: the
    // lane must never wait for text that later samples' queues hold.
    AheadGate* gate = nullptr;
    std::atomic<bool> claimed{false};
    std::atomic<bool> abandoned{false};   // nobody will take from this queue any more (a run that ends early): the reader stops
    void put(FastqBatch&& b) {
        const uint64_t sz = b.bytes();
        if (gate) {
            std::unique_lock<std::mutex> gl(gate->m);
            gate->cv.wait(gl, [&] { return abandoned.load() || claimed.load() || gate->held == 0 || gate->held + sz <= gate->budget; });
            if (abandoned.load()) return;
            gate->held += sz;
        }
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return abandoned.load() || (gate && !claimed.load()) || q.size() < kDepth; });
        if (abandoned.load()) return;
        q.push_back(std::move(b));
        cv.notify_all();
    }
    void abandon() {
        abandoned.store(true);
        if (gate) { std::unique_lock<std::mutex> gl(gate->m); gate->cv.notify_all(); }
        { std::unique_lock<std::mutex> lk(m); cv.notify_all(); }
    }
    FastqBatch take() {
        FastqBatch b;
        {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return !q.empty(); });
            b = std::move(q.front());
            q.pop_front();
            cv.notify_all();
        }
        if (gate) {
            { std::unique_lock<std::mutex> gl(gate->m); gate->held -= std::min<uint64_t>(gate->held, b.bytes()); }
            gate->cv.notify_all();
        }
        return b;
    }
    void claim() {   // a lane takes the sample over
        claimed.store(true);
        if (gate) { std::unique_lock<std::mutex> gl(gate->m); gate->cv.notify_all(); }
        { std::unique_lock<std::mutex> lk(m); cv.notify_all(); }
    }
    void recycle(FastqBatch&& b) {
        std::unique_lock<std::mutex> lk(m);
        if (spare.size() < kDepth + 2) spare.push_back(std::move(b));
    }
    FastqBatch fresh() {
        FastqBatch b;
        {
            std::unique_lock<std::mutex> lk(m);
            if (!spare.empty()) { b = std::move(spare.back()); spare.pop_back(); }
        }
        b.buf.clear(); b.off.clear(); b.off.push_back(0); b.qual.clear(); b.packed.clear(); b.is_packed = false; b.last = false; b.error.clear();
        return b;
    }
};
static void parse_fastq(const std::string& path, BatchQueue& out, const CallConfig& cfg, unsigned inflate_threads) {
    constexpr uint64_t kBatchReads = 1u << 16;   // (10 MB of bases: the engine pins three staging slots of that size per lane)
    FastqBatch cur;
    try {
        if (inflate_threads > 1) {
            // threads to spare: the file's text is taken apart and 2-bit packed piece by piece on as many threads (fastq_pack.hpp);
            // a few MB of text make a piece, pieces are gathered into batches of a quarter of a million records (a scan launch has
            // a fixed cost: small pushes are slow pushes)
            constexpr uint64_t kBatchRecords = 1u << 18;
            FastqPacker in(path, cfg.k, inflate_threads, cfg.min_qual, cfg.trims());
            PackedBatch b;
            cur.is_packed = true;
            while (in.next(b)) {
                if (cur.packed.n_records && (cur.packed.stride != b.stride || cur.packed.n_records + b.n_records > 2 * kBatchRecords)) {
                    out.put(std::move(cur)); cur = out.fresh(); cur.is_packed = true;
                    if (out.abandoned.load()) break;
                }
                if (!cur.packed.n_records) { const uint64_t r = cur.packed.n_reads; cur.packed = std::move(b); cur.packed.n_reads += r; b = PackedBatch(); }
                else {
                    cur.packed.words.insert(cur.packed.words.end(), b.words.begin(), b.words.end());
                    cur.packed.lens.insert(cur.packed.lens.end(), b.lens.begin(), b.lens.end());
                    cur.packed.ends.insert(cur.packed.ends.end(), b.ends.begin(), b.ends.end());
                    cur.packed.n_records += b.n_records; cur.packed.n_reads += b.n_reads;
                }
                if (cur.packed.n_records >= kBatchRecords) { out.put(std::move(cur)); cur = out.fresh(); cur.is_packed = true; if (out.abandoned.load()) break; }
            }
        } else {
            GzLineReader in(path, inflate_threads);
            uint64_t n = 0;
            // --min-base-qual: a record's quality line (line 3) goes into the batch too, and the batch ends behind it
            auto check = [&](uint64_t ln, size_t qn) {
                const size_t sn = cur.off.back() - cur.off[cur.off.size() - 2];
                if (qn != sn)
                    throw std::runtime_error(path + ": record " + std::to_string(ln / 4 + 1) + ": quality line of " + std::to_string(qn) +
                                             " bytes for a sequence of " + std::to_string(sn) + " (--min-base-qual)");
            };
            for (uint64_t ln = 0;; ln++) {               // 4-line FASTQ records: @id / sequence / + / quality
                if (cfg.min_qual > 0 && (ln & 3) == 3) {
                    const size_t q0 = cur.qual.size();
                    const bool got = in.append_next(cur.qual);   // (none: a record cut short, an empty quality line)
                    check(ln, cur.qual.size() - q0);
                    if (!got) break;
                    if (n % kBatchReads == 0) { out.put(std::move(cur)); cur = out.fresh(); if (out.abandoned.load()) break; }
                    continue;
                }
                if ((ln & 3) != 1) {
                    if (!in.skip_next()) { if (cfg.min_qual > 0 && (ln & 3) == 2) check(ln, 0); break; }
                    continue;
                }
                if (!in.append_next(cur.buf)) break;     // (the sequence line goes straight into the batch)
                cur.off.push_back(cur.buf.size());
                if (++n % kBatchReads == 0 && cfg.min_qual == 0) { out.put(std::move(cur)); cur = out.fresh(); if (out.abandoned.load()) break; }
            }
        }
    } catch (const std::exception& e) {
        cur = FastqBatch();
        cur.error = e.what();
    }
    cur.last = true;
    out.put(std::move(cur));
}
struct SampleReaders {
    std::deque<BatchQueue> queues;   // (a deque: BatchQueue holds a mutex and does not move)
    std::vector<std::thread> readers;
};
// bytes of sequence lines a sample's batches will hold, estimated from the files' sizes; false: a mate is not a regular file
static bool text_estimate(const std::vector<std::string>& mates, uint64_t* out) {
    uint64_t n = 0;
    bool regular = true;
    for (const auto& p : mates) {
        struct stat st;
        if (stat(p.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) { regular = false; continue; }
        n += (uint64_t)st.st_size * 2;   // (FASTQ text is ~3.5x its gzip, the sequence lines half of it)
    }
    *out = n;
    return regular;
}
ReadAhead::ReadAhead(const std::vector<std::vector<std::string>>& samples, const CallConfig& cfg, unsigned concurrency, uint64_t budget)
    : samples_(samples), cfg_(cfg), state_(samples.size(), 0), held_(samples.size()), concurrency_(std::max(1u, concurrency)) {
    gate_.budget = budget;
    uint64_t all = 0;
    bool regular = true;
    for (const auto& m : samples) { uint64_t n = 0; regular = text_estimate(m, &n) && regular; all += n; }
    covers_all_ = regular && all <= budget;
    manager_ = std::thread([this] { run(); });
}
void ReadAhead::set_concurrency(unsigned n) {
    { std::unique_lock<std::mutex> lk(m_); concurrency_ = std::max(1u, n); }
    cv_.notify_all();
}
ReadAhead::~ReadAhead() {
    { std::unique_lock<std::mutex> lk(m_); stop_ = true; }
    cv_.notify_all();
    if (manager_.joinable()) manager_.join();
    // (readers of samples no lane came for -- a run that ended early -- must not wait for room that nobody will make)
    for (auto& h : held_) if (h) for (auto& q : h->queues) q.abandon();
    for (auto& h : held_) if (h) for (auto& t : h->readers) if (t.joinable()) t.join();
}
std::unique_ptr<SampleReaders> ReadAhead::claim(size_t i) {
    std::unique_lock<std::mutex> lk(m_);
    if (state_[i] == 1) {
        state_[i] = 2;
        for (auto& q : held_[i]->queues) q.claim();
        return std::move(held_[i]);
    }
    state_[i] = 2;
    return nullptr;
}
void ReadAhead::run() {
    for (size_t i = 0; i < samples_.size(); i++) {
        // room for another sample?  (real bytes: three quarters of the budget held means the readers already started fill the rest)
        for (;;) {
            { std::unique_lock<std::mutex> lk(m_); if (stop_) return; }
            std::unique_lock<std::mutex> gl(gate_.m);
            if (gate_.held <= gate_.budget / 4 * 3) break;
            gate_.cv.wait_for(gl, std::chrono::milliseconds(20));
        }
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || active_ + samples_[i].size() <= concurrency_; });
        if (stop_) return;
        if (state_[i] != 0) continue;                 // a lane got there first
        uint64_t need = 0;
        if (!text_estimate(samples_[i], &need)) continue;   // (a stream: its lane reads it)
        auto sr = std::unique_ptr<SampleReaders>(new SampleReaders);
        for (size_t m = 0; m < samples_[i].size(); m++) { sr->queues.emplace_back(); sr->queues.back().gate = &gate_; }
        for (size_t m = 0; m < samples_[i].size(); m++) {
            active_++;
            sr->readers.emplace_back([this, i, m, q = &sr->queues[m]] {
                parse_fastq(samples_[i][m], *q, cfg_, cfg_.ahead_inflate_threads);
                { std::unique_lock<std::mutex> lk2(m_); active_--; }
                cv_.notify_all();
            });
        }
        state_[i] = 1;
        held_[i] = std::move(sr);
    }
}

uint64_t push_fastqs(const std::vector<bk_engine*>& engs, const std::vector<std::string>& mates, const CallConfig& cfg,
                     unsigned inflate_threads, ReadAhead* ahead, size_t sample_id) {
    const size_t nm = mates.size();
    size_t n_batches = 0;
    std::unique_ptr<SampleReaders> sr = ahead ? ahead->claim(sample_id) : nullptr;
    if (!sr) {
        sr.reset(new SampleReaders);
        for (size_t m = 0; m < nm; m++) sr->queues.emplace_back();
        for (size_t m = 0; m < nm; m++) sr->readers.emplace_back(parse_fastq, std::cref(mates[m]), std::ref(sr->queues[m]), std::cref(cfg), inflate_threads);
    }
    std::deque<BatchQueue>& queues = sr->queues;
    std::vector<std::thread>& readers = sr->readers;
    uint64_t n_reads = 0;
    std::string error;
    std::vector<bool> done(nm, false);
    for (size_t left = nm; left;) {
        for (size_t m = 0; m < nm; m++) {
            if (done[m]) continue;
            FastqBatch b = queues[m].take();
            if (!b.error.empty() && error.empty()) error = b.error;
            // (a batch that is pushed goes to the next engine in turn)
            const bool pushed = error.empty() && (b.is_packed ? b.packed.n_records != 0 : b.off.size() > 1);
            bk_engine* const eng = pushed ? engs[n_batches++ % engs.size()] : nullptr;
            if (error.empty() && b.is_packed) {
                if (pushed && cfg.trims())
                    hip_check(bk_push_reads_packed_ends(eng, (int)m, b.packed.words.data(), b.packed.stride, b.packed.lens.data(), b.packed.ends.data(), b.packed.n_records),
                              "bk_push_reads_packed_ends");
                else if (pushed)
                    hip_check(bk_push_reads_packed(eng, (int)m, b.packed.words.data(), b.packed.stride, b.packed.lens.data(), b.packed.n_records), "bk_push_reads_packed");
                n_reads += b.packed.n_reads;
            } else if (pushed) {
                const uint8_t* bases = reinterpret_cast<const uint8_t*>(b.buf.data());
                if (cfg.min_qual > 0)
                    hip_check(bk_push_reads_ascii_qual(eng, (int)m, bases, reinterpret_cast<const uint8_t*>(b.qual.data()), b.off.data(), b.off.size() - 1, cfg.min_qual), "bk_push_reads_ascii_qual");
                else hip_check(bk_push_reads_ascii(eng, (int)m, bases, b.off.data(), b.off.size() - 1), "bk_push_reads_ascii");
                n_reads += b.off.size() - 1;
            }
            if (b.last) { done[m] = true; left--; }
            else queues[m].recycle(std::move(b));   // (bk_push_reads_ascii has copied it to its pinned ring)
        }
    }
    for (auto& t : readers) t.join();
    if (!error.empty()) throw std::runtime_error(error);
    return n_reads;
}

}  // namespace bronko
