// reads.hpp -- the reader side of `bronko call`: FASTQ(.gz) files -> batches -> the engine's push entry points (reads.cpp).
#pragma once
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include "cli.hpp"

namespace bronko {

struct SampleReaders;   // a sample's mate files being read: a queue and a reader thread each (reads.cpp)

// The sequence text that samples read ahead of their turn hold in their queues, all of them together: counted as it is queued
// (a batch's real bytes, not an estimate from the compressed size: amplicon FASTQ inflates 8-10x), released as lanes consume.
struct AheadGate {
    std::mutex m;
    std::condition_variable cv;
    uint64_t held = 0, budget = 0;
};

// The files of the samples to come are read while the index and the engine's tables are being made (seconds with a hundred
// genomes: host work that leaves most cores idle) and while earlier samples are on their way: a manager thread starts the
// readers of sample after sample, `concurrency` files at a time, as long as the text the started samples hold in their queues
// stays within `budget` bytes (AheadGate: real bytes; readers wait when it is full and go on as lanes consume); a lane that
// reaches a sample takes its readers over (claim) or, if they were not started, reads it itself as before.  Inputs that are not
// regular files (a FIFO, /dev/fd/N) are never read ahead: their size is unknown and they can be read once.
class ReadAhead {
public:
    // (samples and cfg outlive this object; the readers start packing at once: cfg is complete before)
    ReadAhead(const std::vector<std::vector<std::string>>& samples, const CallConfig& cfg, unsigned concurrency, uint64_t budget);
    ~ReadAhead();
    bool covers_all() const { return covers_all_; }   // every sample's text fits the budget (by the estimate): the lanes only push
    void set_concurrency(unsigned n);                 // (few files at a time while the engine's tables are made on the same cores, more behind that)
    // the readers of sample i if it is being read ahead; otherwise nullptr, and it will not be
    std::unique_ptr<SampleReaders> claim(size_t i);
private:
    void run();
    const std::vector<std::vector<std::string>>& samples_;
    const CallConfig& cfg_;
    std::vector<int> state_;                              // 0 not started, 1 being read ahead, 2 taken by its lane
    std::vector<std::unique_ptr<SampleReaders>> held_;
    unsigned concurrency_, active_ = 0;
    AheadGate gate_;
    bool stop_ = false, covers_all_ = false;
    std::mutex m_;
    std::condition_variable cv_;
    std::thread manager_;
};

// The mate files of sample `sample_id`, pushed into engs: one engine (the sample's reads all go there) or one per GPU of a sharded
// sample -- batches are dealt to them in turn.  The readers are those of `ahead` if it has started them, otherwise the call's own,
// with `inflate_threads` threads per file.  Returns reads seen; throws what a reader could not read.
uint64_t push_fastqs(const std::vector<bk_engine*>& engs, const std::vector<std::string>& mates, const CallConfig& cfg,
                     unsigned inflate_threads, ReadAhead* ahead, size_t sample_id);

}  // namespace bronko
