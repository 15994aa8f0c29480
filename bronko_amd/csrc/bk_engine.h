// bk_engine.h -- private to the host side of the engine: error reporting, device and pinned buffers, host-thread helpers, the
// index tables that bk_engine_create builds and its forks share, and struct bk_engine itself.  Included by bk_index_tables.cpp (the
// index tables), bk_ingest.cpp (reads -> records ready to scan: the bk_push_reads_* entry points, K0, the trimming stage, the host
// packer), bk_engine.cpp (the engine's life, the sample path from push_device to bk_sample_download), bk_riders.cpp (the passes that
// ride behind every scan: the k-mer dump, indels, linkage and the codon, haplotype and read-pileup counts over linkage's rows), bk_reports.cpp (the reports made of a pileup: calls, consensus, minor alleles, regions)
// and bk_cohort.hip (the distances of a cohort of consensus sequences, its minimum spanning forest and the alleles its samples carry of each other).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bronko_hip.h"
#include "bk_device.h"
#include "bk_kernels.h"

// (the library's exports are the C ABI of bronko_hip.h: nothing declared here leaves it)
#pragma GCC visibility push(hidden)

extern thread_local std::string g_err;   // bk_last_error

int fail(int code, const char* fmt, ...);
struct bk_engine;

#define BK_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return fail(BK_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// One device allocation, freed with its owner.  Not copyable: a copy would free the same memory twice.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t count) {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = count;
        return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
    }
    template <class A>
    hipError_t upload(const std::vector<T, A>& h) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};
static_assert(!std::is_copy_constructible_v<DevBuf<int>> && !std::is_copy_assignable_v<DevBuf<int>>, "DevBuf owns its memory");
// Room for `need` elements: a buffer that is too small is allocated again a quarter (+ `extra`) larger, its contents lost.  `drain`:
// null when nothing in flight can still use the old memory (the caller has waited for it), else the stream to drain before it goes.
template <typename T>
hipError_t grow(DevBuf<T>& b, size_t need, size_t extra = 0, hipStream_t drain = nullptr) {
    if (b.n >= need) return hipSuccess;
    if (drain) { hipError_t e = hipStreamSynchronize(drain); if (e != hipSuccess) return e; }
    return b.alloc(need + need / 4 + extra);
}

// A pinned host allocation and an event, each freed with its owner (move-only)
template <typename T>
struct PinnedBuf {
    T* p = nullptr; size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t grow(size_t need, size_t extra = 0) {   // (like grow of a DevBuf)
        if (n >= need) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr; n = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), (need + need / 4 + extra) * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) n = need + need / 4 + extra;
        return e;
    }
};
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }   // (first use)
    operator hipEvent_t() const { return ev; }
};

// A batch of records on the device, as the scan and what runs beside it read them
struct Records {
    const uint32_t* words;                      // [n][stride_words] 2-bit bases, 16 a word
    uint32_t stride_words;
    const uint16_t* lens;                       // [n]
    uint64_t n;                                 // records; with n_dev, the slots the batch can fill at most
    const unsigned long long* n_dev = nullptr;  // null, or the device's count of the slots in use (K0)
    uint64_t kmers_upper = 0;                   // a bound on the batch's k-mers (0: every base of every record)
};
// The device buffers that hold such a batch for the engine: a slot of the ASCII or the packed pushes, bk_engine::dev_ascii
struct RecordBufs {
    DevBuf<uint32_t> words; DevBuf<uint16_t> lens;
    DevBuf<uint8_t> ends;                       // primers or adapters set: the records' end flags
    hipError_t reserve(uint64_t n, uint32_t stride_words, hipStream_t drain) {   // (words and lengths; `drain` as for grow)
        hipError_t e = grow(words, (size_t)n * stride_words, 0, drain);
        return e != hipSuccess ? e : grow(lens, (size_t)n, 0, drain);
    }
    Records view(uint32_t stride_words, uint64_t n, const unsigned long long* n_dev = nullptr, uint64_t kmers_upper = 0) const {
        return Records{words.p, stride_words, lens.p, n, n_dev, kmers_upper};
    }
};

struct TimedSpan { hipEvent_t a, b; int kind; };

// fn(begin, end) over [0, n) on up to hardware_concurrency() threads (capped at 256): host-side table construction only
template <typename F>
void parallel_for(size_t n, F&& fn) {
    unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 256u);
    if (n < (size_t)nt * 1024) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (unsigned i = 0; i < nt; i++) {
        const size_t b = std::min(n, i * per), en = std::min(n, b + per);
        if (b < en) th.emplace_back([&fn, b, en] { fn(b, en); });
    }
    for (auto& t : th) t.join();
}

// A host array whose elements are not initialised by its constructor (the GB-sized tables of a many-genome index: a serial
// value-initialisation was 0.3 s each; they are filled by parallel_for)
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    template <class U, class... A>
    void construct(U* p, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new (static_cast<void*>(p)) U;
        else ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
    }
};
template <class T> using HostVec = std::vector<T, NoInitAlloc<T>>;
template <class T>
HostVec<T> filled(size_t n, const T& v) {
    HostVec<T> a(n);
    parallel_for(n, [&](size_t i0, size_t i1) { std::fill(a.begin() + (ptrdiff_t)i0, a.begin() + (ptrdiff_t)i1, v); });
    return a;
}

// Testing / measurement aids exist only in the -DBK_TESTING build (libbronko_hip_testing.so, loaded by the tests that force a
// path and by the profiling tools); the release library reads no environment variable.
#ifdef BK_TESTING
inline const char* test_env(const char* name) { return getenv(name); }
#else
inline const char* test_env(const char*) { return nullptr; }
#endif

// BK_CREATE_TIMING=1 (testing build): wall-clock of the phases of bk_engine_create on stderr (host-side table construction)
struct PhaseClock {
    bool on = test_env("BK_CREATE_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[bk_engine_create] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// An open-addressing table of u64 keys (~0 = free) and u32 counts whose load stays below one half as a sample fills it
// (ensure_room): full_kmer_stats' statistics table and the k-mer dump's count table (bk_kmer_dump_enable).  Its device-side
// companion `out` holds the overflow flag at [4] and the tallies of new keys at [8 ..] (ktab_insert_key, kmer_dump_count_kernel).
struct GrowTable {
    DevBuf<unsigned long long> keys;
    DevBuf<unsigned int> cnt;
    uint32_t log2 = 0;                      // current capacity (grows with the sample: ensure_room)
    PinnedBuf<unsigned long long> h_fill;   // pinned copy of the tallies, refreshed after every push
    Event fill_ev;
    bool fill_pending = false;              // a copy of the tallies is in flight / unread
    uint64_t fill_known = 0, fill_unknown_upper = 0;   // keys in the table at the last reading; k-mers pushed since (upper bound on new keys)
    std::vector<std::pair<unsigned long long*, unsigned int*>> old;   // outgrown tables, freed at the next sample / destroy
    void read_fill() {   // (the copy of the tallies has arrived)
        fill_known = 0; fill_unknown_upper = 0; fill_pending = false;
        for (uint32_t i = 0; i < bk::ktab_fill_words(); i++) fill_known += h_fill.p[i];
    }
    ~GrowTable() { for (auto& o : old) { (void)hipFree(o.first); (void)hipFree(o.second); } }
    // (bk_engine.cpp: on the engine's stream; `out` is the table's device-side companion)
    int clear(bk_engine* e);                                                  // a sample starts from an empty table
    int ensure_room(bk_engine* e, unsigned long long* out, uint64_t upper);   // before a batch of at most `upper` k-mers
    int note_fill(bk_engine* e, const unsigned long long* out);               // after it: a fresh copy of the tallies
};

// bk_kmer_dump_enable: the sample's count table of every strand-specific k-mer (bk_kmer_dump.hip) and, per finalized mate file, its
// selected entries sorted by k-mer
struct KmerDump {
    GrowTable t;
    DevBuf<unsigned long long> out;         // [mate][2] kept, distinct + [4] overflow flag + [8 ..] tallies of new keys
    DevBuf<unsigned long long> sel_keys, keys[2];   // selected (unsorted, padded with ~0) -> sorted, per mate file
    DevBuf<unsigned int> sel_cnt, cnt[2];
    DevBuf<unsigned char> sort_tmp;
    uint64_t upper[2] = {0, 0};             // k-mers pushed per mate file in this sample (bounds its distinct keys)
    uint64_t n_sorted[2] = {0, 0};          // length of the sorted arrays of the last finalize (selected entries, then padding)
    bool in_sample = false;                 // enabled when the current / last sample began
    int finalized_mates = 0;                // mate files the last finalize selected (0: none, or finalized by shards)
    int begin_sample(bk_engine* e);         // (bk_riders.cpp: these three issue work on the engine's stream)
    int push(bk_engine* e, int mate, const Records& r, uint64_t upper);   // in front of the scan of the same records
    int finalize(bk_engine* e, int n_mates);                              // at the end of a whole-sample finalize
};

// What bk_primers_set and bk_adapters_set keep alike: the sample's counters and whether the stage was set when the sample began
struct TrimStage {
    const uint32_t n_stats;                 // counters per mate file
    DevBuf<unsigned long long> stats;       // [2][n_stats] (zeroed by bk_sample_begin)
    bool in_sample = false;                 // set when the current / last sample began
    explicit TrimStage(uint32_t n_stats_) : n_stats(n_stats_) {}
    int begin_sample(bk_engine* e);         // (bk_ingest.cpp)
};
// bk_primers_set: the primer table (bk_primers.hip); stats: reads trimmed at 5', at 3', bases masked
struct Primers : TrimStage {
    Primers() : TrimStage(3) {}
    DevBuf<uint32_t> table;                 // [n][bk::kPrimerEntryWords]
    uint32_t n = 0;
    uint32_t max_mismatches = 0;
};
// bk_adapters_set: the adapter table as the kernels take it (bk_adapters.hip) and the per-record scratch; stats: reads cut, bases removed
struct Adapters : TrimStage {
    Adapters() : TrimStage(2) {}
    bk::AdapterEntry entry[bk::kMaxAdapters] = {};
    uint32_t n = 0;
    uint32_t min_overlap = 0;
    uint64_t allowed_steps = 0;             // bk::AdapterArgs::allowed_steps
    DevBuf<uint32_t> cut;                   // [records of the largest batch so far] bk::kNoCut between launches
};

// bk_regions_set: the region table as region_depth_kernel takes it (bk_regions.hip) and the result buffers, allocated with it
struct Regions {
    DevBuf<uint2> table;                    // [n] {first cell, L}, grouped by genome file, the caller's order within a file
    DevBuf<uint32_t> file_off;              // [n_files + 1]
    DevBuf<bk_region_depth> rows;           // [max_file_regions]
    DevBuf<bk_region_summary> out;
    uint32_t max_file_regions = 0;          // regions of the genome file with the most: the kernel's grid
};

// What placing a record by two anchor k-mers reads beside the index tables (bk_anchor.h): built by the first of bk_indels_enable,
// bk_junctions_enable, bk_copybacks_enable, bk_chimeras_enable, bk_breakends_enable, bk_duplications_enable and bk_link_enable, used by all of them, freed
// with the last
struct AnchorTables {
    DevBuf<uint32_t> unique_bits;           // one bit per reference k-mer id: it starts at exactly one cell (a histogram of id_at)
    DevBuf<uint32_t> seq_lo;                // [sequences + 1] first cells, then total_cells
    DevBuf<uint2> nruns;                    // IndexTables::h_nonacgt
};

// One count over the sample's row store at a time -- what bk_sample_linkage (Linkage), bk_sample_codons (Codons),
// bk_sample_haplotypes (Haplotypes) and bk_sample_read_pileup (ReadPileup) keep alike.  A call replaces the tables, counters and pinned copies that the last call's kernels may
// still read, so it first waits for them, and for them alone; it ends by recording `counted` behind its own launches.
struct StoreCount {
    Event counted;                          // behind the last count's launches
    bool count_in_flight = false;
    bool made = false;                      // the results are this sample's (cleared by Linkage::begin_sample and while a call replaces them)
    int wait_last();                        // (bk_riders.cpp) nothing else of the stream's work is waited for; the results are void from here on
    int record(hipStream_t stream);         // behind this count's launches: the results are this sample's
};

// bk_sample_codons: the region tables and the counters of the last call (bk_codons.hip).  Made by the first call, freed with the Linkage
// whose row store it reads; its buffers grow and never shrink
struct Codons : StoreCount {
    DevBuf<uint4> sorted;                   // [regions] by first cell (bk_kernels.h CodonArgs::sorted)
    DevBuf<uint2> regions;                  // [regions] the caller's order
    DevBuf<unsigned int> cover_diff;        // [codons + 1]
    DevBuf<unsigned int> counts;            // [codons][64]
    PinnedBuf<uint4> h_sorted;              // pinned host copies: the uploads are asynchronous
    PinnedBuf<uint2> h_regions;
    uint32_t n_regions = 0, n_codons = 0;
};

// bk_sample_haplotypes: the region tables, the hot counters, the table of distinct haplotypes and the entry list of the last call
// (bk_haplotypes.hip).  Made by the first call, freed with the Linkage whose row store it reads; its buffers grow and never shrink
struct Haplotypes : StoreCount {
    DevBuf<uint2> sorted;                   // [regions] by first cell (bk_kernels.h HapArgs::sorted)
    DevBuf<uint2> regions;                  // [regions] the caller's order
    DevBuf<unsigned int> hot;               // [regions][2] cover, ref_count
    DevBuf<unsigned long long> owner;       // [2^table_log2]
    DevBuf<unsigned int> count;             // [2^table_log2]
    DevBuf<unsigned long long> tallies;     // [2] entries, dropped
    DevBuf<bk_hap_entry> entries;           // [2^table_log2]
    PinnedBuf<uint2> h_sorted, h_regions;   // pinned host copies: the uploads are asynchronous
    uint32_t n_regions = 0, table_log2 = 0;
};

// bk_sample_read_pileup: the work arrays and the cells of the last call (bk_read_pileup.hip).  Made by the first call for the index's
// cells, freed with the Linkage whose row store it reads
struct ReadPileup : StoreCount {
    DevBuf<unsigned int> work;              // [15 cells + 3] ReadPileupArgs::diff, mm, mm_near in this order: zeroed by one memset
    DevBuf<bk_read_pileup_cell> cells;      // [cells]
    DevBuf<unsigned long long> tallies;     // [2] covered, bases
    uint32_t end_dist = 0;
};

// bk_link_enable: the sample's row store (one bk_link_row per placed record), its tallies, and what the last bk_sample_linkage made
// (the StoreCount it is itself)
struct Linkage : StoreCount {
    bk_link_config cfg{};
    std::shared_ptr<AnchorTables> anchors;  // shared with bk_indels_enable
    DevBuf<uint4> rows;                     // [2 * capacity in rows]
    std::vector<std::pair<uint4*, Event>> old;   // outgrown stores with the event behind the copy out of them: freed once it has passed
    uint64_t rows_upper = 0;                // a bound on the rows in the store: the records of every batch pushed (the count is the device's)
    DevBuf<unsigned long long> tallies;     // [4] bk_kernels.h LinkArgs::tallies; [1] is the store's count of rows (RowStoreView::placed)
    DevBuf<uint32_t> sites, pair_lo;        // the last bk_sample_linkage's
    DevBuf<unsigned int> counts;            // [pairs][16]
    PinnedBuf<uint32_t> h_sites, h_pair_lo; // pinned host copies: the uploads are asynchronous, the download reads the enumeration
    uint32_t n_sites = 0, max_dist = 0;
    uint64_t n_pairs = 0;
    bool in_sample = false;                 // enabled when the current / last sample began
    std::unique_ptr<Codons> codons;         // bk_sample_codons (null: never called, no buffers)
    std::unique_ptr<Haplotypes> haps;       // bk_sample_haplotypes (likewise)
    std::unique_ptr<ReadPileup> read_pileup;   // bk_sample_read_pileup (likewise)
    ~Linkage() { for (auto& o : old) (void)hipFree(o.first); }
    int begin_sample(bk_engine* e);         // (bk_riders.cpp)
    int push(bk_engine* e, const Records& r);   // behind the scan of the same records, and behind the indels' pass
};

// An event pass of the engine (device side: bk_event_pass.h): what bk_indels_enable, bk_junctions_enable, bk_copybacks_enable,
// bk_chimeras_enable, bk_breakends_enable and bk_duplications_enable each allocate alike -- the sample's event table, span array and
// tallies -- and the sample's lifecycle (bk_riders.cpp: enable, begin_sample, push, report, download written once over these)
struct EventPass {
    std::shared_ptr<AnchorTables> anchors;  // shared with the other event passes and bk_link_enable
    DevBuf<unsigned long long> keys;        // [2^table_log2] the event table's key word (~0 = free; its layouts: event_insert, bk_anchor.h)
    DevBuf<unsigned int> counts;            // [2^table_log2][2] the two counters of a slot
    DevBuf<unsigned int> span;              // [total_cells + 2] difference array; prefix-summed by the sample's first bk_sample_x
    DevBuf<unsigned long long> tallies;     // [Args::kTallies] bk_kernels.h
    uint32_t table_log2 = 0;
    bool in_sample = false;                 // enabled when the current / last sample began
    bool summed = false;                    // span is prefix-summed (this sample's bk_sample_x ran)
    bool made = false;                      // ... and the rows are this sample's
    virtual ~EventPass() = default;
    int begin_sample(bk_engine* e);         // an empty table, a zero span array, zero tallies
    virtual int push(bk_engine* e, const Records& r) = 0;   // x_scan_kernel behind the scan of the same records
    virtual int clear_table(bk_engine* e);  // the part of begin_sample a pass with more than keys and counts adds to
};
// ... with what is typed by the pass: its configuration and the report's rows [2^table_log2]
template <class Cfg, class Row>
struct EventPassOf : EventPass {
    Cfg cfg{};
    DevBuf<Row> rows;
};
struct Indels : EventPassOf<bk_indel_config, bk_indel_record> {
    DevBuf<unsigned long long> key0, key1;  // [2^table_log2] the event table's two key words, in place of `keys`
    int push(bk_engine* e, const Records& r) override;
    int clear_table(bk_engine* e) override;
};
struct Junctions : EventPassOf<bk_junction_config, bk_junction_record> { int push(bk_engine* e, const Records& r) override; };
struct Copybacks : EventPassOf<bk_copyback_config, bk_copyback_record> { int push(bk_engine* e, const Records& r) override; };
struct Chimeras : EventPassOf<bk_chimera_config, bk_chimera_record> { int push(bk_engine* e, const Records& r) override; };
struct Breakends : EventPassOf<bk_breakend_config, bk_breakend_record> {
    DevBuf<unsigned int> site;              // [total_cells][2] the supporting records of every (cell, side), over every tag
    int push(bk_engine* e, const Records& r) override;
    int clear_table(bk_engine* e) override;
};
struct Duplications : EventPassOf<bk_duplication_config, bk_duplication_record> { int push(bk_engine* e, const Records& r) override; };

// bk_cohort_set: the cohort's bit planes, the output block of the last bk_cohort_distances and what bk_cohort_set_minor adds (bk_cohort.hip).  No part of a sample:
// bk_sample_begin and what follows it never look at it
struct Cohort {
    uint64_t n = 0, positions = 0;          // samples, letters of each
    uint64_t W = 0;                         // words of a plane: ceil(positions / 64)
    uint64_t n_stride = 0;                  // n rounded up to 64, plus 64: the padding samples are all zero
    DevBuf<unsigned long long> planes;      // [3][W][n_stride] valid, b0, b1
    DevBuf<unsigned int> out;               // [2][rows of the largest block so far][n] diff, compared
    // bk_cohort_set_minor (empty before it: no minor planes)
    DevBuf<unsigned long long> minor;       // [4][W][n_stride] M_A, M_C, M_G, M_T: X is present, the consensus is a base and not X
    DevBuf<unsigned int> minor_sites;       // [n] positions with any of the four
    DevBuf<unsigned int> ex_out;            // [rows of the largest block so far][n] explained (bk_cohort_explained's own block)
    // bk_cohort_mst (allocated by its first call on this cohort; empty before)
    DevBuf<unsigned int> mst_label;         // [n] a sample's component, named by the component's first sample
    DevBuf<unsigned long long> mst_row_key; // [n] per row the least diff << 32 | j over the admissible columns of another component (~0: none)
    DevBuf<unsigned int> mst_row_cmp;       // [n] ... and that pair's compared
    DevBuf<unsigned int> mst_comp_diff;     // [n] per label the least diff of its rows' bests (~0: none)
    DevBuf<unsigned long long> mst_comp_pair;   // [n] per label the least lo << 32 | hi among its rows' bests of that diff (~0: none)
};

// What bk_engine_create derives from the index and the table-shaping parameters (bk_index_tables.cpp): immutable once built, shared
// by an engine and its forks, freed with the last of them.
struct IndexTables {
    // engines that share these tables (the creating one and its forks, alive): with samples in flight next to each other the
    // binned scan leaves a quarter of the CUs to the siblings' small kernels (push_device)
    mutable std::atomic<int> family{1};
    int k = 0, wstart = 0, W = 0, n_files = 0;
    uint64_t total_cells = 0, n_slots = 0;
    uint32_t log2s = 4, log2nb = 0, log2p = 0, m = 1, n_u = 0, n_full = 0, n_lds_bins = 0;
    uint64_t n_prows = 0;  // V rows of the pseudo k-mers (bk_device.h)
    int v_omin = 0, v_span = 0;
    uint64_t v_off = 0, plane_len = 0;      // counter_plane_layout (bk_device.h)
    DevBuf<uint32_t> prow_id;
    DevBuf<uint8_t> prow_t;
    bool ref_in_lds = false;
    int lo_bases = 0, n_cus = 256;

    DevBuf<bk::KmerPos> kmer_pos;
    DevBuf<bk::IndexView> d_view;   // device copy of view()
    DevBuf<uint64_t> kmer_of;
    DevBuf<bk::IdRec> id_rec;
    DevBuf<bk::DirtyAns> dirty_ans;
    DevBuf<uint8_t> cell_flags;
    DevBuf<uint32_t> ref_words, cell_codes, cell_has, cell_clean, cell_clean3, cell_yf, cell_yr, id_at, cell_fast, cell_nat, cell_natrow;
    DevBuf<uint2> cell_blk, seed_tab, seed_tab2;
    uint32_t seed_log2 = 0, seed2_log2 = 0;
    DevBuf<uint32_t> rc_words;              // the reference read backwards and complemented (scan_items_kernel: reads against the reference)
    struct HalfBufs { DevBuf<uint16_t> pilots; DevBuf<bk::HalfDir> dir; DevBuf<bk::NbEntry> cand; uint32_t m = 1, log2nb = 0, log2p = 0; DevBuf<uint32_t> bits; uint32_t bits_log2 = 0, bits_exact = 0; } half_lo, half_hi;
    DevBuf<uint32_t> slot_of, estat_off, estat;
    DevBuf<bk::SlotRec> slot_rec;
    DevBuf<uint4> ent_files, slot_files, id_own_files, estat_files;
    DevBuf<uint16_t> cell_file;
    DevBuf<uint32_t> slot_alias;
    DevBuf<uint64_t> merged_slots;          // [n_merged_slots][2]: slot | window position << 32, the slot's key
    uint32_t n_merged_slots = 0;
    bool gather_ok = false;                 // IndexView::gather_ok
    DevBuf<uint32_t> id_rest_off, id_rest;
    DevBuf<uint8_t> amb;
    DevBuf<uint16_t> pilots;
    DevBuf<bk::TableSlot> table;
    DevBuf<uint32_t> ent_off, ent_len;
    DevBuf<bk::DevEntry> entries;
    // multi-genome indexes: the LDS window (difference array + Level 1's arrays) sits on the genome the sample looks like
    DevBuf<uint32_t> occ;                   // [n_full][n_files] first occurrence of each reference k-mer in each genome file
    DevBuf<uint32_t> file_cell_lo_d;        // [n_files]
    std::vector<uint32_t> file_cell_lo;     // first cell of each genome file
    // after the pileup (bk_sample_call): sequence geometry
    DevBuf<uint64_t> genome_len, seq_cell, seq_len_d;
    DevBuf<int32_t> seq_first, n_seqs_d;
    std::vector<uint64_t> h_seq_cell, h_seq_len;   // host copies of seq_cell, seq_len_d, seq_first, n_seqs_d (bk_regions_set checks against them)
    std::vector<int32_t> h_seq_first, h_n_seqs;
    std::vector<uint2> h_nonacgt;           // {first cell, end} of every run of reference letters that are not ACGT, ascending (bk_indels_enable)
    int max_seqs_per_file = 0;
    uint64_t max_file_cells = 0;
    uint64_t max_file_cells_idx = 0;        // cells of the genome file with the most (pileup rows)
    // testing aids read at create (a fork sees its parent's values)
    int ablate = 0;   // BK_SCAN_ABLATE (measurement aid): see scan_count_kernel
    int item_v_mode = -1;                   // BK_ITEM_V_MODE: force BinArgs::v_mode
    uint64_t max_launch_records = 0;   // BK_MAX_LAUNCH_RECORDS: split pushes into launches of at most this many records

    bk::IndexView view() const {
        bk::IndexView v{};
        v.kmer_pos = kmer_pos.p; v.pilots = pilots.p; v.m = m; v.log2nb = log2nb; v.log2p = log2p;
        v.kmer_of = kmer_of.p; v.id_rec = id_rec.p; v.dirty_ans = dirty_ans.p; v.cell_flags = cell_flags.p; v.ref_words = ref_words.p; v.cell_codes = cell_codes.p; v.cell_has = cell_has.p; v.cell_clean = cell_clean.p; v.cell_clean3 = cell_clean3.p; v.cell_yf = cell_yf.p; v.cell_yr = cell_yr.p; v.id_at = id_at.p; v.cell_fast = cell_fast.p; v.cell_nat = cell_nat.p; v.cell_natrow = cell_natrow.p; v.cell_blk = cell_blk.p; v.seed_tab = seed_tab.p; v.seed_log2 = seed_log2; v.total_cells = (uint32_t)total_cells; v.n_u = n_u;
        v.n_full = n_full; v.n_prows = n_prows; v.prow_id = prow_id.p; v.prow_t = prow_t.p; v.v_omin = v_omin; v.v_span = v_span; v.v_off = v_off;
        v.lo = bk::HalfView{half_lo.pilots.p, half_lo.dir.p, half_lo.cand.p, half_lo.m, half_lo.log2nb, half_lo.log2p, half_lo.bits.p, half_lo.bits_log2, half_lo.bits_exact};
        v.hi = bk::HalfView{half_hi.pilots.p, half_hi.dir.p, half_hi.cand.p, half_hi.m, half_hi.log2nb, half_hi.log2p, half_hi.bits.p, half_hi.bits_log2, half_hi.bits_exact};
        v.lo_bases = lo_bases; v.slot_of = slot_of.p; v.slot_rec = slot_rec.p; v.ent_files = ent_files.p; v.slot_files = slot_files.p; v.slot_alias = slot_alias.p; v.gather_ok = gather_ok ? 1u : 0u; v.id_own_files = id_own_files.p; v.cell_file = cell_file.p; v.id_rest_off = id_rest_off.p; v.id_rest = id_rest.p; v.estat_files = estat_files.p; v.amb = amb.p; v.estat_off = estat_off.p; v.estat = estat.p;
        v.table = table.p; v.ent_off = ent_off.p; v.ent_len = ent_len.p;
        v.entries = entries.p; v.n_slots = n_slots; v.log2s = log2s; v.k = k; v.wstart = wstart; v.W = W; v.n_files = n_files;
        return v;
    }
};

// Builds `tab` (all but d_view, which the caller uploads last) from a validated index on the current device; the laps of `pc`
// time its stages.  BK_OK or the error code, with bk_last_error set.
int build_index_tables(const bk_index_desc* ix, const bk_params* prm, IndexTables& tab, PhaseClock& pc);

// One mate file's counter plane and what a sample keeps beside it (bk_engine::mate).  The plane's states, and what moves it:
//   stale    it may hold an earlier sample (begin_sample).  zero_if_stale makes it current at the mate file's first push, pointer,
//            transport or finalize pass, zeroing it only when it is `used`.
//   used     counters may be non-zero: a push or a transport wrote it (written), or a caller holds it (handed_out).  A finalize of
//            the whole sample leaves it all zero (finalized_clean: dense planes by K2a and the E part's zeroing, sparse planes by
//            clear_touched); a sharded or abandoned sample leaves it used for the next zero_if_stale.
//   v_clean  the V part is known all zero (zero_if_stale): the sample's first bin_count launch stores where it would add
//            (take_v_clean); a caller's pointer (handed_out) clears it.
// Fuse (bk_finalize_lean.hip): the V items of the mate file's first scan launch wait (bk_engine::pending) for the regional finalize,
// which takes its counts from them; Level 2 notes the V rows it writes meanwhile in fuse_touch (items_wait).  A second launch sends
// the items to the plane first (flush_pending_items) and the mate file waits no more in this sample (no_more_waiting).  The regional
// finalize clears the rows it read (items_taken); begin_sample clears what an unfinalized sample left.
struct MatePlane {
    DevBuf<unsigned long long> counters;
    DevBuf<unsigned int> touch_v, touch_b, touch_p, touch_e, v_list, p_list, e_list, n_list;   // sparse planes: touch bitmaps, finalize's lists
    DevBuf<unsigned int> fuse_touch;        // a bit per V row Level 2 wrote to while the launch's items wait
    DevBuf<unsigned long long> alias_hits;  // gathered votes: the deferred k-mers that reach a bucket through an alias key
    // sharded finalize: the part of the plane the reduce-scatter leaves here, widened to u64 again (bk_shard_received) -- what
    // bk_sample_finalize_shard maps; reduced_shards > 0: it holds part `reduced_shard` of that many for the current sample
    DevBuf<unsigned long long> reduced;
    int reduced_shards = 0, reduced_shard = 0;
    uint64_t pushed_records = 0;            // records pushed packed in this sample (the ASCII pushes tally theirs on the device)
    bool stale = true, used = false, v_clean = false, fuse_off = false, touch_used = false;
    int begin_sample(bk_engine* e);   // (bk_engine.cpp: these two issue work on the engine's stream)
    int zero_if_stale(bk_engine* e);
    void written() { used = true; }
    void handed_out() { used = true; v_clean = false; }   // (the caller may write it: collectives)
    void finalized_clean() { used = false; }
    bool take_v_clean() { const bool c = v_clean; v_clean = false; return c; }
    void items_wait() { touch_used = true; }
    void no_more_waiting() { fuse_off = true; }
    void items_taken() { touch_used = false; }
};

// One engine: its parameters, its stream and all that a sample writes.  The index tables are `ix`, shared with the engine it was
// forked from and its forks.
struct bk_engine {
    bk_params params{};
    std::shared_ptr<const IndexTables> ix;
    DevBuf<unsigned long long> shard_sums;  // sharded finalize: [stats 2*n_files*3 | present 2*n_files | kstats 8 | transport flag]
    MatePlane mate[2];                      // R1, R2
    // sharded finalize, transport of the planes (bk_shard_transport / bk_shard_received): the packed plane of the mate file being
    // exchanged and the part the reduce-scatter leaves here (MatePlane::reduced: the plane itself stays as the scans left it)
    DevBuf<unsigned char> xport_send, xport_recv;
    DevBuf<unsigned long long> xport_flag;  // [0] a packer of this sample met a counter too large for its width, [1] sticky copy after
                                            // the ranks' sums were merged, [2..3] bk_shard_measure: max E count, max |V element|
    bool xport_ever = false;                // some sample of this engine went through bk_shard_transport (bk_sample_download then looks at the flag)
    int device = 0;

    DevBuf<unsigned int> deferred, n_deferred, deferred_mask;
    DevBuf<unsigned long long> deferred_n;   // dense planes: the deferred k-mers' counts (K2a zeroes the counters it reads)
    DevBuf<unsigned int> fin_partials;      // per-workgroup finalize tallies (small genome sets only)
    GrowTable ktab;                         // full_kmer_stats: open-addressing table of non-index-touching k-mers
    DevBuf<unsigned long long> ktab_out;    // [2 mates][2] distinct, kept  + [4] overflow flag + [8 ..] tallies of new keys
    DevBuf<unsigned long long> xchg_keys, xchg_cursors;   // bk_kmer_table_partition: the table's entries grouped by owner rank
    DevBuf<unsigned int> xchg_cnt;
    bool ktab_exchanged = false;            // bk_kmer_table_replace was called in this sample
    std::unique_ptr<Primers> primers;       // bk_primers_set (null: no primers, no launch, no end flags)
    std::unique_ptr<Adapters> adapters;     // bk_adapters_set (null: no adapters, no launch; end flags only if primers are set)
    bool trims() const { return primers || adapters; }   // the records' end flags are wanted
    std::unique_ptr<KmerDump> dump;         // bk_kmer_dump_enable (null: no table, no launch)
    // gathered votes (bk_gather.hip): this engine's voting pass is gather_votes_kernel (sparse planes of a many-genome index)
    bool gather_mode = false;
    DevBuf<unsigned int> row_bits;              // one bit per V row of the reference k-mers: touched by the sample (set by prefix_rows_kernel for voter_table_kernel)
    DevBuf<uint32_t> vote_tab;                  // [n_full][W][8] the voters of every (reference k-mer, window position) of the sample (bk_gather.hip; every genome's rows)
    DevBuf<unsigned int> n_alias_hits;          // [2] (MatePlane::alias_hits)
    static constexpr unsigned int kAliasCap = 1u << 20;
    DevBuf<int> last_sel;                   // pileup_selected_only with gathered votes: the genome whose rows the previous sample wrote (-1: none) -- all that
                                            // the next sample has to zero
    DevBuf<unsigned int> slabs;             // [n_cus][n_lds_bins] workgroup histograms of the last scan launch (scan_count_kernel only)
    // the binned scan (bk_scan_items.hip; dense planes with the window's reference in LDS): the scan workgroups' items and where
    // each bin's segment starts, the overflow list and its fill
    bool use_items = false;
    bk::ItemGeom ig{};
    DevBuf<unsigned short> items, item_tab;
    DevBuf<unsigned short> item_gext;       // [items_max_grid][bins][kItemGCap] the bins' extensions in device memory
    DevBuf<unsigned int> ov;
    DevBuf<unsigned long long> ov_n;
    uint32_t ov_par = 0;                    // parity of the next scan_items launch (which of the two overflow counts it appends to)
    bool fuse_ok = false;                   // the index, planes and parameters admit the fuse (MatePlane; alloc_sample_state)
    struct PendingItems { bool on = false; int mate = 0; bk::BinArgs b{}; } pending;
    DevBuf<unsigned int> n_bits, n_any;     // scan -> Level 2: one bit per k-mer of each record of a launch / per record (bk_kernels.h ScanArgs): the N runs; all zero between launches
    DevBuf<unsigned int> l2_bits;           // Level 2's first pass -> its second: the k-mers looked at one by one, same layout
    DevBuf<unsigned int> l2_any;            // ... one bit per record: its row has bits
    DevBuf<unsigned int> l2_plan;           // one word: the workgroups of level2_kernel that work (ScanArgs::l2_plan)
    DevBuf<uint2> l2_diag;                  // ... and each record's diagonal
    bool sparse = false;                    // sparse planes (large indexes): MatePlane's touch bitmaps and lists
    DevBuf<unsigned long long> pileup;      // 4 planes
    DevBuf<unsigned long long> stats;       // [2][n_files][3]
    DevBuf<unsigned char> present;          // [2][n_files]
    DevBuf<unsigned long long> kstats;      // [2 sets][2][4]: a sample uses the set of its parity (kstats_cur), so that the set of the next
                                            // sample can be zeroed while this one is being counted
    int kstats_par = 0;                     // the current sample's set
    unsigned long long* kstats_cur() const { return kstats.p + kstats_par * 8; }
    unsigned long long* kstats_other() const { return kstats.p + (kstats_par ^ 1) * 8; }
    // The zero ride (bk_engine.cpp, bk_sample_begin): a sample's outputs are zeroed by workgroups of its first Level 2 launch, not by
    // a launch of their own.
    bool zero_owed = false;                 // this sample's pileup, stats, present and n_deferred are not zeroed yet
    bool next_clean = false;                // the other set of kstats is known to be zero
    // bk_push_reads_packed: two staging slots, so that the copy of a batch overlaps the scan of the previous one
    struct StageSlot {
        RecordBufs rec;
        PinnedBuf<uint8_t> h;                   // pinned host copy of the caller's batch (words, then lens, then end flags)
        Event done; bool busy = false;
    } stage[2];
    int next_stage = 0;

    // asynchronous ASCII ingest (bk_push_reads_ascii): pinned staging + device buffers per slot
    struct IngestSlot {
        PinnedBuf<uint8_t> h_bases, h_quals;    // (h_quals, d_quals: bk_push_reads_ascii_qual's quality lines; first use allocates)
        PinnedBuf<unsigned long long> h_off;
        DevBuf<uint8_t> d_bases, d_quals;
        DevBuf<unsigned long long> d_off, d_nrec;
        DevBuf<uint32_t> d_work;               // pack_words_kernel's work list
        RecordBufs rec;                        // what the packer writes (with primers or adapters set, the *_ends_kernel variants of K0)
        Event uploaded, done;
        bool busy = false;
    };
    IngestSlot slots[3];
    // the device pushes' records (device buffers only, ordered by the engine's stream): what the packer makes of a
    // bk_push_reads_ascii*_device batch, and the copy of a bk_push_reads_packed_ends_device batch that is trimmed
    IngestSlot dev_ascii;
    int next_slot = 0;
    hipStream_t copy_stream = nullptr;

    hipStream_t own_stream = nullptr, stream = nullptr;
    bool in_sample = false;
    int finalized_mates = 0;                // mate files of the sample whose finalize was enqueued last (0: none since bk_sample_begin / create)
    // multi-genome indexes: the LDS window (difference array + Level 1's arrays) sits on the genome the sample looks like
    DevBuf<unsigned int> win_votes;         // [n_files]
    DevBuf<uint32_t> win_sel;               // {window's genome file, window's first cell} of the current sample, chosen on the device
    bool win_chosen = false;                // for the current sample

    // after the pileup (bk_sample_call): per-engine scratch and results
    DevBuf<double> call_noise, noise_maf, noise_tbl, noise_sums;   // (get_baseline_noise, the walk taken apart: CallArgs)
    DevBuf<unsigned int> noise_cnt, noise_state;
    DevBuf<bk_call_record> call_records;
    DevBuf<bk_call_summary> call_out;
    DevBuf<bk_call_summary> sel_out;        // pileup_selected_only: the genome selected between the two finalize passes
    bool called = false;                    // bk_sample_call ran for the current sample (call_out.p only says: for some sample)
    // bk_sample_consensus (first use allocates): a letter per cell of the largest genome, the summary; made for the current sample
    DevBuf<uint8_t> cons_letters;
    DevBuf<bk_consensus_summary> cons_out;
    bool cons_made = false;
    bk_consensus_params cons_prm{};         // ... with these parameters
    // bk_sample_minor_alleles (first use allocates): a present mask per cell of the largest genome, the summary; made for the current sample
    DevBuf<uint8_t> minor_masks;
    DevBuf<bk_minor_summary> minor_out;
    bool minor_made = false;
    // bk_sample_consensus_indels (first use allocates): best and ties of every boundary, the accepted events, the summary; made of the
    // current sample's letters as they are (a later bk_sample_consensus or bk_sample_call clears it)
    DevBuf<unsigned int> ci_bounds;         // [2][total_cells + 1] ConsensusIndelArgs::best, ties in this order: zeroed by one memset
    DevBuf<bk_consensus_indel_record> ci_rows;   // [BK_CONSENSUS_INDEL_MAX]
    DevBuf<bk_consensus_indel_summary> ci_out;
    bool ci_made = false;
    std::unique_ptr<Regions> regions;       // bk_regions_set (null: no regions, no launch, no buffers)
    bool regions_made = false;              // bk_sample_region_depths ran for the current sample and table
    std::unique_ptr<Indels> indels;         // bk_indels_enable (null: no table, no launch, no buffers)
    std::unique_ptr<Junctions> junctions;   // bk_junctions_enable (null: no table, no launch, no buffers)
    std::unique_ptr<Copybacks> copybacks;   // bk_copybacks_enable (null: no table, no launch, no buffers)
    std::unique_ptr<Chimeras> chimeras;     // bk_chimeras_enable (null: no table, no launch, no buffers)
    std::unique_ptr<Breakends> breakends;   // bk_breakends_enable (null: no table, no launch, no buffers)
    std::unique_ptr<Duplications> duplications;   // bk_duplications_enable (null: no table, no launch, no buffers)
    // the six event passes in the order they begin a sample and ride behind a scan (null: not enabled)
    std::array<EventPass*, 6> event_passes() const { return {indels.get(), junctions.get(), copybacks.get(), chimeras.get(), breakends.get(), duplications.get()}; }
    std::unique_ptr<Linkage> linkage;       // bk_link_enable (null: no row store, no launch, no buffers)
    std::weak_ptr<AnchorTables> anchors;    // the anchor tables while any of the seven features holds them
    std::unique_ptr<Cohort> cohort;         // bk_cohort_set (null: no cohort, no launch, no buffers)
    DevBuf<unsigned long long> dbg;   // BK_L2_STATS (testing build): tallies of what the scan leaves to Level 2
    bool timing = false;
    unsigned timing_kinds = 0xfu, timing_every = 1, timing_seen[4] = {0, 0, 0, 0};
    std::vector<TimedSpan> spans;
    std::vector<hipEvent_t> free_events;

    hipEvent_t get_event() {
        if (!free_events.empty()) { hipEvent_t e = free_events.back(); free_events.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    struct Span {
        bk_engine* e; int kind; hipEvent_t a = nullptr;
        Span(bk_engine* eng, int k) : e(eng), kind(k) {
            if (e->timing && (e->timing_kinds >> k) & 1 && e->timing_seen[k]++ % e->timing_every == 0) { a = e->get_event(); (void)hipEventRecord(a, e->stream); }
        }
        ~Span() {
            if (a) { hipEvent_t b = e->get_event(); (void)hipEventRecord(b, e->stream); e->spans.push_back({a, b, kind}); }
        }
    };
};

// The scan of a batch of records and all that follows it on the engine's stream (bk_engine.cpp); every push of bk_ingest.cpp ends here
int push_device(bk_engine* e, int mate, const Records& r);

// `count` elements from the device to the host on the engine's stream, waited for
template <class T>
int download(bk_engine* e, T* host_dst, const void* dev_src, size_t count) {
    BK_HIP(hipMemcpyAsync(host_dst, dev_src, count * sizeof(T), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    return BK_OK;
}

#pragma GCC visibility pop
