// call_run.cpp -- one `bronko call` behind its checked arguments: the index, the engines on the GPUs, the lanes that whole samples
// are dealt to (or one sample over several GPUs), and the per-sample code (reference: src/call.rs:151-402, per-sample orchestration).
// The k-mer counting + map_kmers stages of the per-sample loop run on the GPU through the C ABI of include/bronko_hip.h; everything
// else here is host code.  A per-sample report is one unit here: the six anchor passes a description each, over which
// every stage of a sample is one template; the other seven a group of functions each (resolve, launch, download, write-and-log).
#include <cerrno>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <tuple>

#include <sys/stat.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h>   // streams and buffers of the one-sample-over-several-GPUs path (RCCL collectives on the engines' streams)
#include <rccl/rccl.h>

#include "reads.hpp"

namespace bronko {
namespace {

const char* const T = "bronko::call";

struct Engine {
    bk_engine* e = nullptr;
    ~Engine() { if (e) bk_engine_destroy(e); }
};

// ---- one sample over several GPUs (BASELINE config 4: one 200 M-read sample, eight GPUs) ---------------------
// The reads' batches are dealt to one engine per GPU; what is additive -- the k-mer occurrence counter planes -- is
// reduce-scattered by RCCL over xGMI on the engines' own streams (the engine packs a plane to 16- or 32-bit elements first,
// bk_shard_transport), every GPU maps its part (bk_sample_finalize_shard), and the small results are combined: max of the depth
// planes, sums of the #k-mer planes and of the statistics.  Pileups of read shards are never summed (thresholds and max are not
// linear).  One process, one communicator per device (ncclCommInitAll), collectives grouped over the devices.
void nccl_check(ncclResult_t r, const char* what) {
    if (r != ncclSuccess) die("bronko::call", std::string(what) + ": " + ncclGetErrorString(r));
}
void hipx(hipError_t r, const char* what) {
    if (r != hipSuccess) die("bronko::call", std::string(what) + ": " + hipGetErrorString(r));
}
struct ShardGroup {
    std::vector<int> devices;
    std::vector<bk_engine*> engs;
    std::vector<ncclComm_t> comms;
    std::vector<hipStream_t> streams;
    int n() const { return (int)engs.size(); }
};
// narrowest width at which the reduce-scatter over n ranks is exact (bronko_amd/dist.py::pick_width; include/bronko_hip.h)
int pick_width(uint64_t max_e, uint64_t max_v, int n) {
    if (max_v * (uint64_t)n <= 32767 && max_e < (1ull << 32)) return 16;
    if (std::max(max_e, max_v) * (uint64_t)n <= 2147483647ull) return 32;
    return 64;
}
// between the last push and the finalize of a sample whose batches went to g.engs in turn
void sharded_finalize(ShardGroup& g, int n_mates, uint64_t cells4) {
    const int S = g.n();
    // KMC's distinct / counted k-mer totals (full_kmer_stats): every k-mer that touches no bucket moves to its owner GPU
    {
        std::vector<void*> keys((size_t)S), cnts((size_t)S), rkeys((size_t)S, nullptr), rcnts((size_t)S, nullptr);
        std::vector<std::vector<uint64_t>> off((size_t)S, std::vector<uint64_t>((size_t)S + 1));
        for (int s = 0; s < S; s++) hip_check(bk_kmer_table_partition(g.engs[(size_t)s], S, &keys[(size_t)s], &cnts[(size_t)s], off[(size_t)s].data()), "bk_kmer_table_partition");
        std::vector<uint64_t> n_in((size_t)S, 0);
        for (int r = 0; r < S; r++) for (int s = 0; s < S; s++) n_in[(size_t)r] += off[(size_t)s][(size_t)r + 1] - off[(size_t)s][(size_t)r];
        for (int r = 0; r < S; r++) {
            hipx(hipSetDevice(g.devices[(size_t)r]), "hipSetDevice");
            hipx(hipMalloc(&rkeys[(size_t)r], std::max<uint64_t>(n_in[(size_t)r], 1) * 8), "hipMalloc");
            hipx(hipMalloc(&rcnts[(size_t)r], std::max<uint64_t>(n_in[(size_t)r], 1) * 4), "hipMalloc");
        }
        std::vector<uint64_t> at((size_t)S, 0);   // fill of each receiver
        nccl_check(ncclGroupStart(), "ncclGroupStart");
        for (int s = 0; s < S; s++)
            for (int r = 0; r < S; r++) {
                const uint64_t n = off[(size_t)s][(size_t)r + 1] - off[(size_t)s][(size_t)r], o = off[(size_t)s][(size_t)r];
                if (!n) continue;
                uint64_t* dk = static_cast<uint64_t*>(rkeys[(size_t)r]) + at[(size_t)r];
                uint32_t* dc = static_cast<uint32_t*>(rcnts[(size_t)r]) + at[(size_t)r];
                at[(size_t)r] += n;
                if (s == r) {   // (its own group: a copy on its stream)
                    hipx(hipSetDevice(g.devices[(size_t)s]), "hipSetDevice");
                    hipx(hipMemcpyAsync(dk, static_cast<uint64_t*>(keys[(size_t)s]) + o, n * 8, hipMemcpyDeviceToDevice, g.streams[(size_t)s]), "hipMemcpyAsync");
                    hipx(hipMemcpyAsync(dc, static_cast<uint32_t*>(cnts[(size_t)s]) + o, n * 4, hipMemcpyDeviceToDevice, g.streams[(size_t)s]), "hipMemcpyAsync");
                    continue;
                }
                nccl_check(ncclSend(static_cast<uint64_t*>(keys[(size_t)s]) + o, n, ncclUint64, r, g.comms[(size_t)s], g.streams[(size_t)s]), "ncclSend");
                nccl_check(ncclSend(static_cast<uint32_t*>(cnts[(size_t)s]) + o, n, ncclUint32, r, g.comms[(size_t)s], g.streams[(size_t)s]), "ncclSend");
                nccl_check(ncclRecv(dk, n, ncclUint64, s, g.comms[(size_t)r], g.streams[(size_t)r]), "ncclRecv");
                nccl_check(ncclRecv(dc, n, ncclUint32, s, g.comms[(size_t)r], g.streams[(size_t)r]), "ncclRecv");
            }
        nccl_check(ncclGroupEnd(), "ncclGroupEnd");
        for (int r = 0; r < S; r++) hip_check(bk_kmer_table_replace(g.engs[(size_t)r], rkeys[(size_t)r], rcnts[(size_t)r], n_in[(size_t)r]), "bk_kmer_table_replace");
        for (int r = 0; r < S; r++) {   // (the table was rebuilt from them on the engine's stream)
            hipx(hipSetDevice(g.devices[(size_t)r]), "hipSetDevice");
            hipx(hipStreamSynchronize(g.streams[(size_t)r]), "hipStreamSynchronize");
            hipx(hipFree(rkeys[(size_t)r]), "hipFree"); hipx(hipFree(rcnts[(size_t)r]), "hipFree");
        }
    }
    for (int m = 0; m < n_mates; m++) {
        // the narrowest exact width: the largest E count and |V element| over all GPUs' planes
        uint64_t max_e = 0, max_v = 0;
        std::vector<void*> dmax((size_t)S);
        for (int s = 0; s < S; s++) hip_check(bk_shard_measure(g.engs[(size_t)s], m, &dmax[(size_t)s]), "bk_shard_measure");
        for (int s = 0; s < S; s++) {
            uint64_t mx[2] = {0, 0};
            hipx(hipSetDevice(g.devices[(size_t)s]), "hipSetDevice");
            hipx(hipMemcpyAsync(mx, dmax[(size_t)s], sizeof mx, hipMemcpyDeviceToHost, g.streams[(size_t)s]), "hipMemcpyAsync");
            hipx(hipStreamSynchronize(g.streams[(size_t)s]), "hipStreamSynchronize");
            max_e = std::max(max_e, mx[0]); max_v = std::max(max_v, mx[1]);
        }
        int width = pick_width(max_e, max_v, S);
        std::vector<void*> send((size_t)S), recv((size_t)S);
        uint64_t part_bytes = 0;
        for (int s = 0; s < S; s++) {
            int rc = bk_shard_transport(g.engs[(size_t)s], m, S, width, &send[(size_t)s], &part_bytes, &recv[(size_t)s]);
            if (rc != 0 && width == 16 && s == 0) { width = 32; rc = bk_shard_transport(g.engs[0], m, S, width, &send[0], &part_bytes, &recv[0]); }   // (16 does not shrink this plane at S shards)
            hip_check(rc, "bk_shard_transport");
        }
        const ncclDataType_t dt = width == 64 ? ncclInt64 : ncclInt32;
        const size_t count = (size_t)(part_bytes / (width == 64 ? 8 : 4));
        nccl_check(ncclGroupStart(), "ncclGroupStart");
        for (int s = 0; s < S; s++) nccl_check(ncclReduceScatter(send[(size_t)s], recv[(size_t)s], count, dt, ncclSum, g.comms[(size_t)s], g.streams[(size_t)s]), "ncclReduceScatter");
        nccl_check(ncclGroupEnd(), "ncclGroupEnd");
        for (int s = 0; s < S; s++) hip_check(bk_shard_received(g.engs[(size_t)s], m, s, S, width), "bk_shard_received");
    }
    for (int s = 0; s < S; s++) hip_check(bk_sample_finalize_shard(g.engs[(size_t)s], n_mates, s, S), "bk_sample_finalize_shard");
    // the small results: depth = max, #k-mers and statistics add up
    std::vector<void*> pile((size_t)S), sums((size_t)S);
    uint64_t n_sums = 0;
    for (int s = 0; s < S; s++) {
        hip_check(bk_pileup_device_ptr(g.engs[(size_t)s], &pile[(size_t)s]), "bk_pileup_device_ptr");
        hip_check(bk_shard_sums_device_ptr(g.engs[(size_t)s], &sums[(size_t)s], &n_sums), "bk_shard_sums_device_ptr");
    }
    nccl_check(ncclGroupStart(), "ncclGroupStart");
    for (int s = 0; s < S; s++) {
        uint64_t* p = static_cast<uint64_t*>(pile[(size_t)s]);
        nccl_check(ncclAllReduce(p, p, (size_t)(2 * cells4), ncclUint64, ncclMax, g.comms[(size_t)s], g.streams[(size_t)s]), "ncclAllReduce");
        nccl_check(ncclAllReduce(p + 2 * cells4, p + 2 * cells4, (size_t)(2 * cells4), ncclUint64, ncclSum, g.comms[(size_t)s], g.streams[(size_t)s]), "ncclAllReduce");
        nccl_check(ncclAllReduce(sums[(size_t)s], sums[(size_t)s], (size_t)n_sums, ncclUint64, ncclSum, g.comms[(size_t)s], g.streams[(size_t)s]), "ncclAllReduce");
    }
    nccl_check(ncclGroupEnd(), "ncclGroupEnd");
    for (int s = 0; s < S; s++) hip_check(bk_sample_merge_shards(g.engs[(size_t)s]), "bk_sample_merge_shards");
}

void ensure_output_dir(const std::string& out) {
    if (mkdir(out.c_str(), 0777) != 0 && errno != EEXIST) {
        // create_dir_all: create missing parents too
        std::string partial;
        for (size_t i = 0; i <= out.size(); i++) {
            if (i == out.size() || out[i] == '/') { if (!partial.empty()) mkdir(partial.c_str(), 0777); }
            if (i < out.size()) partial += out[i];
        }
        struct stat st;
        if (stat(out.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) die(T, "Unable to create outputs in output directory 2");
    }
}

// ---- engines and lanes ---------------------------------------------------------------------------------------------------------
// decoded index -> GPU engine(s) (include/bronko_hip.h).  Samples are independent (call.rs:212 / :297 handle them one after
// the other), so whole samples are dealt to *lanes* in turn -- no collective.  A lane is a host thread that ingests its
// samples (gunzip + parse are host work: ~1 M reads/s per FASTQ file, a thousand times slower than the scan behind them)
// into its own pair of engines; the lanes of one device share that device's tables (bk_engine_fork), every device holds
// its own copy.  BRONKO_DEVICES=0,1,.. names the devices (default: all visible ones; naming a device twice doubles its
// lanes), BRONKO_DEVICE=d the single device of earlier versions, BRONKO_LANES=n the lanes per device (default: -t / 2
// over the devices, at most 16 -- a 256-thread host inflates 8 gzip streams side by side at full speed and 32 at half --
// and no more than fit six tenths of the device's free memory: a lane keeps two samples'
// counter planes there -- 0.2 GB for one SARS-CoV-2 genome, 9 GB for a hundred at k = 31).
struct Lane { int device = 0; int parent = -1; Engine eng, fork; std::vector<size_t> mine; };   // parent: the lane whose engine built the device's tables
// the first engine of every device named: its tables, and what a sample's state weighs (dev: -1 where the device was named before)
struct FirstEngines { std::vector<Engine> eng; std::vector<int> dev; };

std::vector<int> devices_from_env() {
    std::vector<int> devices;
    if (const char* dl = getenv("BRONKO_DEVICES")) {
        for (const char* q = dl; *q;) {
            char* end = nullptr;
            const long d = strtol(q, &end, 10);
            if (end == q) break;
            devices.push_back((int)d);
            q = *end == ',' ? end + 1 : end;
        }
    } else if (const char* dv = getenv("BRONKO_DEVICE")) {
        devices.push_back(atoi(dv));
    } else {
        const int nd = bk_device_count();
        for (int d = 0; d < std::max(nd, 1); d++) devices.push_back(d);
    }
    if (devices.empty()) devices.push_back(0);
    return devices;
}

// Fewer samples than GPUs (BASELINE config 4: ONE 200 M-read sample, eight GPUs): a sample's batches are dealt to all of them and
// the counter planes are reduce-scattered by RCCL (sharded_finalize above).  BRONKO_SHARD=1 / 0 forces / forbids it (1 with a single
// GPU runs every collective on a communicator of one rank).  The shard count is a power of two (it divides 64).
// Returns the GPUs a sample is sharded over; none: whole samples go to lanes.
std::vector<const char*> one_file_reports(const CallConfig& cfg);   // (below, with the report units)
std::vector<int> plan_shards(const Args& a, const CallConfig& cfg, const std::vector<int>& devices, size_t n_samples) {
    std::vector<int> shard_devices;
    for (int d : devices) if (std::find(shard_devices.begin(), shard_devices.end(), d) == shard_devices.end()) shard_devices.push_back(d);
    bool shard_mode = shard_devices.size() >= 2 && n_samples < shard_devices.size();
    if (const char* sh = getenv("BRONKO_SHARD")) shard_mode = atoi(sh) != 0;
    // (the k-mer counts of a sample are one engine's, and so are its events, span arrays and row store: whole samples go to the GPUs in turn)
    std::vector<const char*> whole = one_file_reports(cfg);
    if (a.keep_kmer_info) whole.insert(whole.begin(), "--keep-kmer-info");
    if (shard_mode && !whole.empty()) {
        LOG_DEBUG(T, std::string(whole[0]) + ": samples are not sharded over GPUs, each sample's reads go to one GPU");
        shard_mode = false;
    }
    { size_t S = 1; while (S * 2 <= std::min<size_t>(shard_devices.size(), 64)) S *= 2; shard_devices.resize(S); }
    if (!shard_mode) shard_devices.clear();
    return shard_devices;
}

void release_lanes(std::vector<Lane>& lanes) {
    // (forks go before the engine they were forked from; side by side: releasing dozens of engines one after the other takes a second)
    std::vector<std::thread> th;
    for (auto& ln : lanes)
        if (ln.parent >= 0 && ln.eng.e) th.emplace_back([&ln] { bk_engine_destroy(ln.eng.e); ln.eng.e = nullptr; });
    for (auto& t : th) t.join();
}

// ---- the per-sample report units ---------------------------------------------------------------------------------------------------
// One table of a sample's rows as a report brings it back from the device: its summary and its rows, in the host's struct
template <class Summ, class Row>
struct Rows { Summ summ{}; std::vector<Row> rows; };

// ... by a first download for the summary, of which `count` is the rows' number, then that many rows.  Row is the host's struct for
// the engine's record Rec
template <class Summ, class Rec, class Row>
void download_rows(bk_engine* e, int (*download)(bk_engine*, Summ*, Rec*, uint64_t), const char* name, Rows<Summ, Row>& t, const uint64_t& count) {
    static_assert(sizeof(Row) == sizeof(Rec), "the host's struct is the engine's record");
    hip_check(download(e, &t.summ, nullptr, 0), name);
    t.rows.resize((size_t)count);
    hip_check(download(e, &t.summ, reinterpret_cast<Rec*>(t.rows.data()), t.rows.size()), name);
}

constexpr uint32_t kHapTableLog2 = 16, kHapTableLog2Max = 24;   // --haplotypes: the table's first size (768 KB + 2.5 MB of entries); four times as many slots after each that was full
constexpr uint64_t kLinkInitialRows = 1ull << 20;   // --linkage: first capacity of an engine's row store (32 MB; it doubles as a sample needs)
constexpr uint32_t kEventTableLog2 = 18;  // the anchor passes: slots of an engine's event table (a sample with more distinct candidate events is an error)
constexpr uint32_t kDumpTableLog2 = 24;   // --keep-kmer-info: first capacity of an engine's k-mer count table

// The six anchor passes, one description each (the engine's side of them: bk_riders.cpp): the pass's C types and the host's row, its
// three entry points with their names for hip_check, its switch, config and params out of CallConfig, its option (an index of one
// genome file; no sharding), its file's suffix, its log sentence and its writer.  The stages of CallRun are one template each over these.
#define BK_PASS(noun, Row_, switch_, enable_, report_, download_)                                                                                      \
    using Config = bk_##noun##_config; using Params = bk_##noun##_params; using Summary = bk_##noun##_summary; using Row = Row_;                   \
    static constexpr auto enable = enable_, report = report_; static constexpr auto download = download_;                                       \
    static constexpr const char *enable_name = #enable_, *report_name = #report_, *download_name = #download_;                                     \
    static bool on(const CallConfig& c) { return c.switch_; }
inline std::string num(uint64_t x) { return std::to_string(x); }
struct IndelPass {
    BK_PASS(indel, IndelEvent, indels, bk_indels_enable, bk_sample_indels, bk_sample_download_indels);
    static constexpr const char *option = "--indels", *suffix = ".indels.vcf";
    static Config config(const CallConfig& c) { return {c.indel.max_len, c.indel.max_mismatches, kEventTableLog2}; }
    static Params params(const CallConfig& c) { return {c.indel.min_reads, c.indel.min_af_ppm}; }
    static std::string sentence(const Summary& s) {
        return "Indels: " + num(s.anchored) + " of " + num(s.records) + " records anchored, " + num(s.ref_spanning) + " reference-spanning, " + num(s.supporting) +
               " supporting, " + num(s.candidates) + " candidate events, " + num(s.reported) + " reported";
    }
    static void write(const std::string& path, const std::string& reads, const Index& ix, int best, const Rows<Summary, Row>& t, const CallConfig& c) { write_indels_vcf(path, reads, ix, best, t.rows, c.indel); }
};
struct JunctionPass {
    BK_PASS(junction, JunctionEvent, junctions, bk_junctions_enable, bk_sample_junctions, bk_sample_download_junctions);
    static constexpr const char *option = "--junctions", *suffix = ".junctions.tsv";
    static Config config(const CallConfig& c) { return {c.junction.min_len, c.junction.max_mismatches, kEventTableLog2}; }
    static Params params(const CallConfig& c) { return {c.junction.min_reads}; }
    static std::string sentence(const Summary& s) {
        return "Junctions: " + num(s.anchored) + " of " + num(s.records) + " records anchored, " + num(s.ref_spanning) + " reference-spanning, " + num(s.supporting) +
               " supporting, " + num(s.short_) + " short, " + num(s.backward) + " backward, " + num(s.discordant) + " discordant, " + num(s.candidates) +
               " candidate junctions, " + num(s.reported) + " reported";
    }
    static void write(const std::string& path, const std::string&, const Index& ix, int best, const Rows<Summary, Row>& t, const CallConfig& c) { write_junctions_tsv(path, ix, best, t.rows, c.junction); }
};
struct CopybackPass {
    BK_PASS(copyback, CopybackEvent, copybacks, bk_copybacks_enable, bk_sample_copybacks, bk_sample_download_copybacks);
    static constexpr const char *option = "--copybacks", *suffix = ".copybacks.tsv";
    static Config config(const CallConfig& c) { return {c.copyback.max_mismatches, kEventTableLog2}; }
    static Params params(const CallConfig& c) { return {c.copyback.min_reads, c.copyback.min_dist}; }
    static std::string sentence(const Summary& s) {
        return "Copy-backs: " + num(s.records) + " records, " + num(s.same_strand) + " on one strand, " + num(s.ref_spanning) + " reference-spanning, " + num(s.switched) +
               " switched, " + num(s.supporting) + " supporting, " + num(s.discordant) + " discordant, " + num(s.candidates) + " candidate copy-backs, " + num(s.reported) +
               " reported";
    }
    static void write(const std::string& path, const std::string&, const Index& ix, int best, const Rows<Summary, Row>& t, const CallConfig& c) { write_copybacks_tsv(path, ix, best, t.rows, c.copyback); }
};
struct ChimeraPass {   // (a genome file of one sequence: the headers alone)
    BK_PASS(chimera, ChimeraEvent, chimeras, bk_chimeras_enable, bk_sample_chimeras, bk_sample_download_chimeras);
    static constexpr const char *option = "--chimeras", *suffix = ".chimeras.tsv";
    static Config config(const CallConfig& c) { return {c.chimera.max_mismatches, kEventTableLog2}; }
    static Params params(const CallConfig& c) { return {c.chimera.min_reads}; }
    static std::string sentence(const Summary& s) {
        return "Chimeras: " + num(s.records) + " records, " + num(s.same_strand) + " on one strand of one sequence, " + num(s.ref_spanning) + " reference-spanning, " +
               num(s.crossed) + " crossed, " + num(s.supporting) + " supporting, " + num(s.discordant) + " discordant, " + num(s.candidates) + " candidate chimeras, " +
               num(s.reported) + " reported";
    }
    static void write(const std::string& path, const std::string&, const Index& ix, int best, const Rows<Summary, Row>& t, const CallConfig& c) { write_chimeras_tsv(path, ix, best, t.rows, c.chimera, t.summ.supporting, t.summ.ref_spanning); }
};
struct BreakendPass {
    BK_PASS(breakend, BreakendEvent, breakends, bk_breakends_enable, bk_sample_breakends, bk_sample_download_breakends);
    static constexpr const char *option = "--breakends", *suffix = ".breakends.tsv";
    static Config config(const CallConfig& c) { return {c.breakend.min_clip, c.breakend.max_mismatches, kEventTableLog2}; }
    static Params params(const CallConfig& c) { return {c.breakend.min_reads}; }
    static std::string sentence(const Summary& s) {
        return "Breakends: " + num(s.records) + " records, " + num(s.one_anchor) + " with one anchor, " + num(s.ref_spanning) + " reference-spanning, " + num(s.supporting) +
               " supporting, " + num(s.short_) + " short, " + num(s.through) + " through, " + num(s.discordant) + " discordant, " + num(s.unplaced) + " unplaced, " +
               num(s.candidates) + " candidate breakends, " + num(s.reported) + " reported";
    }
    static void write(const std::string& path, const std::string&, const Index& ix, int best, const Rows<Summary, Row>& t, const CallConfig& c) {
        const Summary& s = t.summ;
        BreakendTallies bt;
        bt.records = s.records; bt.one_anchor = s.one_anchor; bt.ref_spanning = s.ref_spanning; bt.supporting = s.supporting; bt.short_ = s.short_;
        bt.through = s.through; bt.discordant = s.discordant; bt.unplaced = s.unplaced; bt.candidates = s.candidates; bt.reported = s.reported;
        write_breakends_tsv(path, ix, best, t.rows, c.breakend, bt);
    }
};
struct DuplicationPass {
    BK_PASS(duplication, DuplicationEvent, duplications, bk_duplications_enable, bk_sample_duplications, bk_sample_download_duplications);
    static constexpr const char *option = "--duplications", *suffix = ".duplications.tsv";
    static Config config(const CallConfig& c) { return {c.duplication.min_len, c.duplication.max_mismatches, kEventTableLog2}; }
    static Params params(const CallConfig& c) { return {c.duplication.min_reads}; }
    static std::string sentence(const Summary& s) {
        return "Duplications: " + num(s.anchored) + " of " + num(s.records) + " records anchored, " + num(s.ref_spanning) + " reference-spanning, " + num(s.supporting) +
               " supporting, " + num(s.short_) + " short, " + num(s.forward) + " forward, " + num(s.discordant) + " discordant, " + num(s.candidates) +
               " candidate duplications, " + num(s.reported) + " reported";
    }
    static void write(const std::string& path, const std::string&, const Index& ix, int best, const Rows<Summary, Row>& t, const CallConfig& c) { write_duplications_tsv(path, ix, best, t.rows, c.duplication); }
};
using AnchorPasses = std::tuple<IndelPass, JunctionPass, CopybackPass, ChimeraPass, BreakendPass, DuplicationPass>;   // as they launch and are written
template <class F>
void each_anchor_pass(F&& f) { std::apply([&](auto... p) { (f(p), ...); }, AnchorPasses{}); }   // f(P{}) for every pass P, in that order
template <class P> using PassRows = Rows<typename P::Summary, typename P::Row>;
template <class... P> std::tuple<PassRows<P>...> rows_of(std::tuple<P...>);

// the reports that count a sample's reads against the cells of one genome file (a k-mer's cell in the engine's table is its first among
// all files, not the selected genome's), on the one engine that holds their tables: the options that are on, in the order they are named
std::vector<const char*> one_file_reports(const CallConfig& cfg) {
    std::vector<const char*> on;
    each_anchor_pass([&](auto p) { if (p.on(cfg)) on.push_back(p.option); });
    if (cfg.linkage) on.push_back("--linkage");
    if (cfg.codons()) on.push_back("--codons");
    if (cfg.haps()) on.push_back("--haplotypes");
    if (cfg.read_pileup) on.push_back("--read-pileup");
    return on;
}

// what a sample's completion brings back from the device
struct SampleData {
    Pileup p;                                             // depth planes under --pileup; stats and present summed over the mates
    std::vector<uint64_t> stats, kstats;                  // per mate file
    std::vector<uint8_t> present;
    bk_call_summary summ{};
    std::vector<bk_call_record> recs;
    Rows<bk_consensus_summary, uint8_t> consensus;        // --consensus: the letters
    Rows<bk_consensus_indel_summary, ConsensusIndel> cons_indels;   // --consensus-indels
    Rows<bk_minor_summary, uint8_t> minor;                // --contamination: the present masks
    Rows<bk_region_summary, bk_region_depth> regions;     // --regions, --region-window
    decltype(rows_of(AnchorPasses{})) events;             // the anchor passes: a PassRows<P> each
    Rows<bk_link_summary, LinkPair> linkage;              // --linkage
    std::vector<LinkSite> link_sites;                     // ... and the sample's VCF records its pairs are of
    Rows<bk_codon_summary, uint32_t> codons;              // --codons: 64 counts a codon
    bk_hap_summary hap_summ{};                            // --haplotypes
    HapTable hap_table;
    Rows<bk_read_pileup_summary, ReadPileupCell> read_pileup;   // --read-pileup
};

struct CallRun {
    const Args& a;
    const CallConfig& cfg;
    std::vector<std::vector<std::string>> samples;   // in input order
    std::unique_ptr<ReadAhead> ahead;                // (reads `samples` and `cfg`: declared behind them)
    Index ix;
    std::vector<OverviewRow> overview;               // by sample, in input order
    std::vector<SampleCalls> all_calls;              // --alignment
    std::vector<std::vector<uint8_t>> cohort_letters;   // --distances: by sample, its consensus letters (n x positions bytes of host memory in all)
    std::vector<int> cohort_genome;                  // ... and the genome file it selected (-1: none)
    std::vector<std::vector<uint8_t>> cohort_masks;  // --contamination: by sample, its present masks (n x positions more bytes)
    int dump_threads = 1;                            // --keep-kmer-info: threads that format one sample's counts (set before the lanes start)

    // the samples, in input order; their files are read ahead from here on (ReadAhead): the index and the engine's tables take
    // seconds to make with many genomes, and a lane's next sample need not wait for its previous one's reads
    CallRun(const Args& args, const CallConfig& config) : a(args), cfg(config) {
        for (const auto& r : a.reads) samples.push_back({r});
        for (size_t i = 0; i < a.first_pairs.size(); i++) samples.push_back({a.first_pairs[i], a.second_pairs[i]});
        overview.resize(samples.size());
        if (a.alignment) all_calls.resize(samples.size());
        if (a.distances) { cohort_letters.resize(samples.size()); cohort_genome.assign(samples.size(), -1); }
        if (a.contamination) cohort_masks.resize(samples.size());
        if (!getenv("BRONKO_NO_READ_AHEAD")) {
            const uint64_t ram = (uint64_t)sysconf(_SC_PHYS_PAGES) * (uint64_t)sysconf(_SC_PAGE_SIZE);
            ahead.reset(new ReadAhead(samples, cfg, (unsigned)std::max<long>(2, a.threads / 8), std::min<uint64_t>(ram / 4, 32ull << 30)));
        }
    }

    void open_index() {
        if (a.has_genomes()) {                                            // call.rs:170-178
            LOG_INFO(T, "Creating bronko index from provided reference genomes");
            try { ix = build_index_any(T, (int)a.kmer, a.genomes, (int)a.threads); }
            catch (const std::exception& e) { die(T, std::string(e.what()) + " | Reference failed to build"); }
        } else {                                                        // call.rs:179-200
            LOG_INFO(T, "Reading in provided bronko index");
            try { ix = load_index(a.db); }
            catch (const std::exception& e) { die(T, e.what()); }
            if (ix.k != a.kmer)   // (the readers may have packed with -k before the database was read)
                die(T, "Database k is not the same as provided, please set -k to " + std::to_string(ix.k) + " or build a new index");
        }
        // (a few genomes: the engine's tables are made in a fraction of a second, the cores are the readers' from here on; with many
        // the readers stay few until the engines stand -- bk_engine_create runs on all cores for seconds)
        if (ahead && ix.files.size() <= 8) ahead->set_concurrency((unsigned)std::max<long>(2, a.threads / 2));
        regions_resolve();   // every report's BED lines meet the CHROM tokens of the index here, before any device is touched
        for (const char* opt : one_file_reports(cfg))
            if (ix.files.size() != 1) die(T, std::string(opt) + " needs an index of one genome file, this one has " + std::to_string(ix.files.size()));
        codons_resolve();
        haps_resolve();
    }

    // ---- the other seven reports, a group of functions each: what open_index resolves for it, its launch, its download and its
    // write-and-log, side by side.  The stages below call them in a fixed order; `base` is <DIR>/<stem>, `best` the selected genome file.
    // --consensus: on the device, behind the calls; only the letters travel
    void consensus_launch(bk_engine* e) const { if (a.consensus) hip_check(bk_sample_consensus(e, &cfg.consensus), "bk_sample_consensus"); }
    void consensus_download(bk_engine* e, uint64_t longest, SampleData& d) const {
        if (!a.consensus) return;
        d.consensus.rows.resize((size_t)longest);
        hip_check(bk_sample_download_consensus(e, &d.consensus.summ, d.consensus.rows.data(), d.consensus.rows.size()), "bk_sample_download_consensus");
    }
    void consensus_write(const std::string& base, const std::string& stem, int best, const SampleData& d) const {
        if (!a.consensus) return;
        const bk_consensus_summary& c = d.consensus.summ;
        LOG_INFO(T, "Consensus of " + num(c.positions) + " positions: " + num(c.called) + " called (" + num(c.substitutions) + " substitutions), " + num(c.ambiguous) +
                        " ambiguous, " + num(c.masked) + " masked");
        if (!a.consensus_indels) write_consensus_fasta(base + ".consensus.fa", stem, ix, best, d.consensus.rows.data(), c.positions);
    }
    // --contamination: the present masks, on the device, behind the consensus; only the bytes travel
    void minor_launch(bk_engine* e) const { if (a.contamination) hip_check(bk_sample_minor_alleles(e, &cfg.minor), "bk_sample_minor_alleles"); }
    void minor_download(bk_engine* e, uint64_t longest, SampleData& d) const {
        if (!a.contamination) return;
        d.minor.rows.resize((size_t)longest);
        hip_check(bk_sample_download_minor_alleles(e, &d.minor.summ, d.minor.rows.data(), d.minor.rows.size()), "bk_sample_download_minor_alleles");
    }
    void minor_log(const SampleData& d) const {
        if (a.contamination) LOG_INFO(T, "Minor alleles: " + num(d.minor.summ.mixed) + " mixed positions, " + num(d.minor.summ.present) + " bases present");
    }
    // --consensus-indels: the indels join the letters where both lie; the few accepted events travel
    void consensus_indels_launch(bk_engine* e) const { if (a.consensus_indels) hip_check(bk_sample_consensus_indels(e), "bk_sample_consensus_indels"); }
    void consensus_indels_download(bk_engine* e, SampleData& d) const {
        if (a.consensus_indels) download_rows(e, bk_sample_download_consensus_indels, "bk_sample_download_consensus_indels", d.cons_indels, d.cons_indels.summ.accepted);
    }
    // (the letters came with '-' at the applied deletions; a sample without accepted events: the header lines alone)
    void consensus_indels_write(const std::string& base, const std::string& stem, int best, const SampleData& d) const {
        if (!a.consensus_indels) return;
        const bk_consensus_indel_summary& s = d.cons_indels.summ;
        LOG_INFO(T, "Consensus indels: " + num(s.accepted) + " of " + num(s.candidates) + " candidate events accepted, " + num(s.applied) + " applied (" + num(s.deletions) +
                        " deletions of " + num(s.deleted_bases) + " bases, " + num(s.insertions) + " insertions of " + num(s.inserted_bases) + " bases, " +
                        num(s.frameshifts) + " frameshifts), " + num(s.contested) + " contested");
        write_consensus_indels_fasta(base + ".consensus.fa", stem, ix, best, d.consensus.rows.data(), d.consensus.summ.positions, d.cons_indels.rows);
        write_consensus_indels_tsv(base + ".consensus_indels.tsv", ix, best, d.cons_indels.rows, cfg.consensus.min_depth, cfg.consensus.min_freq);
    }
    // --regions: the BED lines against the index; --region-window: the tiling; a few numbers per region travel
    std::vector<Region> regions;         // every genome file's
    std::vector<bk_region> region_table;         // ... as bk_regions_set takes them (every engine that completes a sample holds them)
    size_t max_file_regions = 0;          // regions of the genome file with the most
    void regions_resolve() {
        if (!cfg.region_report()) return;
        try { regions = cfg.region_window ? window_regions(ix, cfg.region_window) : resolve_bed(ix, cfg.bed, cfg.regions_path); }
        catch (const std::exception& e) { die(T, e.what()); }
        std::vector<size_t> per_file(ix.files.size(), 0);
        for (const Region& g : regions) {
            region_table.push_back(bk_region{g.file_id, g.seq, g.start, g.end});
            max_file_regions = std::max(max_file_regions, ++per_file[(size_t)g.file_id]);
        }
        LOG_DEBUG(T, num(regions.size()) + " regions over " + num(ix.files.size()) + " genome file(s)");
    }
    void regions_set(bk_engine* e) const { if (!region_table.empty()) hip_check(bk_regions_set(e, region_table.data(), region_table.size()), "bk_regions_set"); }
    void regions_launch(bk_engine* e) const { if (!region_table.empty()) hip_check(bk_sample_region_depths(e, cfg.region_min_depth), "bk_sample_region_depths"); }
    void regions_download(bk_engine* e, SampleData& d) const {
        if (region_table.empty()) return;
        d.regions.rows.resize(max_file_regions);
        hip_check(bk_sample_download_region_depths(e, &d.regions.summ, d.regions.rows.data(), d.regions.rows.size()), "bk_sample_download_region_depths");
        d.regions.rows.resize(std::min<size_t>(d.regions.rows.size(), d.regions.summ.n_regions));
    }
    void regions_write(const std::string& base, int best, const SampleData& d) const {   // (a genome without a region: the two header lines)
        if (!cfg.region_report()) return;
        const bk_region_summary& s = d.regions.summ;
        LOG_INFO(T, "Depth of " + num(s.n_regions) + " regions at minimum depth " + num(cfg.region_min_depth) + ": " + num(s.full) + " full, " + num(s.partial) +
                        " partial, " + num(s.empty) + " empty");
        std::vector<RegionDepth> rows;
        for (const bk_region_depth& g : d.regions.rows) { RegionDepth o; o.sum = g.sum; o.min = g.min; o.max = g.max; o.median = g.median; o.covered = g.covered; rows.push_back(o); }
        write_regions_tsv(base + ".regions.tsv", ix, best, regions, rows.data(), rows.size(), cfg.region_min_depth);
    }
    // --linkage: the sites are the sample's own VCF records, so it is counted once the calls are down; a few rows travel
    void linkage_count(bk_engine* e, SampleData& d) const {
        if (!cfg.linkage) return;
        const FileMeta& fm = ix.files[0];     // (one genome file: checked as the index was opened)
        std::vector<uint64_t> seq_cell(fm.sequences.size(), 0);
        for (size_t q = 1; q < fm.sequences.size(); q++) seq_cell[q] = seq_cell[q - 1] + fm.sequences[q - 1].len;
        for (uint64_t i = 0; i < std::min<uint64_t>(d.summ.n_records, d.recs.size()); i++) {
            const bk_call_record& c = d.recs[i];
            LinkSite s;
            s.cell = (uint32_t)(seq_cell[(size_t)c.seq_id] + c.pos - 1); s.ref_base = (uint8_t)c.ref_base; s.alt_base = (uint8_t)c.alt_base;
            d.link_sites.push_back(s);
        }
        const std::vector<uint32_t> sites = link_sites(d.link_sites);
        hip_check(bk_sample_linkage(e, sites.data(), (uint32_t)sites.size(), cfg.link.max_dist), "bk_sample_linkage");
        download_rows(e, bk_sample_download_linkage, "bk_sample_download_linkage", d.linkage, d.linkage.summ.n_pairs);
    }
    void linkage_write(const std::string& base, int best, const SampleData& d) const {   // (a sample without such a pair: the header alone)
        if (!cfg.linkage) return;
        const uint64_t lines = write_linkage_tsv(base + ".linkage.tsv", ix, best, d.link_sites, d.linkage.rows, cfg.link);
        LOG_INFO(T, "Linkage: " + num(d.linkage.summ.placed) + " of " + num(d.linkage.summ.records) + " records placed, " + num(d.linkage.summ.n_pairs) +
                        " pairs counted, " + num(lines) + " lines written");
    }
    // --codons: counted from the same rows, behind the calls; 256 bytes a codon travel
    std::vector<CodonGene> genes;             // the BED lines against the index
    std::vector<bk_codon_region> gene_table;       // ... as bk_sample_codons takes them
    void codons_resolve() {
        if (!cfg.codons()) return;
        try { genes = resolve_codon_bed(ix, 0, cfg.codon_bed, cfg.codons_path); }
        catch (const std::exception& e) { die(T, e.what()); }
        for (const CodonGene& g : genes) gene_table.push_back(bk_codon_region{g.reg.cell0, g.reg.n_codons});
        LOG_DEBUG(T, num(genes.size()) + " coding regions");
    }
    void codons_count(bk_engine* e, SampleData& d) const {
        if (!cfg.codons()) return;
        bk_codon_summary& s = d.codons.summ;
        hip_check(bk_sample_codons(e, gene_table.data(), (uint32_t)gene_table.size()), "bk_sample_codons");
        hip_check(bk_sample_download_codons(e, &s, nullptr, 0), "bk_sample_download_codons");
        d.codons.rows.resize((size_t)s.n_codons * 64);
        hip_check(bk_sample_download_codons(e, &s, d.codons.rows.data(), s.n_codons), "bk_sample_download_codons");
    }
    void codons_write(const std::string& base, int best, const SampleData& d) const {   // (a sample without such a triplet: the header alone)
        if (!cfg.codons()) return;
        const uint64_t lines = write_codons_tsv(base + ".codons.tsv", ix, best, genes, d.codons.rows, cfg.codon);
        LOG_INFO(T, "Codons: " + num(d.codons.summ.rows) + " placed records over " + num(d.codons.summ.n_regions) + " regions, " + num(d.codons.summ.n_codons) +
                        " codons counted, " + num(lines) + " lines written");
    }
    // --haplotypes / --hap-window: likewise; a table that was full: the same rows again into one of four times the slots
    std::vector<HapWindow> hap_wins;              // the BED lines against the index, or the tiling
    std::vector<bk_hap_region> hap_regs;          // ... as bk_sample_haplotypes takes them
    void haps_resolve() {
        if (!cfg.haps()) return;
        try { hap_wins = cfg.hap_window ? hap_windows(ix, 0, cfg.hap_window, cfg.hap_step) : resolve_hap_bed(ix, 0, cfg.hap_bed, cfg.haps_path); }
        catch (const std::exception& e) { die(T, e.what()); }
        for (const HapWindow& w : hap_wins) hap_regs.push_back(bk_hap_region{w.reg.cell0, w.reg.len});
        LOG_DEBUG(T, num(hap_wins.size()) + " haplotype regions");
    }
    void haps_count(bk_engine* e, SampleData& d) const {
        if (!cfg.haps()) return;
        bk_hap_summary& s = d.hap_summ;
        d.hap_table.cover.assign(hap_regs.size(), 0u); d.hap_table.ref_count.assign(hap_regs.size(), 0u);
        for (uint32_t log2 = kHapTableLog2;; log2 += 2) {
            hip_check(bk_sample_haplotypes(e, hap_regs.data(), (uint32_t)hap_regs.size(), log2), "bk_sample_haplotypes");
            const int rc = bk_sample_download_haplotypes(e, &s, d.hap_table.cover.data(), d.hap_table.ref_count.data(), nullptr, 0);
            if (rc == BK_ERR_RANGE && log2 + 2 <= kHapTableLog2Max) {
                LOG_INFO(T, "Haplotypes: a table of 2^" + num(s.table_log2) + " slots was full (" + num(s.dropped) + " counts dropped), counting again with four times as many");
                continue;
            }
            hip_check(rc, "bk_sample_download_haplotypes");
            break;
        }
        static_assert(sizeof(HapEntry) == sizeof(bk_hap_entry), "HapEntry is bk_hap_entry");
        d.hap_table.entries.resize((size_t)s.entries);
        hip_check(bk_sample_download_haplotypes(e, &s, nullptr, nullptr, reinterpret_cast<bk_hap_entry*>(d.hap_table.entries.data()), d.hap_table.entries.size()),
                  "bk_sample_download_haplotypes");
    }
    void haps_write(const std::string& base, int best, const SampleData& d) const {   // (a sample without such a haplotype: the header alone)
        if (!cfg.haps()) return;
        const HapStats hs = write_haplotypes_tsv(base + ".haplotypes.tsv", ix, best, hap_wins, d.hap_table, cfg.hap);
        LOG_INFO(T, "Haplotypes: " + num(d.hap_summ.rows) + " placed records over " + num(d.hap_summ.n_regions) + " regions, " + num(hs.no_cover) + " without cover, " +
                        num(hs.distinct) + " distinct haplotypes, " + num(hs.lines) + " lines written, table of 2^" + num(d.hap_summ.table_log2) + " slots");
    }
    // --read-pileup: likewise; 48 bytes a position travel
    void read_pileup_count(bk_engine* e, SampleData& d) const {
        if (!cfg.read_pileup) return;
        static_assert(sizeof(ReadPileupCell) == sizeof(bk_read_pileup_cell), "ReadPileupCell is bk_read_pileup_cell");
        hip_check(bk_sample_read_pileup(e, cfg.read_pile.end_dist), "bk_sample_read_pileup");
        d.read_pileup.rows.resize((size_t)ix.genome_len(0));
        hip_check(bk_sample_download_read_pileup(e, &d.read_pileup.summ, reinterpret_cast<bk_read_pileup_cell*>(d.read_pileup.rows.data()), d.read_pileup.rows.size()),
                  "bk_sample_download_read_pileup");
    }
    void read_pileup_write(const std::string& base, int best, const SampleData& d) const {
        if (!cfg.read_pileup) return;
        const bk_read_pileup_summary& s = d.read_pileup.summ;
        write_read_pileup_tsv(base + ".read_pileup.tsv", ix, best, d.read_pileup.rows, cfg.read_pile);
        LOG_INFO(T, "Read pileup: " + num(s.rows) + " placed records, " + num(s.covered) + " of " + num(s.n_cells) + " positions covered, " + num(s.bases) +
                        " bases, near an end within " + num(s.end_dist));
    }

    void make_engine(int device, Engine& out, bool selected_only = true) const {
        std::vector<int32_t> n_seqs;
        std::vector<uint64_t> seq_lens;
        std::vector<const uint8_t*> seqs;
        for (const auto& f : ix.files) {
            n_seqs.push_back((int32_t)f.sequences.size());
            for (const auto& s : f.sequences) { seq_lens.push_back(s.len); seqs.push_back(s.seq.data()); }
        }
        bk_index_desc d{};
        d.k = ix.k; d.n_buckets = ix.ids.size(); d.bucket_ids = ix.ids.data(); d.bucket_off = ix.off.data();
        d.entries = reinterpret_cast<const bk_bucket_info*>(ix.entries.data()); d.n_entries = ix.entries.size();
        d.n_files = (int32_t)ix.files.size(); d.n_seqs = n_seqs.data(); d.seq_lens = seq_lens.data(); d.seqs = seqs.data();
        bk_params p;
        bk_params_default(&p);
        p.n_fixed = (int32_t)a.n_fixed; p.use_full_kmer = a.use_full_kmer ? 1 : 0; p.ci = (uint64_t)a.min_kmers;
        p.pileup_selected_only = selected_only ? 1 : 0;   // calls, pileup TSV and overview read the selected genome's rows only (call.rs:229-293)
        p.full_kmer_stats = 1;   // KMC's "unique counted k-mers" feeds num_unmapped_kmers and the <0.2 warning (call.rs:242-248)
        if (const char* tl = getenv("BRONKO_KMER_TABLE_LOG2")) p.kmer_table_log2 = (uint32_t)atoi(tl);
        p.device = device;
        hip_check(bk_engine_create(&d, &p, &out.e), "bk_engine_create");
    }

    // one engine per GPU of shard_devices and their communicators; false: this index cannot be sharded
    bool build_shards(const std::vector<int>& shard_devices, ShardGroup& shards, std::vector<Engine>& shard_engines) const {
        // one engine per GPU, every genome's rows (the two-pass selected-only finalize cannot be sharded: the selection needs the
        // statistics of all parts first); an index so large that its planes are kept sparse cannot be sharded at all
        shard_engines = std::vector<Engine>(shard_devices.size());
        std::vector<std::thread> th;
        for (size_t q = 0; q < shard_devices.size(); q++) th.emplace_back([&, q] { make_engine(shard_devices[q], shard_engines[q], ix.files.size() <= 1); });
        for (auto& t : th) t.join();
        if (!bk_can_shard(shard_engines[0].e)) {
            LOG_WARN(T, "The index keeps its counter planes sparse: a sample cannot be sharded over GPUs, whole samples go to the GPUs in turn");
            shard_engines.clear();
            return false;
        }
        shards.devices = shard_devices;
        shards.comms.resize(shard_devices.size());
        nccl_check(ncclCommInitAll(shards.comms.data(), (int)shard_devices.size(), shard_devices.data()), "ncclCommInitAll");
        for (auto& en : shard_engines) { shards.engs.push_back(en.e); shards.streams.push_back(static_cast<hipStream_t>(bk_engine_get_stream(en.e))); }
        LOG_INFO(T, "Every sample's reads go to " + std::to_string(shard_devices.size()) + " GPU(s); RCCL reduce-scatter of the k-mer counter planes");
        return true;
    }

    FirstEngines first_engines(const std::vector<int>& devices) const {
        FirstEngines first{std::vector<Engine>(devices.size()), std::vector<int>(devices.size(), -1)};
        std::vector<std::thread> th;   // table construction is host work: the devices' engines are created side by side
        for (size_t l = 0; l < devices.size(); l++) {
            bool seen = false;
            for (size_t q = 0; q < l; q++) seen = seen || devices[q] == devices[l];
            if (!seen) { first.dev[l] = devices[l]; th.emplace_back([this, &devices, &first, l] { make_engine(devices[l], first.eng[l]); }); }
        }
        for (auto& t : th) t.join();
        return first;
    }

    // the device of every lane: `devices` dealt per_device times over, no more lanes than samples
    std::vector<int> size_lanes(const std::vector<int>& devices, const FirstEngines& first) const {
        if (devices.empty()) return {};
        size_t per_device = std::min<size_t>(16, std::max<size_t>(1, (size_t)a.threads / 2 / devices.size()));
        for (size_t q = 0; q < first.eng.size(); q++) {
            if (!first.eng[q].e) continue;
            // what a lane's two engines keep on the device: two counter planes, the deferred lists and touch lists (as much
            // again), pileups, the k-mer statistics table (it starts at 0.8 GB) -- against six tenths of what the device has free
            const double per_engine = 4.0 * 8.0 * (double)bk_counter_len(first.eng[q].e) + 64.0 * (double)bk_total_cells(first.eng[q].e) + 1.0e9;
            uint64_t free_b = 0, total_b = 0;
            if (bk_device_memory(first.dev[q], &free_b, &total_b) != 0) free_b = 64ull << 30;
            per_device = std::min<size_t>(per_device, std::max<size_t>(1, (size_t)(0.6 * (double)free_b / (2.0 * per_engine))));
        }
        // with every file read ahead of its turn a lane only pushes, finalizes and writes: two per device are what pays (32 x 1 M reads
        // 2.9 -> 2.4 s, 64 samples against 100 strains 13.9 -> 11.6 s; a lane's engines and their forks are not free)
        if (ahead && ahead->covers_all()) per_device = std::min<size_t>(per_device, 2);
        if (const char* nl = getenv("BRONKO_LANES")) per_device = std::max<size_t>(1, (size_t)atoi(nl));
        std::vector<int> lanes_on;
        for (size_t r = 0; r < per_device; r++)                       // device-major rounds: every device gets a lane before any gets two
            for (int d : devices) lanes_on.push_back(d);
        if (lanes_on.size() > std::max<size_t>(samples.size(), 1)) lanes_on.resize(std::max<size_t>(samples.size(), 1));
        return lanes_on;
    }

    // a lane per entry of `devices`: a device's first lane takes its first engine, the others fork it
    std::vector<Lane> build_lanes(const std::vector<int>& devices, FirstEngines& first) const {
        std::vector<Lane> lanes(devices.size());
        for (size_t l = 0; l < lanes.size(); l++) {
            lanes[l].device = devices[l];
            for (size_t q = 0; q < l && lanes[l].parent < 0; q++)
                if (lanes[q].device == devices[l]) lanes[l].parent = (int)(lanes[q].parent < 0 ? q : (size_t)lanes[q].parent);
        }
        if (lanes.size() > 1) {
            std::string names;
            for (int d : devices) names += (names.empty() ? "" : ",") + std::to_string(d);
            LOG_INFO(T, "Samples go to " + std::to_string(lanes.size()) + " GPU lanes in turn (devices " + names + ")");
        }
        for (auto& ln : lanes)
            for (size_t q = 0; q < first.eng.size() && ln.parent < 0; q++)
                if (first.eng[q].e && !ln.eng.e && first.dev[q] == ln.device) std::swap(ln.eng.e, first.eng[q].e);
        std::vector<std::thread> th;   // (a fork allocates and zeroes a sample's planes: gigabytes with a large index)
        for (auto& ln : lanes)
            if (ln.parent >= 0) th.emplace_back([&lanes, &ln] { hip_check(bk_engine_fork(lanes[(size_t)ln.parent].eng.e, &ln.eng.e), "bk_engine_fork"); });
        for (auto& t : th) t.join();
        return lanes;
    }

    // ---- one sample ----------------------------------------------------------------------------------------------------------------
    // one sample = one -r file (call.rs:213-293) or one R1/R2 pair (call.rs:298-386); outputs are named after R1.
    // A sample has two halves: ingest (parse the FASTQ files, push the reads: host-bound, the scan runs behind it) and
    // complete (finalize on the GPU, download, pick the genome, call variants, write the files).  With several samples the two
    // halves of consecutive samples overlap: sample i+1 is ingested into a second engine on the same device tables
    // (bk_engine_fork) while a worker thread completes sample i.  Results are reported in input order.
    void ingest(const std::vector<bk_engine*>& engs, size_t sample_id, unsigned inflate) {
        const auto& mates = samples[sample_id];
        LOG_INFO(T, mates.size() == 1 ? "Processing " + mates[0] : "Processing paired reads " + mates[0] + ", " + mates[1]);
        for (bk_engine* e : engs) hip_check(bk_sample_begin(e), "bk_sample_begin");
        uint64_t total_reads = 0;
        try { total_reads = push_fastqs(engs, mates, cfg, inflate, ahead.get(), sample_id); }
        catch (const std::exception& ex) { die(T, ex.what()); }
        LOG_INFO(T, std::to_string(total_reads) + " reads counted from " + mates[0]);
    }

    // --adapter, --primers: every engine that takes reads trims them (bk_adapters_set, bk_primers_set are per engine), and every engine
    // that completes a sample holds the region table (bk_regions_set, per engine as well); under
    // --verbose, what was trimmed per reads file, summed over the sample's engines
    template <class Set>
    static void set_seqs(const std::vector<std::string>& list, Set&& set) {   // set(seqs, lens, n): the bk_*_set call
        std::vector<const uint8_t*> seqs;
        std::vector<uint32_t> lens;
        for (const auto& p : list) { seqs.push_back(reinterpret_cast<const uint8_t*>(p.data())); lens.push_back((uint32_t)p.size()); }
        if (!list.empty()) set(seqs.data(), lens.data(), (uint32_t)seqs.size());
    }
    void set_trims(bk_engine* e) const {
        if (!e) return;
        set_seqs(cfg.adapters, [&](const uint8_t* const* q, const uint32_t* l, uint32_t n) { hip_check(bk_adapters_set(e, q, l, n, cfg.adapter_min_overlap, cfg.adapter_error_rate), "bk_adapters_set"); });
        set_seqs(cfg.primers, [&](const uint8_t* const* q, const uint32_t* l, uint32_t n) { hip_check(bk_primers_set(e, q, l, n, cfg.primer_mismatches), "bk_primers_set"); });
        regions_set(e);
        each_anchor_pass([&](auto p) {
            if (!p.on(cfg)) return;
            const auto c = p.config(cfg);
            hip_check(p.enable(e, &c), p.enable_name);
        });
        if (cfg.row_store()) {   // (--codons, --haplotypes and --read-pileup read --linkage's row store; alone each brings its own M, together they are equal)
            const bk_link_config lc{cfg.row_store_mismatches(), kLinkInitialRows};
            hip_check(bk_link_enable(e, &lc), "bk_link_enable");
        }
    }
    // text(sum): the line's start; stats(e, mate, out): the bk_*_stats call, n counters a mate file
    template <class Stats, class Text>
    static void log_sums(const std::vector<bk_engine*>& engs, const std::vector<std::string>& mates, int n, Stats&& stats, const char* fn, Text&& text) {
        for (size_t m = 0; m < mates.size(); m++) {
            uint64_t sum[3] = {0, 0, 0};
            for (bk_engine* e : engs) {
                uint64_t o[3] = {0, 0, 0};
                hip_check(stats(e, (int)m, o), fn);
                for (int i = 0; i < n; i++) sum[i] += o[i];
            }
            LOG_TRACE(T, text(sum) + " in " + mates[m]);
        }
    }
    void log_trim_stats(const std::vector<bk_engine*>& engs, const std::vector<std::string>& mates) const {
        if (!log_enabled(4)) return;
        if (!cfg.adapters.empty())
            log_sums(engs, mates, 2, bk_adapter_stats, "bk_adapter_stats", [](const uint64_t* s) {
                return "adapters: " + std::to_string(s[0]) + " reads cut, " + std::to_string(s[1]) + " bases removed"; });
        if (!cfg.primers.empty())
            log_sums(engs, mates, 3, bk_primer_stats, "bk_primer_stats", [](const uint64_t* s) {
                return "primers: " + std::to_string(s[0]) + " reads trimmed at the 5' end, " + std::to_string(s[1]) + " at the 3' end, " + std::to_string(s[2]) + " bases masked"; });
    }

    // finalize, then reference selection + baseline noise + variant calls, all on the device and asynchronous
    // (bk_sample_call); the pileup arrays only travel when --pileup wants them written
    void launch_calls(bk_engine* e, const std::vector<std::string>& mates, bool finalized) const {
        const int n_mates = (int)mates.size();
        if (!finalized) hip_check(bk_sample_finalize(e, n_mates), "bk_sample_finalize");   // (a sharded sample: sharded_finalize has done it)
        if (!finalized) log_trim_stats(std::vector<bk_engine*>{e}, mates);
        each_anchor_pass([&](auto p) {   // (they need the finalize only: the events that pass the thresholds, a few rows travel)
            if (!p.on(cfg)) return;
            const auto q = p.params(cfg);
            hip_check(p.report(e, &q), p.report_name);
        });
        hip_check(bk_sample_call(e, n_mates, &cfg.call), "bk_sample_call");
        consensus_launch(e);        // behind the calls, in this order
        minor_launch(e);
        consensus_indels_launch(e);
        regions_launch(e);
    }
    void download_pileup(bk_engine* e, int n_mates, SampleData& d) const {
        const size_t n_files = ix.files.size(), cells4 = ix.total_cells() * 4;
        d.stats.resize((size_t)n_mates * n_files * 3); d.kstats.resize((size_t)n_mates * 4); d.present.resize((size_t)n_mates * n_files);
        if (a.pileup) { d.p.fwd_depth.resize(cells4); d.p.rev_depth.resize(cells4); }
        hip_check(bk_sample_download(e, n_mates, a.pileup ? d.p.fwd_depth.data() : nullptr, a.pileup ? d.p.rev_depth.data() : nullptr, nullptr, nullptr,
                                     d.stats.data(), d.present.data(), d.kstats.data()), "bk_sample_download");
    }
    // call.rs:1202-1211, kept by --keep-kmer-info (:404-420): <output>/<stem>_counts.txt per reads file
    void write_kmer_count_files(bk_engine* e, const std::vector<std::string>& mates) const {
        for (size_t m = 0; m < mates.size(); m++) {
            uint64_t n_kept = 0, n_distinct = 0;
            hip_check(bk_kmer_dump_size(e, (int)m, &n_kept, &n_distinct), "bk_kmer_dump_size");
            if (n_kept == ~0ull) die(T, "k-mer count table overflowed: --keep-kmer-info cannot write the counts of " + mates[m]);
            std::vector<uint64_t> km(std::max<uint64_t>(n_kept, 1)), ct(std::max<uint64_t>(n_kept, 1));
            hip_check(bk_kmer_dump_download(e, (int)m, km.data(), ct.data(), n_kept), "bk_kmer_dump_download");
            const std::string path = a.output + "/" + clean_sample_id(mates[m]) + "_counts.txt";
            LOG_DEBUG(T, "Writing " + std::to_string(n_kept) + " k-mer counts (" + std::to_string(n_distinct) + " distinct k-mers) to " + path);
            try { write_kmer_counts(path, (int)a.kmer, km.data(), ct.data(), n_kept, dump_threads); }
            catch (const std::exception& ex) { die(T, ex.what()); }
        }
    }
    void download_calls(bk_engine* e, SampleData& d) const {
        uint64_t longest = 1;   // at most three alternative bases per position of the selected genome
        for (size_t f = 0; f < ix.files.size(); f++) longest = std::max<uint64_t>(longest, ix.genome_len(f));
        d.recs.resize((size_t)(3 * longest));
        hip_check(bk_sample_download_calls(e, &d.summ, d.recs.data(), d.recs.size()), "bk_sample_download_calls");
        consensus_download(e, longest, d);
        minor_download(e, longest, d);
        consensus_indels_download(e, d);
        regions_download(e, d);
        each_anchor_pass([&](auto p) {
            using P = decltype(p);
            PassRows<P>& t = std::get<PassRows<P>>(d.events);
            if (p.on(cfg)) download_rows(e, p.download, p.download_name, t, t.summ.reported);
        });
        linkage_count(e, d);        // the readers of the row store, behind the calls: each launches and downloads here
        codons_count(e, d);
        haps_count(e, d);
        read_pileup_count(e, d);
    }
    // the mates' statistics summed into d.p; returns KMC's "No. of unique counted k-mers", summed over mate files (call.rs:336)
    uint64_t merge_mates(const std::vector<std::string>& mates, SampleData& d) const {
        const size_t n_files = ix.files.size();
        d.p.stats.assign(n_files * 3, 0);
        d.p.present.assign(n_files, 0);
        uint64_t kept = 0;
        bool kept_exact = true;
        for (size_t m = 0; m < mates.size(); m++) {                  // pick_best_genome_paired sums R1 + R2 (call.rs:457-474)
            for (size_t i = 0; i < n_files * 3; i++) d.p.stats[i] += d.stats[m * n_files * 3 + i];
            for (size_t f = 0; f < n_files; f++) d.p.present[f] |= d.present[m * n_files + f];
            if (d.kstats[m * 4 + 3] == ~0ull) kept_exact = false; else kept += d.kstats[m * 4 + 3];
        }
        // (the engine grows the table with the sample; only a sample with more than 2^30 distinct erroneous k-mers gets here)
        if (!kept_exact) die(T, "k-mer statistics table overflowed: num_unmapped_kmers cannot be reported for " + mates[0]);
        return kept;
    }
    CallSummary to_call_summary(const SampleData& d) const {
        const bk_call_summary& summ = d.summ;
        CallSummary cs;
        cs.n_major = summ.n_major; cs.n_minor = summ.n_minor;
        cs.breadth = (double)summ.covered / (double)summ.positions;               // call.rs:1144
        cs.depth = (double)summ.coverage / (double)summ.covered;                  // call.rs:1145 (NaN when nothing is covered)
        for (uint64_t i = 0; i < std::min<uint64_t>(summ.n_records, d.recs.size()); i++) {
            const bk_call_record& r = d.recs[i];
            // SOR as printed: the reference's expression on the host's libm (the device's ln made the decision; the two agree
            // to the last ulps, the printed three decimals are the host's)
            const double sor = strand_odds(r.fwd_ref, r.rev_ref, r.fwd_alt, r.rev_alt, cfg.cp);
            cs.records.push_back(VcfRecord{r.seq_id, r.pos, r.ref_base, r.alt_base, r.fwd_ref, r.rev_ref, r.fwd_alt, r.rev_alt, r.depth, r.af, sor});
        }
        return cs;
    }
    void write_outputs(const std::vector<std::string>& mates, int best, const SampleData& d, const CallSummary& cs) const {
        const std::string stem = clean_sample_id(mates[0]), base = a.output + "/" + stem;
        try {
            if (a.pileup) { LOG_INFO(T, "Writing output to pileup"); write_pileup_tsv(base + ".tsv", ix, best, d.p); }
            LOG_INFO(T, "Writing output to VCF");
            write_vcf(base + ".vcf", mates[0], ix, best, cs.records);
            consensus_write(base, stem, best, d);
            minor_log(d);
            consensus_indels_write(base, stem, best, d);
            regions_write(base, best, d);
            each_anchor_pass([&](auto p) {   // (a sample without events: the headers alone)
                using P = decltype(p);
                if (!p.on(cfg)) return;
                const PassRows<P>& t = std::get<PassRows<P>>(d.events);
                LOG_INFO(T, p.sentence(t.summ));
                p.write(base + p.suffix, mates[0], ix, best, t, cfg);
            });
            linkage_write(base, best, d);
            codons_write(base, best, d);
            haps_write(base, best, d);
            read_pileup_write(base, best, d);
        } catch (const std::exception& ex) { die(T, ex.what()); }
    }

    void complete(bk_engine* e, const std::vector<std::string>& mates, size_t sample_id, bool finalized = false) {
        SampleData d;
        LOG_INFO(T, "Mapping kmers to all genomes (" + mates[0] + ")");
        launch_calls(e, mates, finalized);
        download_pileup(e, (int)mates.size(), d);
        if (a.keep_kmer_info) write_kmer_count_files(e, mates);
        download_calls(e, d);
        const uint64_t kept = merge_mates(mates, d);
        LOG_INFO(T, "Selecting the most representative genome");
        const int best = d.summ.file_id;
        if (best < 0) die(T, "Unable to pick a best genome");
        const std::string& gname = ix.files[best].name;
        LOG_INFO(T, "Selected a representative genome: " + gname);
        const uint64_t n_perfect = d.p.stats[(size_t)best * 3], n_variant = d.p.stats[(size_t)best * 3 + 1];
        const uint64_t n_unmapped = kept >= n_perfect + n_variant ? kept - n_perfect - n_variant : 0;   // call.rs:242,336
        if (kept > 0 && (double)(n_variant + n_perfect) / (double)kept < 0.2)                            // call.rs:246-248
            LOG_WARN(T, "Percent of kmers found is very low for this reference, suggesting lack of a representative reference, a bad sequencing run, contamination in sample, or some other issue");
        LOG_INFO(T, "Mapped " + std::to_string(n_perfect) + "/" + std::to_string(kept) + " kmers perfectly (" +
                        std::to_string(d.p.stats[(size_t)best * 3 + 2]) + " unique among refs), " + std::to_string(n_variant) + "/" +
                        std::to_string(kept) + " had a variant");
        LOG_INFO(T, "Calling variants for " + gname);
        const CallSummary cs = to_call_summary(d);
        LOG_INFO(T, "Called " + std::to_string(cs.n_major) + " major variants, " + std::to_string(cs.n_minor) + " minor above maf = " + std::to_string(a.min_af));
        write_outputs(mates, best, d, cs);
        overview[sample_id] = OverviewRow{mates[0], gname, cs.n_major, cs.n_minor, cs.breadth, cs.depth, n_perfect, n_variant, n_unmapped};
        if (a.alignment) all_calls[sample_id] = SampleCalls{mates[0], gname, cs.breadth, cs.records};
        if (a.distances) {   // (the letters as they were written: with '-' at the deletions --consensus-indels applied)
            cohort_letters[sample_id].assign(d.consensus.rows.begin(), d.consensus.rows.begin() + (ptrdiff_t)std::min<uint64_t>(d.consensus.summ.positions, d.consensus.rows.size()));
            cohort_genome[sample_id] = best;
        }
        if (a.contamination) cohort_masks[sample_id].assign(d.minor.rows.begin(), d.minor.rows.begin() + (ptrdiff_t)std::min<uint64_t>(d.minor.summ.positions, d.minor.rows.size()));
    }

    // ---- --mst: the minimum spanning forest of the cohort the engine holds, found on the device; OUT/<genome>.mst.tsv ----
    void write_forest(bk_engine* e, const std::string& gname, const std::vector<std::string>& names, uint64_t positions) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint64_t n = names.size();
        const uint32_t min_compared = cohort_min_compared(a.mst_min_breadth, positions);
        std::vector<bk_mst_edge> edges((size_t)(n - 1));
        std::vector<bk_mst_nearest> nearest((size_t)n);
        uint64_t n_edges = 0;
        uint32_t rounds = 0;
        hip_check(bk_cohort_mst(e, min_compared, edges.data(), edges.size(), &n_edges, nearest.data(), &rounds), "bk_cohort_mst");
        CohortForest f;
        try {
            std::vector<CohortMstEdge> ev;
            std::vector<CohortMstNearest> nr;
            for (uint64_t k = 0; k < n_edges; k++) ev.push_back(CohortMstEdge{edges[k].lo, edges[k].hi, edges[k].diff, edges[k].compared});
            for (const auto& x : nearest) nr.push_back(CohortMstNearest{x.sample, x.diff, x.compared});
            f = root_forest(n, ev);
            write_cohort_mst_tsv(a.output + "/" + gname + ".mst.tsv", names, f, nr, a.mst_min_breadth, min_compared);
        } catch (const std::exception& ex) { die(T, ex.what()); }
        char secs[32];
        snprintf(secs, sizeof secs, "%.3f", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        LOG_INFO(T, "Forest for " + gname + ": " + std::to_string(n) + " samples, " + std::to_string(n_edges) + " edges, " + std::to_string(f.n_components) +
                        " components, the largest of " + std::to_string(f.largest) + " samples, longest edge " + std::to_string(f.longest) + ", " +
                        std::to_string(rounds) + " rounds (" + secs + " s)");
    }

    // ---- --distances: the samples' consensus letters compared pair by pair, per selected genome, on one engine that is still alive ----
    void write_distances(bk_engine* e) {
        constexpr uint64_t kBlockBytes = 256ull << 20;   // a block's host buffers together: two, three under --contamination
        for (size_t i = 0; i < samples.size(); i++)
            if (cohort_genome[i] < 0) LOG_INFO(T, "Distances: " + clean_sample_id(samples[i][0]) + " selected no genome and is left out");
        for (size_t g = 0; g < ix.files.size(); g++) {
            std::vector<size_t> group;
            for (size_t i = 0; i < samples.size(); i++)
                if (cohort_genome[i] == (int)g) group.push_back(i);
            if (group.empty()) continue;
            const std::string& gname = ix.files[g].name;
            if (group.size() < 2) { LOG_INFO(T, "Skipping distances for " + gname + " (1 sample selected it, at least 2 are compared)"); continue; }
            const auto t0 = std::chrono::steady_clock::now();
            const uint64_t n = group.size(), positions = ix.genome_len(g);
            std::vector<std::string> names;
            std::vector<uint8_t> letters((size_t)(n * positions));
            for (size_t r = 0; r < n; r++) {
                names.push_back(clean_sample_id(samples[group[r]][0]));
                std::vector<uint8_t>& l = cohort_letters[group[r]];
                if (l.size() != positions) die(T, "Distances: the consensus of " + names.back() + " is not as long as " + gname);
                std::copy(l.begin(), l.end(), letters.begin() + (ptrdiff_t)(r * positions));
                std::vector<uint8_t>().swap(l);   // (a sample's letters are held once)
            }
            hip_check(bk_cohort_set(e, letters.data(), n, positions), "bk_cohort_set");
            if (a.contamination) {   // (the masks take the letters' place in the same buffer)
                for (size_t r = 0; r < n; r++) {
                    std::vector<uint8_t>& m = cohort_masks[group[r]];
                    if (m.size() != positions) die(T, "Contamination: the minor alleles of " + names[r] + " are not as long as " + gname);
                    std::copy(m.begin(), m.end(), letters.begin() + (ptrdiff_t)(r * positions));
                    std::vector<uint8_t>().swap(m);
                }
                hip_check(bk_cohort_set_minor(e, letters.data(), n, positions), "bk_cohort_set_minor");
            }
            std::vector<uint8_t>().swap(letters);
            const uint64_t block_rows = std::max<uint64_t>(1, std::min<uint64_t>(n, kBlockBytes / ((a.contamination ? 12 : 8) * n)));
            std::vector<uint32_t> diff((size_t)(block_rows * n)), compared((size_t)(block_rows * n)), explained(a.contamination ? (size_t)(block_rows * n) : 0);
            std::vector<uint32_t> minor_sites(a.contamination ? (size_t)n : 0);
            uint64_t max_diff = 0, empty_pairs = 0;
            CohortClusters cl;
            Contamination mix;
            try {
                std::unique_ptr<CohortMatrixWriter> we;
                if (a.contamination) we.reset(new CohortMatrixWriter(a.output + "/" + gname + ".explained.tsv", names));
                std::unique_ptr<ContaminationScanner> scanner;
                if (a.contamination) scanner.reset(new ContaminationScanner(n, cfg.contamination.min_sites, cfg.contamination.min_share));
                CohortMatrixWriter wd(a.output + "/" + gname + ".distances.tsv", names), wc(a.output + "/" + gname + ".compared.tsv", names);
                CohortClusterer clusterer(n, positions, (uint64_t)a.clusters, a.cluster_min_breadth);
                for (uint64_t row0 = 0; row0 < n; row0 += block_rows) {
                    const uint64_t rows = std::min(block_rows, n - row0);
                    hip_check(bk_cohort_distances(e, row0, rows, diff.data(), compared.data()), "bk_cohort_distances");
                    wd.add_rows(row0, rows, diff.data());
                    wc.add_rows(row0, rows, compared.data());
                    if (a.has_clusters()) clusterer.add_rows(row0, rows, diff.data(), compared.data());
                    if (a.contamination) {
                        hip_check(bk_cohort_explained(e, row0, rows, explained.data(), minor_sites.data() + row0), "bk_cohort_explained");
                        we->add_rows(row0, rows, explained.data());
                        scanner->add_rows(row0, rows, diff.data(), compared.data(), explained.data());
                    }
                    for (uint64_t r = 0; r < rows; r++)
                        for (uint64_t j = row0 + r + 1; j < n; j++) {   // (each pair once)
                            max_diff = std::max<uint64_t>(max_diff, diff[r * n + j]);
                            empty_pairs += compared[r * n + j] == 0;
                        }
                }
                wd.close(); wc.close();
                if (a.has_clusters()) {
                    cl = clusterer.finish();
                    write_cohort_clusters_tsv(a.output + "/" + gname + ".clusters.tsv", names, cl, (uint64_t)a.clusters, a.cluster_min_breadth);
                }
                if (a.contamination) {
                    we->close();
                    mix = scanner->finish();
                    write_contamination_tsv(a.output + "/" + gname + ".contamination.tsv", names, mix, minor_sites, cfg.contamination);
                    write_mixture_tsv(a.output + "/" + gname + ".mixture.tsv", names, mix, minor_sites, cfg.contamination);
                }
            } catch (const std::exception& ex) { die(T, ex.what()); }
            char secs[32];
            snprintf(secs, sizeof secs, "%.3f", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            LOG_INFO(T, "Distances for " + gname + ": " + std::to_string(n) + " samples, largest distance " + std::to_string(max_diff) + ", " +
                            std::to_string(empty_pairs) + " pairs with nothing compared" +
                            (a.has_clusters() ? ", " + std::to_string(cl.n_clusters) + " clusters, the largest of " + std::to_string(cl.largest) + " samples" : std::string()) +
                            " (" + secs + " s)");
            if (a.contamination)
                LOG_INFO(T, "Contamination for " + gname + ": " + std::to_string(n) + " samples, " + std::to_string(mix.flagged.size()) + " flagged pairs, " +
                                std::to_string(mix.recipients) + " samples flagged at least once, largest explained " + std::to_string(mix.largest));
            if (a.mst) write_forest(e, gname, names, positions);   // (the cohort is still set)
        }
        hip_check(bk_cohort_clear(e), "bk_cohort_clear");
    }

    // ---- the samples ---------------------------------------------------------------------------------------------------------------
    void run_sharded_samples(ShardGroup& shards, unsigned inflate) {
        for (bk_engine* e : shards.engs) set_trims(e);
        for (size_t i = 0; i < samples.size(); i++) {
            const auto& mates = samples[i];
            ingest(shards.engs, i, inflate);
            sharded_finalize(shards, (int)mates.size(), ix.total_cells() * 4);
            log_trim_stats(shards.engs, mates);
            complete(shards.engs[0], mates, i, true);
        }
        for (auto c : shards.comms) nccl_check(ncclCommDestroy(c), "ncclCommDestroy");
    }
    void run_lane(Lane& ln, unsigned inflate) {
        if (ln.mine.size() > 1) hip_check(bk_engine_fork(ln.eng.e, &ln.fork.e), "bk_engine_fork");
        for (bk_engine* e : {ln.eng.e, ln.fork.e}) set_trims(e);
        if (a.keep_kmer_info)   // (the table grows with the sample)
            for (bk_engine* e : {ln.eng.e, ln.fork.e})
                if (e) hip_check(bk_kmer_dump_enable(e, kDumpTableLog2), "bk_kmer_dump_enable");
        std::thread worker;     // completes the lane's previous sample
        for (size_t n = 0; n < ln.mine.size(); n++) {
            const size_t i = ln.mine[n];
            bk_engine* e = (n & 1) ? ln.fork.e : ln.eng.e;   // (its previous sample, n - 2, was completed before sample n - 1's worker started)
            ingest(std::vector<bk_engine*>{e}, i, inflate);
            if (worker.joinable()) worker.join();
            worker = std::thread([this, e, i] { complete(e, samples[i], i); });
        }
        if (worker.joinable()) worker.join();
        if (ln.fork.e) { bk_engine_destroy(ln.fork.e); ln.fork.e = nullptr; }   // (the fork goes before its parent)
    }
    void run_lanes(std::vector<Lane>& lanes, unsigned inflate) {
        for (size_t i = 0; i < samples.size() && !lanes.empty(); i++) lanes[i % lanes.size()].mine.push_back(i);
        if (lanes.size() == 1) run_lane(lanes[0], inflate);
        else if (!lanes.empty()) {
            std::vector<std::thread> th;
            for (auto& ln : lanes) th.emplace_back([this, &ln, inflate] { run_lane(ln, inflate); });
            for (auto& t : th) t.join();
        }
    }

    void write_run_outputs() const {
        LOG_INFO(T, "Printing overview");
        try { write_overview_tsv(a.output + "/bronko_overview.tsv", overview); }
        catch (const std::exception& e) { die(T, e.what()); }
        LOG_INFO(T, "All samples processed successfully");
        if (a.alignment) {                                                                  // call.rs:394-397
            LOG_INFO(T, "Building alignment(s)");
            try { write_alignments(a.output, ix, all_calls, [](const std::string& m) { LOG_INFO("bronko::call", m); }); }
            catch (const std::exception& e) { die(T, e.what()); }
        }
    }
};

}  // namespace

int call_samples(const Args& a, const CallConfig& cfg) {
    LOG_TRACE(T, "k=" + std::to_string(a.kmer) + ", threads=" + std::to_string(a.threads));
    ensure_output_dir(a.output);
    CallRun run(a, cfg);
    run.open_index();

    std::vector<int> devices = devices_from_env();
    const size_t n_samples = std::max<size_t>(run.samples.size(), 1);
    const std::vector<int> shard_devices = plan_shards(a, cfg, devices, run.samples.size());
    if (devices.size() > n_samples) devices.resize(n_samples);   // no more lanes than samples
    ShardGroup shards;
    std::vector<Engine> shard_engines;
    if (!shard_devices.empty() && run.build_shards(shard_devices, shards, shard_engines)) devices.clear();   // (no whole-sample lanes)
    FirstEngines first = run.first_engines(devices);
    std::vector<Lane> lanes = run.build_lanes(run.size_lanes(devices, first), first);

    // KMC reads a sample's files with all of -t (call.rs:1166-1181); here -t is shared by the files that are open at once: the
    // lanes' samples (one being read per lane) times their mate files (inflate_threads, cli.hpp)
    const unsigned inflate = inflate_threads(a.threads, std::max<size_t>(1, lanes.size()) * (a.first_pairs.empty() ? 1 : 2));
    if (inflate > 1) LOG_INFO(T, "gzip input is inflated on " + std::to_string(inflate) + " threads per file");
    if (run.ahead) run.ahead->set_concurrency((unsigned)std::max<long>(2, a.threads / 2));   // (the engines are made: the cores are the readers')
    run.dump_threads = (int)std::max<size_t>(1, std::min<size_t>(16, (size_t)a.threads / std::max<size_t>(1, lanes.size())));

    if (!shards.engs.empty()) {
        run.run_sharded_samples(shards, inflate);
        if (a.distances) run.write_distances(shards.engs[0]);   // (the cohort step takes one engine that is still alive: the first shard's ...)
        shard_engines.clear();
    }
    run.run_lanes(lanes, inflate);
    if (a.distances && !lanes.empty()) run.write_distances(lanes[0].eng.e);   // (... or the first lane's)
    release_lanes(lanes);
    run.write_run_outputs();
    LOG_INFO(T, "");
    LOG_INFO(T, "bronko complete!");
    return 0;
}

}  // namespace bronko
