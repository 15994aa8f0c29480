/*
 * bronko_hip.h -- C ABI of the MI355X (gfx950) k-mer -> pileup engine.
 *
 * This is the seam a host program binds (Rust `extern "C"` block, C++, ctypes ...).  It replaces, inside
 * bronko's `call()` per-sample loop, the stages
 *
 *     get_kmers        /root/reference/src/call.rs:630-646   (external KMC3: count_kmers_kmc :1152-1233,
 *                                                             load_kmers :1241-1255)
 *     initialize_output_maps                  call.rs:1437-1480
 *     map_kmers                               call.rs:1257-1434
 *
 * i.e. everything between "a FASTQ record was parsed" and "four pileup arrays + per-genome
 * (perfect, variant, unique) statistics exist" (call sites: call.rs:217-226 single-end, :301-317 paired).
 * The reference has no FFI of its own for this path; INTEGRATION.md shows the Rust binding a maintainer
 * would add.  Plain pointers and sizes only; every function returns 0 on success and a negative bk_status on
 * failure (message via bk_last_error(), thread-local).  The library never calls exit(); the host maps a
 * non-zero status to the reference's `error!(..); std::process::exit(1)` convention.  An engine is
 * thread-compatible (one engine per host thread / per GPU); there is no global state.
 *
 * There is NO CPU fallback: if no gfx950 device is visible every entry point that needs one fails with
 * BK_ERR_NO_DEVICE.
 */
#ifndef BRONKO_HIP_H
#define BRONKO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BK_ABI_VERSION 8

typedef enum {
    BK_OK = 0,
    BK_ERR_INVALID = -1,   /* bad argument / inconsistent index            */
    BK_ERR_NO_DEVICE = -2, /* no HIP device / not gfx950                   */
    BK_ERR_HIP = -3,       /* a HIP runtime call failed                    */
    BK_ERR_UNSUPPORTED = -4,
    BK_ERR_STATE = -5,     /* call order violated (e.g. push before begin) */
    BK_ERR_RANGE = -6,     /* a counter did not fit the width its plane was exchanged at (bk_shard_transport) */
    BK_ERR_INTERNAL = -7   /* an invariant of the library did not hold (bk_cohort_mst past its round bound); additive, still v8 */
} bk_status;

/* build.rs:52-60  `#[repr(C)] struct BucketInfo` -- same field order, same layout (12 bytes) */
typedef struct {
    uint16_t file_id;   /* index of the genome file in ViralMetadata.files             */
    uint8_t  seq_id;    /* index of the sequence inside that file                      */
    uint32_t location;  /* 0-based start of the reference k-mer in the forward sequence */
    uint8_t  idx;       /* wildcard position inside the canonical k-mer                */
    uint8_t  canonical; /* 1 = the reference k-mer was reverse-complemented            */
} bk_bucket_info;

/* A decoded BronkoIndex (build.rs:23-50), flattened.  All pointers are host memory, borrowed for the
 * duration of bk_engine_create() only.
 *   global_index: FxHashMap<u64, Vec<BucketInfo>>  ->  bucket_ids[n_buckets] (any order, unique),
 *                 bucket_off[n_buckets + 1] into entries[n_entries]
 *   metadata    : files -> n_seqs[n_files]; sequences of all files concatenated in (file, seq) order:
 *                 seq_lens[total], seqs[total] (raw FASTA bytes as stored in SeqMeta.seq)               */
typedef struct {
    int32_t  k;
    uint64_t n_buckets;
    const uint64_t* bucket_ids;
    const uint64_t* bucket_off;
    const bk_bucket_info* entries;
    uint64_t n_entries;
    int32_t  n_files;
    const int32_t*  n_seqs;
    const uint64_t* seq_lens;
    const uint8_t* const* seqs;
} bk_index_desc;

/* Parameters that reach the hot path from CallArgs (cli.rs:61-166) and the KMC command line (call.rs:1166-1177) */
typedef struct {
    int32_t  n_fixed;        /* --n-fixed        (consts.rs:17, default 2)                                  */
    int32_t  use_full_kmer;  /* --use-full-kmer  (consts.rs:18, default 0)                                  */
    uint64_t ci;             /* --min-kmers -> kmc -ci (consts.rs:5, default 3): keep count >= ci           */
    uint64_t cs;             /* kmc -cs1000000 (call.rs:1173): reported count saturates at cs               */
    uint64_t cx;             /* kmc -cx default 1e9: drop k-mers whose true count exceeds cx                */
    int32_t  device;         /* HIP device ordinal                                                          */
    int32_t  full_kmer_stats;/* 1: also count every k-mer that does NOT touch the index in a device hash table, so
                                that KMC's "No. of unique k-mers" / "No. of unique counted k-mers" (call.rs:1190-1199)
                                are exact; 0 (default): only index-touching k-mers are counted (pileups identical) */
    uint32_t kmer_table_log2;/* initial capacity of that table = 2^kmer_table_log2 slots (default 26); it is rehashed into a
                                larger one whenever a batch might take its load above one half (up to 2^31 slots)          */
    uint32_t pileup_selected_only;/* 1: with several genome files, map_kmers' votes are cast for the SELECTED genome only (two passes:
                                per-genome statistics of all genomes, pick_best_genome on the device, then the votes): the
                                statistics and the selected genome's pileup rows are what the reference computes, the rows of
                                the other genomes stay zero -- nothing downstream of call.rs:229-235 reads them.  0 (default):
                                every genome's rows, as call.rs:1305-1384 fills them */
} bk_params;

typedef struct bk_engine bk_engine;

int         bk_abi_version(void);
/* Number of visible HIP devices (0 when there is none or the runtime cannot be initialised).  A host with several samples
 * creates one engine per device and deals whole samples to them (call.rs:212 / :297: samples are independent). */
int         bk_device_count(void);
/* Free and total memory of a device in bytes (v6): a host that runs several engines per device (bk_engine_fork: every fork holds
 * a sample's counter planes and outputs) sizes their number by it. */
int         bk_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
const char* bk_last_error(void);
void        bk_params_default(bk_params* p);

/* Uploads the index as a device-resident bucket table (see DESIGN.md "HBM layout") and allocates the
 * counter planes (one per mate file) and the four pileup arrays. */
int  bk_engine_create(const bk_index_desc* index, const bk_params* params, bk_engine** out);
void bk_engine_destroy(bk_engine* e);

/* A second engine on the same index: it reads the parent's device-resident tables (immutable after
 * bk_engine_create) and owns everything a sample writes -- counter planes, scan scratch, pileup / statistics
 * outputs, stream.  Samples are independent (call.rs:212 / :390 handle them one after the other), so a host
 * with many samples alternates them over two engines: sample i+1's scan overlaps sample i's finalize on the
 * device.  Same parameters as the parent.  Destroy the forks before the parent. */
int  bk_engine_fork(const bk_engine* parent, bk_engine** out);
/* The same with parameters of its own (v7): ci / cs / cx, pileup_selected_only and kmer_table_log2 belong to a sample's state and
 * may differ from the parent's; n_fixed, use_full_kmer, full_kmer_stats and device shape the shared tables and must not
 * (BK_ERR_INVALID).  E.g. one index, `--min-kmers 3` and `--min-kmers 5` samples side by side. */
int  bk_engine_fork_params(const bk_engine* parent, const bk_params* params, bk_engine** out);

/* Launch all work of this engine on an existing HIP stream (hipStream_t passed as void*); NULL restores the
 * engine's own stream.  Lets a host that already owns a stream (e.g. PyTorch's current stream) order and
 * time the engine's kernels. */
int bk_engine_set_stream(bk_engine* e, void* hip_stream);
/* The stream the engine launches on (hipStream_t as void*): its own, created with the engine, unless
 * bk_engine_set_stream replaced it.  A host orders its own work on the engine's buffers (e.g. RCCL collectives on
 * the counter plane) by enqueueing it on this stream. */
void* bk_engine_get_stream(const bk_engine* e);

/* Geometry of the outputs */
uint64_t bk_total_cells(const bk_engine* e);     /* sum of all sequence lengths = rows of each pileup array */
int32_t  bk_n_files(const bk_engine* e);
uint64_t bk_n_slots(const bk_engine* e);         /* distinct window buckets on the device                   */
uint64_t bk_counter_len(const bk_engine* e);     /* u64 elements in one counter plane                       */
int      bk_can_shard(const bk_engine* e);       /* v8: 1 = one sample's reads may be sharded over engines (bk_counters_device_ptr,
                                                  * bk_shard_*, bk_sample_finalize_shard); 0 = the index is so large that its planes
                                                  * are kept sparse: shard whole samples instead                                      */

/* ---- per-sample protocol (mirrors one iteration of call.rs:213-293 / :298-386) ---------------------------
 * bk_sample_begin      = initialize_output_maps (call.rs:224,314): zero pileups, stats and counter planes.
 * bk_push_reads_*      = the reads of mate file `mate` (0 = -r file or R1, 1 = R2); callable repeatedly.
 * bk_sample_finish     = KMC thresholds (ci/cs/cx, per mate file) + map_kmers for mate 0 then mate 1 into the
 *                        shared arrays (call.rs:316-317), then copy-out.
 *
 * Read batches are 2-bit packed fixed-stride records (produced by bk_pack_reads or by the host itself):
 *   record r = words[r*stride_words .. +stride_words), base i in word i/16 at bits [2*(i%16), 2*(i%16)+2),
 *   A=0 C=1 G=2 T=3; lens[r] = number of valid bases (<= 16*stride_words).  A record holds one maximal
 *   ACGT run (KMC splits reads at any other symbol) or an overlapping chunk of one.
 * The host buffer may be reused as soon as the call returns. */
int bk_sample_begin(bk_engine* e);
int bk_push_reads_packed(bk_engine* e, int mate, const uint32_t* words, uint32_t stride_words,
                         const uint16_t* lens, uint64_t n_records);
/* (bk_push_reads_packed stages the batch through one of two device buffers: the copy of a batch overlaps the scan of the
 * previous one; the call blocks only when both are still in use.) */
/* K0 from device memory (v7): the sequence lines are already resident (d_bases: bytes back to back, d_offsets: u64[n_reads + 1]);
 * the engine packs them into 2-bit records on its stream and scans them -- no copy, no host work beyond the launches.
 * total_bases = offsets[n_reads] - offsets[0] and longest_read (bases; sizes the record stride) are the host's to know.
 * d_bases may have any alignment (a sub-buffer of a larger device allocation is fine); d_offsets is 8-byte aligned. */
int bk_push_reads_ascii_device(bk_engine* e, int mate, const void* d_bases, const void* d_offsets, uint64_t n_reads,
                               uint64_t total_bases, uint32_t longest_read);
/* Same, for a batch that is already resident in device memory (no copy; asynchronous on the engine stream). */
int bk_push_reads_packed_device(bk_engine* e, int mate, const void* d_words, uint32_t stride_words,
                                const void* d_lens, uint64_t n_records);

/* K0 on the device + asynchronous ingest.  `buf` holds the sequence lines of n_reads reads back to back (read i =
 * buf[offsets[i] .. offsets[i+1]), any symbols); the engine copies them into a pinned staging slot, uploads them,
 * packs them into 2-bit records on the GPU (same splitting / chunking rules as bk_pack_reads) and scans them.  The
 * call returns as soon as the staging copy is made -- `buf` may be reused immediately -- and up to three batches
 * are in flight, so FASTQ parsing overlaps the copy, the packing and the scan.  bk_sample_finish waits for all. */
int bk_push_reads_ascii(bk_engine* e, int mate, const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads);

/* Base-quality masking (`bronko call --min-base-qual`).  `qual` holds the reads' quality lines at the same offsets as `buf`
 * (Phred+33); a base whose quality byte is below '!' + min_qual is treated as N, so the batch gives exactly the records of the
 * same call on the sequence lines with those bases replaced by N.  min_qual is 0..93 (BK_ERR_INVALID otherwise); 0 is the
 * unqualified call (`qual` is not read).  The _device form takes the quality lines in device memory, any alignment. */
int bk_push_reads_ascii_qual(bk_engine* e, int mate, const uint8_t* buf, const uint8_t* qual, const uint64_t* offsets, uint64_t n_reads,
                             int min_qual);
int bk_push_reads_ascii_qual_device(bk_engine* e, int mate, const void* d_bases, const void* d_quals, const void* d_offsets,
                                    uint64_t n_reads, uint64_t total_bases, uint32_t longest_read, int min_qual);

/* Multi-GPU hook: the only additive quantity is the per-k-mer occurrence counter plane.
 * (Its u64 elements are difference arrays and counters whose sums wrap modulo 2^64 -- opaque to the host, linear.)
 * A host that shards one sample's reads over several GPUs all-reduces (sum, u64) each plane in place between
 * the last push and bk_sample_finish.  The pointer is device memory of bk_counter_len() u64; call this after the
 * sample's bk_sample_begin (a plane nothing was pushed to yet is zeroed here, not at begin). */
int bk_counters_device_ptr(bk_engine* e, int mate, void** d_ptr);

/* Runs the threshold + map_kmers kernels for mates [0, n_mates) on the device (asynchronous). */
int bk_sample_finalize(bk_engine* e, int n_mates);

/* Multi-GPU, cheaper form: instead of all-reducing the planes and finalizing everything on every rank, REDUCE-SCATTER each
 * plane over the n ranks (n divides 64; bk_counter_len() is a multiple of 64 and a part never cuts a counter row), then
 *   bk_sample_finalize_shard(e, n_mates, rank, n)   maps only the rank-th of n equal parts of each plane -- the part the
 *                                                   reduce-scatter left summed in place on this rank -- into this rank's
 *                                                   pileup arrays and statistics;
 *   all-reduce MAX the two depth planes and SUM the two #k-mer planes (bk_pileup_device_ptr: 4 planes of total_cells * 4
 *   u64, depth fwd, depth rev, #k-mers fwd, #k-mers rev), and SUM the bk_shard_sums_device_ptr vector;
 *   bk_sample_merge_shards(e)                       installs the summed statistics; bk_sample_download then returns the
 *                                                   same results as the all-reduce form on every rank.
 * (map_kmers' votes are max / += per k-mer, so maps of disjoint sets of k-mers combine by max / sum.) */
int bk_sample_finalize_shard(bk_engine* e, int n_mates, int shard, int n_shards);
int bk_shard_sums_device_ptr(bk_engine* e, void** d_ptr, uint64_t* len);
int bk_sample_merge_shards(bk_engine* e);
/* Transport of the planes for the sharded finalize (v7).  The u64 elements of a plane are counts and differences of counts; as
 * signed numbers they are small, and a reduce-scatter of a narrower copy moves a half or a quarter of the bytes over xGMI.  The
 * engine packs and widens on its own stream -- no host-side temporaries -- and leaves the plane itself untouched:
 *   bk_shard_measure(e, mate, &d_max)        optional.  d_max -> two u64 on the device: the largest E count and the largest |V
 *                                            element| of this rank's plane (asynchronous).  The host all-reduces them (MAX) and
 *                                            picks the width: 16 needs max|V| * n <= 32767 and max E < 2^32; 32 needs
 *                                            max(E, |V|) * n <= 2^31 - 1; 64 always fits.
 *   bk_shard_transport(e, mate, n, width, &d_send, &part_bytes, &d_recv)
 *                                            packs the plane (asynchronous) into n parts of part_bytes bytes at d_send: int32
 *                                            words that hold two 16-bit lanes each (width 16: a V element v as v + 32767 / n,
 *                                            an E count as four 8-bit digits -- unsigned lanes whose sums stay below 2^16 add
 *                                            up inside 32-bit additions; RCCL has no 16-bit integer type), int32 elements
 *                                            (32), or the plane itself (64: d_send is the plane).  The host reduce-scatters(sum)
 *                                            d_send -- element type int32 for widths 16 and 32, int64 for 64 -- leaving this
 *                                            rank's part at d_recv.  A packer that meets an element beyond (lane maximum) / n
 *                                            raises a flag that travels with bk_shard_sums_device_ptr to every rank.
 *   bk_shard_received(e, mate, shard, n, width)  widens the received part (asynchronous); bk_sample_finalize_shard(.., shard, n)
 *                                            then maps it instead of the plane's own elements.
 *   bk_transport_overflow(e, &flag)          synchronises; flag = some sample since the last call met such an element (its results are
 *                                            garbage: repeat it wider).  bk_sample_download reports the same as BK_ERR_RANGE.
 * The transport and `reduced` buffers are allocated once, at the first call, for the largest shard count and width there is:
 * pointers stay valid for the engine's lifetime.  Width 16 is refused (BK_ERR_INVALID) where it would send no fewer bytes than
 * width 32 -- every E count travels as four 16-bit lanes, so with many shards, or a plane that is mostly E counts, it does not pay. */
int bk_shard_measure(bk_engine* e, int mate, void** d_max);
int bk_shard_transport(bk_engine* e, int mate, int n_shards, int width, void** d_send, uint64_t* part_bytes, void** d_recv);
int bk_shard_received(bk_engine* e, int mate, int shard, int n_shards, int width);
int bk_transport_overflow(bk_engine* e, int* overflowed);
/* full_kmer_stats with a sharded finalize (v6): a k-mer that touches no window bucket sits in the statistics table of every
 * rank whose reads held it, and KMC's "unique (counted) k-mers" (call.rs:1190-1199) want it once, with its total count.  Between
 * the last push and bk_sample_finalize_shard every rank
 *   bk_kmer_table_partition(e, n, &keys, &counts, off)   lists its table's entries grouped by owner rank (a hash of the key):
 *                                                        device arrays of off[n] keys (u64) / counts (u32), group r = entries
 *                                                        [off[r], off[r + 1]); synchronises (the host sizes the exchange);
 *   exchanges the groups (all-to-all: group r goes to rank r);
 *   bk_kmer_table_replace(e, keys, counts, n_received)   rebuilds its table from what it received (equal keys add up).
 * bk_sample_finalize_shard refuses n_shards > 1 with full_kmer_stats unless the table was replaced in this sample.  The totals
 * then travel in the bk_shard_sums_device_ptr vector like the other statistics. */
int bk_kmer_table_partition(bk_engine* e, int n_parts, void** d_keys, void** d_counts, uint64_t* part_off /* [n_parts + 1] */);
int bk_kmer_table_replace(bk_engine* e, const void* d_keys, const void* d_counts, uint64_t n);
/* Device pointers of the finalized arrays: 4 planes (fwd depth, rev depth, fwd #kmers, rev #kmers) of
 * total_cells*4 u64 each, contiguous, in (file, seq, pos, base) order.  The pointer is the engine's for its lifetime; what it
 * points at holds a finalized sample until the next bk_sample_begin on this engine.  The arrays are zeroed for the next sample
 * on the engine's stream by bk_sample_begin or, where that launch can be saved, by the sample's first push (inside its Level 2
 * launch) or its finalize: between bk_sample_begin and bk_sample_finalize their contents are unspecified. */
int bk_pileup_device_ptr(bk_engine* e, void** d_ptr);
/* Synchronises and copies results to host memory.  Any pointer may be NULL (skipped).
 *   fwd_depth/rev_depth/fwd_nk/rev_nk : total_cells*4 u64 each    (OutputData.counts, call.rs:1235-1239)
 *   stats   : n_mates * n_files * 3 u64  (perfect, variant, unique) per mate file (call.rs:1272)
 *   present : n_mates * n_files bytes, 1 iff the file has a key in map_kmers' returned map
 *   kmer_stats : n_mates * 4 u64 = [0] records pushed, [1] k-mer occurrences scanned (KMC "Total no. of k-mers"),
 *                [2] distinct k-mers ("No. of unique k-mers"), [3] distinct k-mers kept by -ci/-cx ("No. of unique
 *                counted k-mers").  With full_kmer_stats = 0, [2] = 0 and [3] counts index-touching k-mers only;
 *                if the k-mer table could not grow any further and overflowed, [2] = [3] = UINT64_MAX.                */
int bk_sample_download(bk_engine* e, int n_mates, uint64_t* fwd_depth, uint64_t* rev_depth, uint64_t* fwd_nk,
                       uint64_t* rev_nk, uint64_t* stats, uint8_t* present, uint64_t* kmer_stats);
/* bk_sample_finalize + bk_sample_download */
int bk_sample_finish(bk_engine* e, int n_mates, uint64_t* fwd_depth, uint64_t* rev_depth, uint64_t* fwd_nk,
                     uint64_t* rev_nk, uint64_t* stats, uint8_t* present, uint64_t* kmer_stats);

/* ---- the sample's k-mer counts (optional; `bronko call --keep-kmer-info`, call.rs:1202-1211, :404-420) ------------------
 * Count table of every strand-specific k-mer of the pushed records, per mate file: the KMC -k -b -ci -cs -cx contract of
 * SURVEY.md A.3 (a k-mer is kept iff ci <= its true count <= cx; the count reported is min(count, cs)).  A second pass over the
 * records of every push (all four push paths), on the engine's stream; the select and the sort run inside bk_sample_finalize.
 * table_log2 = initial capacity 2^table_log2 slots (10..31; it grows like full_kmer_stats' table); 0 disables and frees.
 * Between samples only (BK_ERR_STATE inside one).  Per engine: forks enable their own. */
int bk_kmer_dump_enable(bk_engine* e, uint32_t table_log2);
/* After bk_sample_finalize / _finish: synchronises; n_kept = entries that pass ci/cx, n_distinct = distinct k-mers of the mate.
 * BK_ERR_STATE if the dump was not enabled for this sample, the mate was not finalized, or the sample was finalized by shards.
 * n_kept = n_distinct = UINT64_MAX if the table overflowed at 2^31 slots.  Valid until the engine's next bk_sample_begin. */
int bk_kmer_dump_size(bk_engine* e, int mate, uint64_t* n_kept, uint64_t* n_distinct);
/* Copies min(cap, n_kept) entries, ascending by k-mer: MSB-first 2-bit codes (A=0 C=1 G=2 T=3), counts = min(count, cs). */
int bk_kmer_dump_download(bk_engine* e, int mate, uint64_t* kmers, uint64_t* counts, uint64_t cap);

/* ---- amplicon primers (`bronko call --primers`; additive, still v8) ---------------------------------------------
 * n primers, each ACGT/acgt only, 12..64 bases, written 5'->3' as synthesised; at most 1024; max_mismatches 0..3 (BK_ERR_INVALID
 * on a violation).  n = 0 clears them.  Between samples only (BK_ERR_STATE inside one).  Per engine: forks set their own.
 * While primers are set, every read pushed is trimmed.  A letter is valid if it is ACGT/acgt (and, with min_qual, at or above
 * the threshold); at the 5' end the longest primer P with Hamming(read[0:L], P) <= max_mismatches (case folded) that lies inside
 * the read's leading run of valid letters is treated as N, at the 3' end the longest P whose reverse complement matches
 * read[n-L:n] inside the trailing run; the 3' match is made on the read as pushed.  If both lie in one run and overlap, the whole
 * read is N.  Only whole primers anchored at a read end match: no indels, no internal or partial occurrences, and none at the
 * ends of a run so long that it is cut into several records.  Every result equals that of the same pushes, without primers, of
 * the reads with those letters replaced by N. */
#define BK_PRIMER_MIN_LEN 12
#define BK_PRIMER_MAX_LEN 64
#define BK_MAX_PRIMERS 1024
#define BK_PRIMER_MAX_MISMATCHES 3
int bk_primers_set(bk_engine* e, const uint8_t* const* seqs, const uint32_t* lens, uint32_t n, int max_mismatches);
/* Packed records with their end flags, one byte a record: bit 0 = the record's first base is its read's first letter, bit 1 =
 * its last base is its read's last letter (a chunk of a cut run carries neither); bk_pack_reads_flat_ends writes them.  With
 * primers or adapters set the flag-less bk_push_reads_packed / _device return BK_ERR_STATE (their records would go untrimmed);
 * with neither set these behave as the plain calls and `ends` is not read.  The _device form trims a copy: the caller's records stay as
 * they are. */
int bk_push_reads_packed_ends(bk_engine* e, int mate, const uint32_t* words, uint32_t stride_words, const uint16_t* lens, const uint8_t* ends,
                              uint64_t n_records);
int bk_push_reads_packed_ends_device(bk_engine* e, int mate, const void* d_words, uint32_t stride_words, const void* d_lens, const void* d_ends,
                                     uint64_t n_records);
/* After bk_sample_finalize / _finish, until the engine's next bk_sample_begin (synchronises): out = {reads trimmed at the 5'
 * end, reads trimmed at the 3' end, bases masked} of the mate file.  The counters are taken on the records: an end whose run
 * of valid letters is shorter than k makes no record (it holds no k-mer, trimmed or not) and is not counted.  BK_ERR_STATE if
 * no primers were set when the sample began. */
int bk_primer_stats(bk_engine* e, int mate, uint64_t out[3]);

/* ---- 3' sequencing adapters (`bronko call --adapter`; additive, still v8) -----------------------------------------
 * n adapters, each ACGT/acgt only, 8..64 bases, written 5'->3' as they appear in a read that runs through its insert; at most 8;
 * min_overlap O: 3 .. the shortest adapter; max_error_rate E: 0 .. 0.3 (BK_ERR_INVALID on a violation, with the adapter or the
 * parameter named).  n = 0 clears them.  Between samples only (BK_ERR_STATE inside one).  Per engine: forks set their own.
 * While adapters are set, every read pushed is cut.  With R = the read's maximal suffix of valid letters (valid as for the
 * primers), r its length and s1 its start: a position p, 0 <= p <= r - O, matches an adapter A of LA bases when, with
 * l = min(LA, r - p), Hamming(R[p : p + l], A[0 : l]) <= floor(E * l) (case folded; the floor of the product in double): the
 * whole adapter anywhere in R, or a prefix of at least O bases at R's end.  The read is truncated to s1 + p letters for the
 * smallest matching p over all adapters.  Substitutions only, no indels; the leftmost match wins, not the best; nothing in
 * front of R (an adapter before an N or a masked base) is found; a run so long that it is cut into several records is left as
 * it is.  The cut is made after quality masking and before the primers, which see the truncated read.  Every result equals
 * that of the same pushes, without adapters, of the truncated reads.
 * The records' end flags are needed as for the primers: with adapters set the flag-less bk_push_reads_packed / _device return
 * BK_ERR_STATE. */
#define BK_ADAPTER_MIN_LEN 8
#define BK_ADAPTER_MAX_LEN 64
#define BK_MAX_ADAPTERS 8
#define BK_ADAPTER_MIN_OVERLAP 3
#define BK_ADAPTER_MAX_ERROR_RATE 0.3
int bk_adapters_set(bk_engine* e, const uint8_t* const* seqs, const uint32_t* lens, uint32_t n, uint32_t min_overlap, double max_error_rate);
/* After bk_sample_finalize / _finish, until the engine's next bk_sample_begin (synchronises): out = {reads cut, bases removed}
 * of the mate file.  The counters are taken on the records: an R shorter than k makes no record (it holds no k-mer, cut or not)
 * and is not counted.  BK_ERR_STATE if no adapters were set when the sample began. */
int bk_adapter_stats(bk_engine* e, int mate, uint64_t out[2]);

/* ---- after the pileup, on the device (optional) ----------------------------------------------
 * For the sample just finalized, asynchronously on the engine's stream:
 *     pick_best_genome / pick_best_genome_paired   call.rs:422-502  (ties -> lowest file id; statistics summed over mates)
 *     get_baseline_noise                           call.rs:799-967  (IEEE doubles in upstream's order; one thread per
 *                                                                    sequence walks the window, see bk_caller.hip)
 *     call_variants                                call.rs:969-1150 (one thread per position)
 * A host with many samples in flight (one engine / fork each) never waits between a sample's reads and its records:
 *     bk_sample_begin .. bk_push_reads_* .. bk_sample_finalize .. bk_sample_call   (all asynchronous)
 *     bk_sample_download_calls                                                        (synchronises, copies the records)
 * The records come back sorted by (sequence, position, alternative base) = upstream's order within a sequence;
 * breadth = covered / positions, depth = coverage / covered (call.rs:1144-1145).  af is exact (one division); sor is the
 * device's ln() of exact ratios -- a host that prints it may re-derive it from the DP4 counts. */
typedef struct {            /* CallArgs fields that reach calling (cli.rs:92-135; defaults consts.rs:2-21) */
    int32_t  k;
    int32_t  no_end_filter, no_strand_filter, no_strand_balance_filter;
    double   min_af;                /* 0.03 */
    double   strand_balance_ratio;  /* 0.1  */
    double   strand_odds_max;       /* 6.0  */
    double   variant_multiplier;    /* 1.5  */
    uint64_t n_per_strand;          /* 2    */
    uint64_t min_depth;             /* 300  */
    uint64_t min_variant_depth;     /* 3    */
} bk_call_params;
typedef struct {            /* call.rs:776-789 VcfRecord */
    int32_t  seq_id;                /* index of the sequence inside the selected genome file */
    uint8_t  ref_base, alt_base;    /* 2-bit codes (A C G T) */
    uint16_t pad;
    uint64_t pos;                   /* 1-based */
    uint64_t fwd_ref, rev_ref, fwd_alt, rev_alt, depth;
    double   af, sor;
} bk_call_record;
typedef struct {
    int32_t  file_id;               /* selected genome file, -1 = none (call.rs:229-235: the host reports and exits) */
    uint32_t pad;
    uint64_t n_records;             /* records produced (all of them were copied iff <= cap) */
    uint64_t n_major, n_minor;      /* AF >= 0.5 / below */
    uint64_t covered, positions, coverage;
} bk_call_summary;
void bk_call_params_default(bk_call_params* p);
int  bk_sample_call(bk_engine* e, int n_mates, const bk_call_params* p);
int  bk_sample_download_calls(bk_engine* e, bk_call_summary* summary, bk_call_record* records, uint64_t cap);
/* Diagnostic: Noise.max of get_baseline_noise (call.rs:953-962) for every position of the genome bk_sample_call selected, in
 * (sequence, position) order -- what call_variants' AF filter compared with (call.rs:1107).  `cap` doubles at `out`; returns
 * the number of positions through *n (0 when no genome was selected).  Synchronises. */
int  bk_sample_download_noise(bk_engine* e, double* out, uint64_t cap, uint64_t* n);

/* ---- per-sample consensus (`bronko call --consensus`; additive, still v8) -------------------------------------------------
 * One letter per position of the genome bk_sample_call selected, made from the two depth planes where they are; only the
 * letters travel.  For a position, tot[b] = forward + reverse depth of base b (A C G T), depth = their sum:
 *   depth < min_depth                 N, the position is masked;
 *   else                              the bases in descending order of tot (equal counts: ascending base code) are taken one by
 *                                     one, their counts summed in cum, until (double)cum >= min_freq * (double)depth -- at least
 *                                     one is taken --, then every further base whose count equals the last taken one's joins
 *                                     them; a base with count 0 is never taken.  The set as a bit mask (A = 1, C = 2, G = 4,
 *                                     T = 8) indexes "-ACMGRSVTWYHKDBN".
 * A set of one base is called, a larger one ambiguous (all four print as N); a called base that differs from the reference code
 * of the cell (a non-ACGT reference letter counts as A, as in call_variants) is a substitution.  Integer arithmetic but for the
 * one product.  No end, strand or noise filter (the consensus is the pileup's majority, independent of the records), no indels here
 * (bk_sample_consensus_indels applies the sample's to these letters): the letters have the reference's length, in (sequence,
 * position) order.
 * min_depth >= 1 and 0 <= min_freq <= 1 (BK_ERR_INVALID otherwise, the parameter named).
 *   bk_sample_consensus            after the sample's bk_sample_call (BK_ERR_STATE before it, inside a sample, and after a later
 *                                  bk_sample_begin); asynchronous on the engine's stream.  Its buffers -- a byte per cell of the
 *                                  largest genome, and the summary -- are allocated at the engine's first call: an engine that never
 *                                  asks allocates and launches nothing.  Per engine: forks own theirs.
 *   bk_sample_download_consensus   synchronises; copies min(cap, positions) letters (letters may be NULL).  No genome selected:
 *                                  file_id = -1, every tally 0, no letters. */
typedef struct { uint64_t min_depth; double min_freq; } bk_consensus_params;
typedef struct {
    int32_t  file_id;               /* the genome bk_sample_call selected, -1 = none */
    uint32_t pad;
    uint64_t positions;             /* letters there are = positions of the genome = called + ambiguous + masked */
    uint64_t called, ambiguous, masked;
    uint64_t substitutions;         /* called positions whose base is not the reference's */
} bk_consensus_summary;
void bk_consensus_params_default(bk_consensus_params* p);   /* 10, 0.5 */
int  bk_sample_consensus(bk_engine* e, const bk_consensus_params* p);
int  bk_sample_download_consensus(bk_engine* e, bk_consensus_summary* summary, uint8_t* letters, uint64_t cap);

/* ---- per-sample minor alleles (`bronko call --contamination`; additive, still v8) --------------------------------------------------
 * Which bases are present at every position of the genome bk_sample_call selected: one byte per position, the present mask, made
 * from the two depth planes where they are; only the bytes travel.  With tot[b] and depth as bk_sample_consensus defines them, bit b
 * of the byte (A = 1, C = 2, G = 4, T = 8) is set iff both hold:
 *   tot[b] >= min_reads
 *   (double)tot[b] >= min_freq * (double)depth
 * The upper four bits are 0.  Integer arithmetic but for the one product.  No end, strand or noise filter, as for the consensus; the
 * bytes lie in (sequence, position) order, as the consensus letters do.  The summary: positions, mixed = the positions with at least
 * two bits set, present = the number of set bits.
 * min_reads >= 1 and 0 <= min_freq <= 1 (BK_ERR_INVALID otherwise, the parameter named).
 *   bk_sample_minor_alleles            the call order of bk_sample_consensus: after the sample's bk_sample_call (BK_ERR_STATE before
 *                                      it, inside a sample, and after a later bk_sample_begin); asynchronous on the engine's stream
 *                                      (minor_alleles_kernel, bk_caller.hip).  Its buffers -- a byte per cell of the largest genome,
 *                                      and the summary -- are allocated at the engine's first call: an engine that never asks
 *                                      allocates and launches nothing.  Per engine: forks own theirs.  Independent of
 *                                      bk_sample_consensus: either may run without the other, in either order.
 *   bk_sample_download_minor_alleles   synchronises; copies min(cap, positions) bytes (masks may be NULL).  No genome selected:
 *                                      file_id = -1, every tally 0, no bytes. */
typedef struct { uint64_t min_reads; double min_freq; } bk_minor_params;
typedef struct {
    int32_t  file_id;               /* the genome bk_sample_call selected, -1 = none */
    uint32_t pad;
    uint64_t positions;             /* bytes there are = positions of the genome */
    uint64_t mixed;                 /* positions with at least two bases present */
    uint64_t present;               /* set bits over all positions */
} bk_minor_summary;
void bk_minor_params_default(bk_minor_params* p);   /* 10, 0.03 */
int  bk_sample_minor_alleles(bk_engine* e, const bk_minor_params* p);
int  bk_sample_download_minor_alleles(bk_engine* e, bk_minor_summary* summary, uint8_t* masks, uint64_t cap);

/* ---- per-region depth report (`bronko call --regions / --region-window`; additive, still v8) -------------------------------
 * Which stretches of the selected genome dropped out, and how deep the rest is, from the two depth planes where they are; a few
 * numbers per region travel.  The rule, all of it integer arithmetic:
 *   depth[p]   of a position p of the selected genome = the sum over the four bases of forward + reverse depth (what the
 *              consensus thresholds), in u64.
 *   region     a half-open range [start, end) of one sequence (`seq`: its index within the genome file) of one genome file, with
 *              0 <= start < end <= the sequence's length; L = end - start.  There is no cap on L.
 *   per region sum     the sum of depth over the region, in u64
 *              min, max
 *              median  the element at index (L - 1) / 2 of the region's depths sorted ascending: the lower median (L = 2 gives
 *                      the smaller value), exact over the whole u64 range
 *              covered the number of positions with depth >= min_depth (min_depth >= 1)
 *   mean       printed from integers only: m = (100 * sum) / L, written as m / 100, ".", two digits of m % 100
 *   per sample n_regions = the selected genome file's regions; full: covered == L; empty: covered == 0; partial: the rest.
 *   bk_regions_set                    validates every region against the index (file, sequence, bounds: BK_ERR_INVALID, the
 *                                     message names the entry) and replaces the engine's table between samples (BK_ERR_STATE
 *                                     inside one); n = 0 clears; at most BK_MAX_REGIONS.  The regions are kept grouped by genome
 *                                     file, in the caller's order within a file.  The result buffers are allocated here: a sample
 *                                     allocates nothing, an engine that never sets regions allocates and launches nothing.  Per
 *                                     engine: forks set their own.
 *   bk_sample_region_depths           after the sample's bk_sample_call (BK_ERR_STATE before it, inside a sample, after a later
 *                                     bk_sample_begin, and with no regions set; BK_ERR_INVALID for min_depth == 0); asynchronous on
 *                                     the engine's stream.
 *   bk_sample_download_region_depths  synchronises; copies min(cap, n_regions) rows, in the order they were set (out may be
 *                                     NULL).  No genome selected: file_id = -1, n_regions and every tally 0, no rows. */
#define BK_MAX_REGIONS (1u << 22)
typedef struct { int32_t file_id; uint32_t seq; uint32_t start, end; } bk_region;   /* seq: index within the file */
typedef struct { uint64_t sum, min, max, median, covered; } bk_region_depth;
typedef struct { int32_t file_id; uint32_t n_regions; uint64_t full, partial, empty; } bk_region_summary;
int  bk_regions_set(bk_engine* e, const bk_region* regions, uint64_t n);
int  bk_sample_region_depths(bk_engine* e, uint64_t min_depth);
int  bk_sample_download_region_depths(bk_engine* e, bk_region_summary* summary, bk_region_depth* out, uint64_t cap);

/* ---- short insertions and deletions from the reads (`bronko call --indels`; additive, still v8) ----------------------------
 * A k-mer that spans an indel is no reference k-mer and no neighbour of one: the pileup only sags there.  A read with one indel
 * follows the reference on one diagonal up to the breakpoint and on another behind it; the difference of the two diagonals is
 * the indel's signed length.  A pass of its own over each batch's records (indel_scan_kernel, behind the scan of the same
 * records) finds the two diagonals from anchor k-mers.  The rule, all of it integer arithmetic:
 *   unit       a record: a run of at least k valid letters as the packers make it, after the trimming stage -- what the scan
 *              reads; a run that the trimming leaves with fewer than k letters is no record and is not counted.  n = its
 *              length; a record of n < 2k is counted in `records` and otherwise ignored.  The index has exactly one genome file (any number of sequences).
 *   anchor k-mer  a k-mer whose canonical form is a reference k-mer (id < n_full) that starts at exactly one cell of the genome,
 *              counting both strands, the genome's k-mers read as the index reads them (a letter that is not ACGT stands for A).
 *              It gives that cell and a strand: against the reference iff the read's k-mer and the cell's k-mer differ in whether
 *              they were reverse-complemented to become canonical.
 *   anchors    from the record's first base the k-mers at offsets 0, 8, 16, 24 are tried in that order (while offset + k <= n),
 *              from its last base the offsets n - k, n - k - 8, n - k - 16, n - k - 24 (while >= 0); the first anchor k-mer from
 *              each end is that end's anchor.  Both must exist and agree on the strand.  r' = the record oriented along the
 *              reference (its reverse complement if the strand says so); a < b the anchors' offsets in r', c_a, c_b their cells.
 *              a + k <= b, else the record is ignored.  Such a record is `anchored`.
 *              dL = c_a - a, dR = c_b - b, delta = dR - dL.  Ignored: |delta| > max_len (counted `discordant`); the two anchors
 *              in different sequences; the cells [min(dL, dR), max(dL, dR) + n) leave that sequence or hold a letter that is
 *              not ACGT (these three are not counted).
 *   delta = 0  m = Hamming(r', ref[dL, dL + n)).  m <= max_mismatches: the record is `ref_spanning` for the sites dL + a + k ..
 *              dL + b: +1 at cell dL + a + k, -1 at cell dL + b + 1 of the per-cell difference array `span`.  Else `discordant`.
 *   delta > 0  a deletion of D = delta.  For p in [a + k, b]: m(p) = #{j < p: r'[j] != ref[dL + j]} + #{j >= p: r'[j] !=
 *              ref[dR + j]}; the smallest p that minimises m(p); m(p) > max_mismatches: `discordant`.  pos = dL + p.  F = the
 *              first cell of the stretch of ACGT letters of the sequence that holds pos - 1.  While pos - 1 > F and ref[pos - 1]
 *              = ref[pos + D - 1]: pos -= 1.  Event (pos, deletion, D).
 *   delta < 0  an insertion of I = -delta.  a + k <= b - I, else `discordant`.  For p in [a + k, b - I]: m(p) = #{j < p: r'[j] !=
 *              ref[dL + j]} + #{j >= p + I: r'[j] != ref[dR + j]}; smallest minimising p, `discordant` as above.  S = r'[p, p + I),
 *              pos = dL + p, F as above.  While pos - 1 > F and ref[pos - 1] = the last base of S: rotate S right by one,
 *              pos -= 1.  Event (pos, insertion, I, S); insertions at one place with different S are different events.
 *   per event  `supporting` records per strand: fwd along the reference, rev against it.  Both mate files add into one table and
 *              one span array.  ref_span = the prefix sum of span at pos; support = fwd + rev.  Reported iff support >= min_reads
 *              and support * 1000000 >= min_af_ppm * (support + ref_span), in u64.
 *   AF         printed from integers: t = 10000 * support / (support + ref_span), as t / 10000, ".", four digits of t % 10000.
 *   bk_indels_enable           between samples (BK_ERR_STATE inside one); NULL disables and frees.  max_len 1..BK_INDEL_MAX_LEN,
 *                              max_mismatches 0..8, table_log2 10..24, an index of one genome file with a window (BK_ERR_INVALID
 *                              otherwise).  The genome has k to 2^27 - 1 positions: only then does the engine hold the
 *                              reverse-complemented reference that reads against the reference are compared with
 *                              (BK_ERR_UNSUPPORTED otherwise, the message says so).  Allocates all the feature needs (the event table of 2^table_log2 slots, as many rows,
 *                              span, one bit per reference k-mer: it starts at one cell) -- a sample allocates nothing; an engine
 *                              that never enables it allocates and launches nothing.  Per engine: forks set their own.  A sample
 *                              that began before the call has no events.
 *   bk_sample_indels           after the sample's bk_sample_finalize (bk_sample_call is not needed): BK_ERR_STATE inside a sample,
 *                              before any finalize, and when the feature was not enabled as the sample began; BK_ERR_INVALID for
 *                              min_reads == 0 or min_af_ppm > 1000000.  Prefix-sums span, selects the rows; asynchronous on the
 *                              engine's stream; may be repeated with other parameters.
 *   bk_sample_download_indels  synchronises; copies min(cap, reported) rows in no particular order (records may be NULL).
 *                              `candidates` = the distinct events of the sample.  A table that met more of them than it holds
 *                              loses nothing silently: overflow = 1 in the summary and BK_ERR_INVALID ("more than 2^n distinct
 *                              candidate events").
 *   bk_sample_download_indel_span  the prefix-summed span array of all cells (cap >= bk_total_cells, BK_ERR_INVALID otherwise).
 * bk_indel_record: cell = pos; len > 0 a deletion of len, < 0 an insertion of -len; seq = S, its base t at bits [2t, 2t + 2),
 * A C G T = 0 1 2 3 (0 for a deletion). */
#define BK_INDEL_MAX_LEN 32
typedef struct { uint32_t max_len, max_mismatches, table_log2; } bk_indel_config;   /* table_log2 10..24 */
typedef struct { uint64_t min_reads; uint32_t min_af_ppm; } bk_indel_params;
typedef struct { uint32_t cell; int32_t len; uint32_t fwd, rev, ref_span, pad; uint64_t seq; } bk_indel_record;
typedef struct { uint64_t records, anchored, ref_spanning, supporting, discordant, candidates, reported; int32_t overflow; } bk_indel_summary;
int  bk_indels_enable(bk_engine* e, const bk_indel_config* cfg);
int  bk_sample_indels(bk_engine* e, const bk_indel_params* p);
int  bk_sample_download_indels(bk_engine* e, bk_indel_summary* summary, bk_indel_record* records, uint64_t cap);
int  bk_sample_download_indel_span(bk_engine* e, uint32_t* span, uint64_t cap);

/* ---- the sample's indels applied to its consensus (`bronko call --consensus-indels`; additive, still v8) ---------------------
 * bk_sample_consensus writes one letter per reference position and bk_sample_indels finds the sample's insertions and deletions;
 * this step joins the two where both lie: it selects the events that reach the consensus thresholds, resolves those that
 * collide, marks the deleted letters and hands the few accepted events to the host, whose writer drops the deleted letters and
 * splices in the inserted ones.  The rule, all of it integer arithmetic but for one product:
 *   inputs     the sample's consensus letters with D = min_depth and F = min_freq of its last bk_sample_consensus; the sample's
 *              whole indel event table -- every candidate, whatever bk_sample_indels' min_reads and min_af_ppm select --; the
 *              prefix-summed span array bk_sample_indels made.
 *   per event  (cell c; a deletion of len, or an insertion of len with sequence S, exactly as bk_indel_record gives them)
 *              s = fwd + rev, r = span[c], n = s + r, in u64.
 *   accepted   iff n >= D and (double)s >= F * (double)n: the compare the consensus makes for a base.
 *   boundaries boundary b lies in front of cell b.  A deletion occupies the boundaries c .. c + len inclusive, an insertion the
 *              boundary c.  So two adjacent deletions collide, an insertion at either edge of a deletion collides with it, and
 *              two insertions at one cell collide.
 *   applied    iff on every boundary it occupies its s is strictly greater than the s of every other accepted event on that
 *              boundary.  An accepted event that is not applied is `contested`.  Equal support on a shared boundary contests both;
 *              there is one round only: an event that loses to a neighbour stays contested even when that neighbour lost too.
 *              Nothing depends on slot order, table size or launch order.
 *   effect     the letter of every cell [c, c + len) of an applied deletion becomes '-' (applied deletions share no boundary);
 *              an applied insertion puts S, upper-case ACGT along the reference, in front of cell c.
 *   tallies    candidates: the table's events; accepted = applied + contested; deletions, insertions: the applied events by
 *              kind; deleted_bases, inserted_bases: their lengths summed; frameshifts: applied events with len % 3 != 0.
 *   cap        at most BK_CONSENSUS_INDEL_MAX accepted events travel.  More: overflow = 1 in the summary and the download fails
 *              with BK_ERR_INVALID, as a full event table does (and a full event table fails this download too).
 *   bk_sample_consensus_indels           after this sample's bk_sample_consensus and bk_sample_indels: BK_ERR_STATE inside a
 *                                        sample, before either call, and when indels were not enabled as the sample began, each
 *                                        with its own message.  Asynchronous on the engine's stream.  Its buffers -- two words per
 *                                        boundary, BK_CONSENSUS_INDEL_MAX rows, the summary -- are allocated at the engine's first
 *                                        call and zeroed on the stream at every call: an engine that never asks allocates and
 *                                        launches nothing.  Per engine: forks own theirs.  A later bk_sample_consensus writes fresh
 *                                        letters and makes the step due again, so it may be repeated with other parameters.
 *                                        After it bk_sample_download_consensus returns the letters with '-' at the applied
 *                                        deletions; bk_consensus_summary's five tallies stay those of the unedited letters.
 *   bk_sample_download_consensus_indels  synchronises; copies min(cap, accepted) rows in no particular order (rows may be NULL).
 *                                        No genome selected: file_id = -1, every tally 0, no rows.
 * bk_consensus_indel_record: cell, len and seq as in bk_indel_record; support = s, ref_span = r; applied = 1 or 0 (contested). */
#define BK_CONSENSUS_INDEL_MAX 65536
typedef struct { uint32_t cell; int32_t len; uint32_t support, ref_span; uint64_t seq; uint32_t applied, pad; } bk_consensus_indel_record;
typedef struct { uint64_t candidates, accepted, applied, contested, deletions, insertions, deleted_bases, inserted_bases, frameshifts;
                 int32_t file_id, overflow; } bk_consensus_indel_summary;
int  bk_sample_consensus_indels(bk_engine* e);
int  bk_sample_download_consensus_indels(bk_engine* e, bk_consensus_indel_summary* s, bk_consensus_indel_record* rows, uint64_t cap);

/* ---- long deletions and subgenomic-RNA junctions from the reads (`bronko call --junctions`; additive, still v8) ---------------
 * A read whose two ends lie on diagonals more than BK_INDEL_MAX_LEN apart is `discordant` to bk_indels_enable and dropped there.
 * Such reads are the leader-body junctions of subgenomic RNAs, the internal deletions of defective genomes, any long deletion.
 * A pass of its own over each batch's records (junction_scan_kernel, behind the scan of the same records) counts them.  The rule,
 * all of it integer arithmetic, in bk_indels_enable's terms:
 *   unit, anchor k-mer, anchors, r', a, b, c_a, c_b, dL, dR, delta   exactly as under bk_indels_enable: a record of n < 2k is
 *              counted in `records` and otherwise ignored; a record with both anchors on one strand and a + k <= b is `anchored`.
 *   ignored    without a tally, before anything else is asked of delta: the two anchors in different sequences; the cells
 *              [min(dL, dR), max(dL, dR) + n) leave that sequence or hold a letter that is not ACGT (so a junction across a run
 *              of N of the reference is not found).
 *   delta = 0  m = Hamming(r', ref[dL, dL + n)).  m <= max_mismatches: the record is `ref_spanning` for the sites dL + a + k ..
 *              dL + b: +1 at cell dL + a + k, -1 at cell dL + b + 1 of the pass's own difference array `span` (not
 *              bk_indels_enable's: either feature works without the other).  Else `discordant`.
 *   0 < |delta| < min_len   counted `short`, nothing else: bk_indels_enable reports those.
 *   delta <= -min_len       counted `backward`, nothing else (duplications: bk_duplications_enable; copy-backs: bk_copybacks_enable).
 *   delta >= min_len        a junction of D = delta.  For p in [a + k, b]: m(p) = #{j < p: r'[j] != ref[dL + j]} + #{j >= p: r'[j]
 *              != ref[dR + j]}; the smallest p that minimises m(p); m(p) > max_mismatches: `discordant`.  pos = dL + p, F as in
 *              the indel rule.  While pos - 1 > F and ref[pos - 1] = ref[pos + D - 1]: pos -= 1.  Event (pos, D): the cells
 *              [pos, pos + D) are left out.  The record is `supporting`: fwd along the reference, rev against it.
 *   per event  reads = fwd + rev; span_donor = the prefix sum of span at pos, span_acceptor = at pos + D.  Reported iff reads >=
 *              min_reads.  Both mate files add into one table and one span array.
 *   bk_junctions_enable        as bk_indels_enable: between samples (BK_ERR_STATE inside one); NULL disables and frees.  min_len
 *                              1..2^27 - 1, max_mismatches 0..8, table_log2 10..24, an index of one genome file with a window
 *                              (BK_ERR_INVALID otherwise) and a genome of k to 2^27 - 1 positions (BK_ERR_UNSUPPORTED otherwise).
 *                              Allocates all the feature needs (the event table of 2^table_log2 slots, as many rows, span; the
 *                              anchor tables are shared with bk_indels_enable and bk_link_enable); an engine that never enables it
 *                              allocates and launches nothing.  Per engine: forks set their own.  A sample that began before the
 *                              call has no events.
 *   bk_sample_junctions        after the sample's bk_sample_finalize: BK_ERR_STATE inside a sample, before any finalize, and when
 *                              the feature was not enabled as the sample began; BK_ERR_INVALID for min_reads == 0.  Prefix-sums
 *                              span, selects the rows; asynchronous on the engine's stream; may be repeated with other parameters.
 *   bk_sample_download_junctions   synchronises; copies min(cap, reported) rows in no particular order (records may be NULL).
 *                              `candidates` = the distinct events of the sample.  A table that met more of them than it holds
 *                              loses nothing silently: overflow = 1 in the summary and BK_ERR_INVALID ("more than 2^n distinct
 *                              candidate junctions").
 *   bk_sample_download_junction_span   the prefix-summed span array of all cells (cap >= bk_total_cells, BK_ERR_INVALID otherwise).
 * bk_junction_record: cell = pos, the first cell left out; len = D; the read continues at cell pos + D. */
#define BK_JUNCTION_MAX_LEN 134217727u   /* 2^27 - 1 */
typedef struct { uint32_t min_len, max_mismatches, table_log2; } bk_junction_config;   /* table_log2 10..24 */
typedef struct { uint64_t min_reads; } bk_junction_params;
typedef struct { uint32_t cell, len, fwd, rev, span_donor, span_acceptor; } bk_junction_record;
typedef struct { uint64_t records, anchored, ref_spanning, supporting, short_, backward, discordant, candidates, reported; int32_t overflow; } bk_junction_summary;
int  bk_junctions_enable(bk_engine* e, const bk_junction_config* cfg);
int  bk_sample_junctions(bk_engine* e, const bk_junction_params* p);
int  bk_sample_download_junctions(bk_engine* e, bk_junction_summary* summary, bk_junction_record* records, uint64_t cap);
int  bk_sample_download_junction_span(bk_engine* e, uint32_t* span, uint64_t cap);

/* ---- strand-switch (copy-back, snap-back) junctions from the reads (`bronko call --copybacks`; additive, still v8) ---------------
 * bk_indels_enable and bk_junctions_enable follow a read on one strand of the reference; a read whose front anchor lies on one strand
 * and whose back anchor on the other is not even `anchored` there.  Those reads are the copy-back and snap-back defective genomes
 * (the polymerase leaves its template and copies the nascent strand back) and the hairpin artefacts of library preparation.  A pass
 * of its own over each batch's records (copyback_scan_kernel, behind the scan of the same records) counts them.  The rule, all of it
 * integer arithmetic, in bk_indels_enable's terms:
 *   unit, anchor k-mer, the offsets tried from each end   exactly as under bk_indels_enable: a record of n < 2k is counted in
 *              `records` and otherwise ignored.  The record `rec` is taken as packed, not re-oriented: its front anchor is (f, c_f,
 *              s_f), its back anchor (g, c_g, s_g); c the first cell of the reference k-mer, s "against the reference".  comp is the
 *              complement.
 *   s_f == s_g     only what the span needs, exactly as under bk_junctions_enable: r', a, b, dL, dR and the `ignored` conditions are
 *              that rule's.  A record with a + k <= b is `same_strand`; with delta = 0 and at most max_mismatches mismatches it is
 *              `ref_spanning`: +1 at cell dL + a + k, -1 at cell dL + b + 1 of this pass's own difference array `span`.  Any other
 *              same-strand record leaves no trace.
 *   s_f != s_g and f + k <= g   the record is `switched`.
 *              kind H (front along, back against): A(j) = c_f - f + j, the base expected at j is ref[A(j)]; B(j) = c_g + k - 1 + g
 *              - j, the base expected is comp(ref[B(j)]).  The read runs up the reference to a cell and comes back down from
 *              another: both arms lie at and below their breakpoints.
 *              kind T (front against, back along): A(j) = c_f + k - 1 + f - j, expected comp(ref[A(j)]); B(j) = c_g - g + j,
 *              expected ref[B(j)].  Both arms lie at and above their breakpoints.
 *   ignored    a switched record, without a further tally: c_f and c_g in different sequences; a cell A(j), 0 <= j < g, or a cell
 *              B(j), f + k <= j < n, leaves that sequence or holds a letter that is not ACGT.  (The arms' own ranges, not the whole
 *              record's: a copy-back whose arms end at the last cell of a sequence is found.)
 *   breakpoint for p in [f + k, g]: m(p) = #{j < p: rec[j] != arm A's base} + #{j >= p: rec[j] != arm B's base}; x(p) = A(p - 1),
 *              y(p) = B(p).  The p that minimises (m(p), min(x(p), y(p)), p) -- the middle term makes a read and its reverse
 *              complement choose the same pair of cells.  m > max_mismatches: `discordant`.  Else `supporting`, and `lo_first` if
 *              x <= y at that p, else `hi_first`.
 *   normalised the pairs (x + t, y - t) that the reference cannot tell apart form a run t0 <= 0 <= t1.  H: the step from (x, y) to
 *              (x + 1, y - 1) is allowed iff ref[x + 1] = comp(ref[y]); T: iff comp(ref[x]) = ref[y - 1]; the step down is the same
 *              condition at the lower pair; both cells of every pair stay inside the sequence and hold ACGT.  Of the two extreme
 *              pairs the one whose smaller cell is smaller (on a tie both are the same two cells); lo = its smaller, hi = its
 *              larger cell.  Event (kind, lo, hi); homology = t1 - t0 (the writer computes it from the reference).
 *   per event  reads = lo_first + hi_first.  With S the prefix sum of span: kind H span_lo = S[lo + 1], span_hi = S[hi + 1]; kind T
 *              span_lo = S[lo], span_hi = S[hi].  Reported iff reads >= min_reads and hi - lo >= min_dist.  Both mate files add
 *              into one table and one span array.  Same-strand backward jumps: bk_duplications_enable.
 *   bk_copybacks_enable        as bk_junctions_enable: between samples (BK_ERR_STATE inside one); NULL disables and frees.
 *                              max_mismatches 0..8, table_log2 10..24, an index of one genome file with a window (BK_ERR_INVALID
 *                              otherwise) and a genome of k to 2^27 - 1 positions (BK_ERR_UNSUPPORTED otherwise).  Allocates all the
 *                              feature needs (the event table of 2^table_log2 slots, as many rows, span; the anchor tables are shared
 *                              with bk_indels_enable, bk_junctions_enable and bk_link_enable); an engine that never enables it
 *                              allocates and launches nothing.  Per engine: forks set their own.  A sample that began before the
 *                              call has no events.
 *   bk_sample_copybacks        after the sample's bk_sample_finalize: BK_ERR_STATE inside a sample, before any finalize, and when
 *                              the feature was not enabled as the sample began; BK_ERR_INVALID for min_reads == 0.  Prefix-sums
 *                              span, selects the rows; asynchronous on the engine's stream; may be repeated with other parameters.
 *   bk_sample_download_copybacks   synchronises; copies min(cap, reported) rows in no particular order (records may be NULL).
 *                              `candidates` = the distinct events of the sample.  A table that met more of them than it holds
 *                              loses nothing silently: overflow = 1 in the summary and BK_ERR_INVALID ("more than 2^n distinct
 *                              candidate copy-backs").
 *   bk_sample_download_copyback_span   the prefix-summed span array of all cells (cap >= bk_total_cells, BK_ERR_INVALID otherwise).
 * bk_copyback_record: kind 0 = H, 1 = T; the read turns between the cells lo <= hi (hi = lo: a hairpin). */
typedef struct { uint32_t max_mismatches, table_log2; } bk_copyback_config;   /* 0..8, 10..24 */
typedef struct { uint64_t min_reads; uint32_t min_dist; } bk_copyback_params;
typedef struct { uint32_t lo, hi, kind, lo_first, hi_first, span_lo, span_hi, pad; } bk_copyback_record;
typedef struct { uint64_t records, same_strand, ref_spanning, switched, supporting, discordant, candidates, reported; int32_t overflow; } bk_copyback_summary;
int  bk_copybacks_enable(bk_engine* e, const bk_copyback_config* cfg);
int  bk_sample_copybacks(bk_engine* e, const bk_copyback_params* p);
int  bk_sample_download_copybacks(bk_engine* e, bk_copyback_summary* summary, bk_copyback_record* records, uint64_t cap);
int  bk_sample_download_copyback_span(bk_engine* e, uint32_t* span, uint64_t cap);

/* ---- junctions between two sequences of the genome file (`bronko call --chimeras`; additive, still v8) ----------------------------
 * bk_indels_enable, bk_junctions_enable, bk_copybacks_enable and bk_duplications_enable each ignore, without a tally, a record whose
 * two anchors lie in different sequences.  Those reads are the inter-segment junctions of segmented viruses, whose segments are the
 * sequences of one genome file, the reads that join virus and spike-in, and the template-switch chimeras of reverse transcription,
 * PCR and library preparation, whose rate is a quality figure of the run.  A pass of its own over each batch's records
 * (chimera_scan_kernel, behind the scan of the same records) counts them.  The rule, all of it integer arithmetic, in the terms of
 * bk_indels_enable and bk_copybacks_enable:
 *   unit, anchor k-mer, the offsets tried from each end   exactly as under bk_indels_enable: a record of n < 2k is counted in
 *              `records` and otherwise ignored.  The record `rec` is taken as packed, as bk_copybacks_enable takes it: its front
 *              anchor is (f, c_f, s_f), its back anchor (g, c_g, s_g); c the first cell of the reference k-mer, s "against the
 *              reference".  comp is the complement.  An anchor k-mer starts at exactly one cell of the whole genome file, so
 *              the k-mers of termini that the segments share make no anchors.  X = seq(c_f), Y = seq(c_g).
 *   X == Y     only what the span needs, exactly bk_copybacks_enable's `s_f == s_g` rule: a record with both anchors on one strand
 *              and a + k <= b is `same_strand`; with delta = 0, the cells [dL, dL + n) inside the sequence and ACGT only, and at
 *              most max_mismatches mismatches it is `ref_spanning`: +1 at cell dL + a + k, -1 at cell dL + b + 1 of this pass's
 *              own difference array `span`.  Every other record of one sequence leaves no trace here.
 *   X != Y and f + k <= g   the record is `crossed`, whatever the two strands are.
 *              arm A, offsets j < p: front along (s_f = 0): A(j) = c_f - f + j, the base expected at j is ref[A(j)], dA = +1;
 *              front against: A(j) = c_f + k - 1 + f - j, expected comp(ref[A(j)]), dA = -1.
 *              arm B, offsets j >= p: back along (s_g = 0): B(j) = c_g - g + j, expected ref[B(j)], dB = +1; back against:
 *              B(j) = c_g + k - 1 + g - j, expected comp(ref[B(j)]), dB = -1.
 *   ignored    a crossed record, without a further tally: a cell A(j), 0 <= j < g, leaves X or holds a letter that is not ACGT; a
 *              cell B(j), f + k <= j < n, leaves Y or holds one.  (The arms' own ranges: an arm may end at the last or begin at
 *              the first cell of its sequence.  The cells of two neighbouring sequences are neighbours in the index; each arm is
 *              held to its own sequence, so no arm walks from one into the next.)
 *   breakpoint for p in [f + k, g]: m(p) = #{j < p: rec[j] != arm A's base} + #{j >= p: rec[j] != arm B's base}; x(p) = A(p - 1),
 *              y(p) = B(p).  The p that minimises (m(p), min(x(p), y(p))) -- X and Y share no cell, so the second term is x
 *              throughout or y throughout, strictly monotonic in p: no further tie; and it makes a read and its reverse
 *              complement choose the same two cells.  m > max_mismatches: `discordant`.  Else `supporting`.
 *   normalised the pairs (x + dA t, y + dB t) that the reference cannot tell apart form a run t0 <= 0 <= t1.  The step from t to
 *              t + 1 is allowed iff the base arm A expects at cell x + dA (t + 1) equals the base arm B expects at cell y + dB t;
 *              the step down is the same condition at the lower pair; both cells of every pair stay inside their own sequence and
 *              hold ACGT.  Of the two extreme pairs the one whose smaller cell is smaller; lo < hi its two cells.  Each cell has a
 *              side: L, the read holds that cell and the cells below it (arm A along, arm B against); R, the read holds that cell
 *              and the cells above it (arm A against, arm B along).  Event (lo, side_lo, hi, side_hi): the same two cells with
 *              other sides are other events.  homology = t1 - t0 (the writer computes it from the reference).
 *   per event  `lo_first` counts the supporting records whose arm A lies at lo, `hi_first` the others: a read and its reverse
 *              complement count on opposite sides.  reads = lo_first + hi_first.  With S the prefix sum of span: a cell c with
 *              side L has span S[c + 1], with side R S[c] (span has total_cells + 2 entries).  Reported iff reads >= min_reads.
 *              Both mate files add into one table and one span array.  Key: lo | sides << 28 | hi << 32 (both cells below 2^27:
 *              never the free word).
 *   bk_chimeras_enable         as bk_copybacks_enable: between samples (BK_ERR_STATE inside one); NULL disables and frees.
 *                              max_mismatches 0..8, table_log2 10..24, an index of one genome file with a window (BK_ERR_INVALID
 *                              otherwise) and a genome of k to 2^27 - 1 positions (BK_ERR_UNSUPPORTED otherwise).  Allocates all the
 *                              feature needs (the event table of 2^table_log2 slots, as many rows, span; the anchor tables are shared
 *                              with the other anchor passes and bk_link_enable); an engine that never enables it allocates and
 *                              launches nothing.  Per engine: forks set their own.  A sample that began before the call has no
 *                              events.  A genome file of one sequence is no error: no record is crossed.
 *   bk_sample_chimeras         after the sample's bk_sample_finalize: BK_ERR_STATE inside a sample, before any finalize, and when
 *                              the feature was not enabled as the sample began; BK_ERR_INVALID for min_reads == 0.  Prefix-sums
 *                              span, selects the rows; asynchronous on the engine's stream; may be repeated with other parameters.
 *   bk_sample_download_chimeras    synchronises; copies min(cap, reported) rows in no particular order (records may be NULL).
 *                              `candidates` = the distinct events of the sample.  A table that met more of them than it holds
 *                              loses nothing silently: overflow = 1 in the summary and BK_ERR_INVALID ("more than 2^n distinct
 *                              candidate chimeras").
 *   bk_sample_download_chimera_span    the prefix-summed span array of all cells (cap >= bk_total_cells, BK_ERR_INVALID otherwise).
 * bk_chimera_record: sides bit 0 the side of lo, bit 1 the side of hi, 1 = R. */
typedef struct { uint32_t max_mismatches, table_log2; } bk_chimera_config;   /* 0..8, 10..24 */
typedef struct { uint64_t min_reads; } bk_chimera_params;
typedef struct { uint32_t lo, hi, sides, lo_first, hi_first, span_lo, span_hi, pad; } bk_chimera_record;
typedef struct { uint64_t records, same_strand, ref_spanning, crossed, supporting, discordant, candidates, reported; int32_t overflow; } bk_chimera_summary;
int  bk_chimeras_enable(bk_engine* e, const bk_chimera_config* cfg);
int  bk_sample_chimeras(bk_engine* e, const bk_chimera_params* p);
int  bk_sample_download_chimeras(bk_engine* e, bk_chimera_summary* summary, bk_chimera_record* records, uint64_t cap);
int  bk_sample_download_chimera_span(bk_engine* e, uint32_t* span, uint64_t cap);

/* ---- reads that leave the reference: records with an anchor at one end only (`bronko call --breakends`; additive, still v8) -------
 * Every pass above places a record by its two end anchors and drops, without a tally, the record of which only one end has an anchor.
 * Those are the reads that run from the virus into host DNA at an integration site, the reads with a junction inside the blind margin
 * of k + 24 bases of the other passes, the reads that run over the first or last base of a sequence, long insertions of novel sequence
 * and untrimmed adapter read-through.  A pass of its own over each batch's records (breakend_scan_kernel, behind the scan of the same
 * records) counts them.  The rule, all of it integer arithmetic, in the terms of bk_indels_enable:
 *   unit, anchor k-mer, the offsets tried from each end, r'   exactly as under bk_indels_enable: a record of n < 2k is counted in
 *              `records` and otherwise ignored.  Both ends are searched, whatever the other end gave.
 *   two anchors    only what the span needs, exactly bk_junctions_enable's: both anchors on one strand with a + k <= b, in one sequence,
 *              the cells [min(dL, dR), max(dL, dR) + n) inside it and ACGT only, delta = 0 and at most max_mismatches mismatches:
 *              `ref_spanning`, +1 at cell dL + a + k, -1 at cell dL + b + 1 of this pass's own difference array `span`.  Every other
 *              record of two anchors leaves no trace here; one of none leaves none either.
 *   one_anchor     exactly one end has an anchor.  Oriented along the reference the anchor lies at offset a of r' at cell c; d = c - a.
 *              s = seq(c); [lo, hi) is the stretch of ACGT letters of s around c.  side = L when the anchor is the left one of r'
 *              (the front anchor of a record along the reference, the back anchor of one against it): the read holds a cell and the
 *              cells below it and leaves the reference above it; else R, the mirror case.
 *   unplaced       the anchor's cells [c, c + k) do not lie in [lo, hi) (an index k-mer reads every other letter as A, so an anchor
 *              may lie over one); or side L and d < lo; or side R and d + n > hi: the end that is held runs off its stretch.
 *   extension      a match scores +1, a mismatch -BK_BREAKEND_MISMATCH_PENALTY (4).
 *              side L: P = min(n, hi - d); for p in [a + k, P]: S(p) = (p - a - k) - 5 #{j in [a + k, p): r'[j] != ref[d + j]};
 *              p* = the smallest p with the largest S.  side R: Q = max(0, lo - d); for q in [Q, a]: S(q) = (a - q) -
 *              5 #{j in [q, a): r'[j] != ref[d + j]}; q* = the largest q with the largest S.  A mismatch followed by four matches
 *              is not crossed, one followed by five is.  The walk never leaves [lo, hi): it enters no run of other letters and not
 *              the neighbouring sequence, whose cells are the next cells of the index.  Foreign bases that happen to continue the
 *              reference are held: the breakpoint lies as far from the anchor as the reference allows.
 *   held part      side L: r'[0, p*); side R: r'[q*, n).  m = its Hamming distance to ref on diagonal d (the mismatches in front of
 *              an anchor found at the second to fourth offset count).  m > max_mismatches: `discordant`.
 *   clip           n - p* (L), q* (R).  0: `through` -- the far end merely failed to anchor.  Below min_clip: `short`.  Else
 *              `supporting`.  Every one_anchor record is in exactly one of unplaced, discordant, through, short, supporting, asked
 *              in that order.
 *   event          (cell, side, tag): cell = d + p* - 1 (L), d + q* (R), the last reference base held; tag = the 16 clipped bases
 *              next to the breakpoint as they lie in r': r'[p*, p* + 16) (L), r'[q* - 16, q*) (R), base t at bits [2t, 2t + 2),
 *              A C G T = 0 1 2 3 (min_clip >= 16: a tag always exists).  Two tags at one cell are two events.
 *   per event      `fwd` / `rev` count the supporting records along / against the reference: a read and its reverse complement give
 *              the same event on opposite counters.  `site_reads`: the supporting records of (cell, side) over every tag, from an
 *              array of its own, so that events below min_reads still count.  With S the prefix sum of span: side L has span
 *              S[cell + 1], side R S[cell] (span has total_cells + 2 entries); 0 at a terminus by construction.  Reported iff
 *              fwd + rev >= min_reads.  Both mate files add into one table.  Key: cell | side << 27 | tag << 32 (a cell is below
 *              2^27: never the free word).
 *   bk_breakends_enable        as bk_junctions_enable: between samples (BK_ERR_STATE inside one); NULL disables and frees.
 *                              min_clip 16..65519, max_mismatches 0..8, table_log2 10..24, an index of one genome file with a window
 *                              (BK_ERR_INVALID otherwise) and a genome of k to 2^27 - 1 positions (BK_ERR_UNSUPPORTED otherwise).
 *                              Allocates all the feature needs (the event table of 2^table_log2 slots, as many rows, the (cell, side)
 *                              array, span; the anchor tables are shared with the other anchor passes and bk_link_enable); an engine
 *                              that never enables it allocates and launches nothing.  Per engine: forks set their own.  A sample
 *                              that began before the call has no events.
 *   bk_sample_breakends        after the sample's bk_sample_finalize: BK_ERR_STATE inside a sample, before any finalize, and when
 *                              the feature was not enabled as the sample began; BK_ERR_INVALID for min_reads == 0.  Prefix-sums
 *                              span, selects the rows; asynchronous on the engine's stream; may be repeated with other parameters.
 *   bk_sample_download_breakends   synchronises; copies min(cap, reported) rows in no particular order (records may be NULL).
 *                              `candidates` = the distinct events of the sample.  A table that met more of them than it holds
 *                              loses nothing silently: overflow = 1 in the summary and BK_ERR_INVALID ("more than 2^n distinct
 *                              candidate breakends").
 *   bk_sample_download_breakend_span   the prefix-summed span array of all cells (cap >= bk_total_cells, BK_ERR_INVALID otherwise).
 * bk_breakend_record: side 0 = L, 1 = R. */
#define BK_BREAKEND_MISMATCH_PENALTY 4
typedef struct { uint32_t min_clip, max_mismatches, table_log2; } bk_breakend_config;   /* 16..65519, 0..8, 10..24 */
typedef struct { uint64_t min_reads; } bk_breakend_params;
typedef struct { uint32_t cell, tag, side, fwd, rev, site_reads, span, pad; } bk_breakend_record;
typedef struct { uint64_t records, one_anchor, ref_spanning, supporting, short_, through, discordant, unplaced, candidates, reported; int32_t overflow; } bk_breakend_summary;
int  bk_breakends_enable(bk_engine* e, const bk_breakend_config* cfg);
int  bk_sample_breakends(bk_engine* e, const bk_breakend_params* p);
int  bk_sample_download_breakends(bk_engine* e, bk_breakend_summary* summary, bk_breakend_record* records, uint64_t cap);
int  bk_sample_download_breakend_span(bk_engine* e, uint32_t* span, uint64_t cap);

/* ---- tandem duplications and circular-origin reads (`bronko call --duplications`; additive, still v8) ----------------------------
 * The one case of a record placed by its two end anchors that the passes above leave: both anchors on one strand, the back one on a
 * diagonal behind the front one's.  bk_junctions_enable counts it `backward` and drops it.  Such a read crosses the junction between
 * the two copies of a tandem duplication (it need not hold a whole copy), or the linearisation point of a circular genome: it runs
 * to the last cell of the sequence and goes on at the first, a backward jump of the sequence's length.  A pass of its own over each
 * batch's records (duplication_scan_kernel, behind the scan of the same records) counts them.  The rule, all of it integer
 * arithmetic, in bk_indels_enable's terms:
 *   unit, anchor k-mer, anchors, r', a, b, c_a, c_b, dL, dR, delta   exactly as under bk_indels_enable: a record of n < 2k is
 *              counted in `records` and otherwise ignored; a record with both anchors on one strand and a + k <= b is `anchored`.
 *   ignored    without a tally, before anything is asked of delta: the two anchors in different sequences.  [lo, hi) are the cells
 *              of the anchors' sequence.
 *   delta = 0  as under bk_junctions_enable: the cells [dL, dL + n) lie in [lo, hi) and hold ACGT only, else the record is ignored.
 *              m = Hamming(r', ref[dL, dL + n)).  m <= max_mismatches: the record is `ref_spanning`: +1 at cell dL + a + k, -1 at
 *              cell dL + b + 1 of this pass's own difference array `span`.  Else `discordant`.
 *   delta > 0  counted `forward`, nothing else (bk_indels_enable and bk_junctions_enable report those).
 *   -min_len < delta < 0   counted `short`, nothing else.
 *   delta <= -min_len   a backward jump of E = -delta.  Ignored without a tally unless lo <= dL and dR + n <= hi.  The breakpoint's
 *              range is clipped to the sequence: p0 = max(a + k, lo - dR), p1 = min(b, hi - dL); p0 > p1: ignored.  The two arms'
 *              cells [dL, dL + p1) and [dR + p0, dR + n) hold ACGT only, else the record is ignored.  (This is the difference from
 *              bk_junctions_enable: the left arm may run to the last cell of the sequence and the right arm may begin at its
 *              first; a virtual overhang beyond either is never read.)  For p in [p0, p1]: m(p) = #{j < p: r'[j] != ref[dL + j]}
 *              + #{j >= p: r'[j] != ref[dR + j]}; the smallest p that minimises m(p); m(p) > max_mismatches: `discordant`.
 *              pos = dL + p: the read leaves the reference behind cell pos - 1 and goes on at cell pos - E; the cells
 *              [pos - E, pos) are read twice.
 *   normalised with two floors: F_L = the first cell of the stretch of ACGT letters of the sequence that holds pos - 1, F_R = the
 *              first cell of the stretch that holds pos - E.  While pos - 1 > F_L and pos - E - 1 >= F_R and ref[pos - 1] =
 *              ref[pos - E - 1]: pos -= 1.  Event (pos, E).  The record is `supporting`: fwd along the reference, rev against it.
 *   per event  reads = fwd + rev; span_start = the prefix sum of span at pos - E, span_end = at pos.  Reported iff reads >=
 *              min_reads.  Both mate files add into one table and one span array.
 *   key        pos | E << 32, both below 2^27, so never the free word; pos = hi is a legal key and a legal index of span, which has
 *              total_cells + 2 entries.
 *   bk_duplications_enable     as bk_junctions_enable: between samples (BK_ERR_STATE inside one); NULL disables and frees.  min_len
 *                              1..2^27 - 1, max_mismatches 0..8, table_log2 10..24, an index of one genome file with a window
 *                              (BK_ERR_INVALID otherwise) and a genome of k to 2^27 - 1 positions (BK_ERR_UNSUPPORTED otherwise).
 *                              Allocates all the feature needs (the event table of 2^table_log2 slots, as many rows, span; the
 *                              anchor tables are shared with bk_indels_enable, bk_junctions_enable, bk_copybacks_enable and
 *                              bk_link_enable); an engine that never enables it allocates and launches nothing.  Per engine: forks
 *                              set their own.  A sample that began before the call has no events.
 *   bk_sample_duplications     after the sample's bk_sample_finalize: BK_ERR_STATE inside a sample, before any finalize, and when
 *                              the feature was not enabled as the sample began; BK_ERR_INVALID for min_reads == 0.  Prefix-sums
 *                              span, selects the rows; asynchronous on the engine's stream; may be repeated with other parameters.
 *   bk_sample_download_duplications   synchronises; copies min(cap, reported) rows in no particular order (records may be NULL).
 *                              `candidates` = the distinct events of the sample.  A table that met more of them than it holds
 *                              loses nothing silently: overflow = 1 in the summary and BK_ERR_INVALID ("more than 2^n distinct
 *                              candidate duplications").
 *   bk_sample_download_duplication_span   the prefix-summed span array of all cells (cap >= bk_total_cells, BK_ERR_INVALID otherwise).
 * bk_duplication_record: cell = pos, the cell behind the last one read twice; len = E; the cells [pos - E, pos) are read twice. */
#define BK_DUPLICATION_MAX_LEN 134217727u   /* 2^27 - 1 */
typedef struct { uint32_t min_len, max_mismatches, table_log2; } bk_duplication_config;   /* table_log2 10..24 */
typedef struct { uint64_t min_reads; } bk_duplication_params;
typedef struct { uint32_t cell, len, fwd, rev, span_start, span_end; } bk_duplication_record;
typedef struct { uint64_t records, anchored, ref_spanning, supporting, short_, forward, discordant, candidates, reported; int32_t overflow; } bk_duplication_summary;
int  bk_duplications_enable(bk_engine* e, const bk_duplication_config* cfg);
int  bk_sample_duplications(bk_engine* e, const bk_duplication_params* p);
int  bk_sample_download_duplications(bk_engine* e, bk_duplication_summary* summary, bk_duplication_record* records, uint64_t cap);
int  bk_sample_download_duplication_span(bk_engine* e, uint32_t* span, uint64_t cap);

/* ---- which substitutions the same reads carry (`bronko call --linkage`; additive, still v8) -------------------------------------
 * The pileup says how often each substitution occurs, not whether two of them sit on the same molecules.  The reads say it: a pass
 * of its own over each batch's records (link_scan_kernel, behind the scan of the same records) keeps, per record that can be placed
 * on the reference, where it lies and where it differs; at the sample's end link_count_kernel counts, for a list of sites, the 4 x 4
 * table of the records' bases at every pair of sites that one record covers.  The rule, all of it integer arithmetic:
 *   unit       a record, as for bk_indels_enable: a run of at least k valid letters after the trimming stage, n its length.  The
 *              index has exactly one genome file.
 *   placed     bk_indels_enable's anchor rule unchanged: the k-mers at offsets 0, 8, 16, 24 from either end are tried, the first
 *              anchor k-mer from each end is that end's anchor, both exist and agree on the strand; r' = the record oriented along
 *              the reference, a < b the anchors' offsets in r', c_a, c_b their cells, a + k <= b; dL = c_a - a, dR = c_b - b.
 *              dR = dL exactly; both anchors in one sequence; the cells [dL, dL + n) inside that sequence and holding ACGT only;
 *              then m = Hamming(r', ref[dL, dL + n)) <= max_mismatches.  A record of n < 2k is never placed.
 *   tallies    every record is counted in `records` and in exactly one of `placed`, `discordant` (every check but the last one
 *              held: more than max_mismatches mismatches) and `unplaced` (all others: n < 2k, no two anchors on one strand with
 *              a + k <= b, dR != dL, other sequences, out of bounds, a letter that is not ACGT).
 *   row        a placed record leaves one bk_link_row in the sample's row store: cell0 = dL, n, strand (1: it reads against the
 *              reference), n_mm = m, and its mismatches ascending by offset: mm[3 i ..] = the offset j from cell0 (16 bits, little
 *              endian) and r'[j] (A C G T = 0 1 2 3); the entries from n_mm on are zero.
 *   covers     a placed record covers every cell of [dL, dL + n) -- no margin at its ends --; its base at cell c is r'[c - dL]: the
 *              reference's unless one of its mismatches sits there.
 *   sites      a strictly ascending list of at most BK_LINK_MAX_SITES cells (each < bk_total_cells).
 *   pairs      all i < j with both cells in one sequence and cell_j - cell_i <= max_dist, in (i, j) order; at most
 *              BK_LINK_MAX_PAIRS of them.
 *   counters   per pair, count[4 bA + bB] = the placed records of both mate files that cover both cells with base bA at cell_i
 *              and bB at cell_j, u32.  A record on either strand counts alike; overlapping mates count twice.
 *   bk_link_enable            between samples (BK_ERR_STATE inside one); NULL disables and frees.  max_mismatches 0..8,
 *                             initial_rows >= 1 (the row store's first capacity; it doubles as the sample needs), an index of one
 *                             genome file with a window (BK_ERR_INVALID otherwise) and a genome of k to 2^27 - 1 positions
 *                             (BK_ERR_UNSUPPORTED otherwise, as bk_indels_enable).  Per engine: forks enable their own.  Works with
 *                             and without bk_indels_enable; the two share their anchor tables.  A sample that began before the call
 *                             has no rows.  An engine that never enables it allocates and launches nothing.
 *   pushes                    before a batch is scanned the store has room for a row of every record of it; growing is an
 *                             allocation and a device copy on the engine's stream, and an allocation that fails is the push's
 *                             error, never a loss.  32 bytes per record pushed (room is made for every record, placed or not); a
 *                             store that grows is held beside its successor until the stream has passed the copy, then freed.
 *                             2^32 records or more in one sample are BK_ERR_UNSUPPORTED.  bk_sample_begin empties the store: an abandoned sample leaves nothing.
 *   bk_sample_linkage         after the sample's bk_sample_finalize (BK_ERR_STATE inside a sample, before any finalize, and when
 *                             the feature was not enabled as the sample began).  BK_ERR_INVALID: sites not strictly ascending or
 *                             not below bk_total_cells, more than BK_LINK_MAX_SITES, max_dist outside 1..65519, more than
 *                             BK_LINK_MAX_PAIRS pairs (the message names the count; the host enumerates, nothing is launched).
 *                             Zeroes the counters and counts; asynchronous on the engine's stream: the sites are staged in
 *                             pinned memory and uploaded on the stream, and the host waits for nothing but an earlier count
 *                             whose buffers the call replaces.  May be repeated with other sites or another max_dist on the
 *                             same sample.
 *   bk_sample_download_linkage   after the sample's finalize; synchronises; the summary and min(cap, n_pairs) rows {site_a,
 *                             site_b, count[16]} in (i, j) order (site_a, site_b are the cells; pairs may be NULL).  Before the
 *                             sample's first bk_sample_linkage there are the tallies and no pairs.
 *   bk_sample_download_link_rows the row store as it is, min(cap, placed) rows in no particular order, after the sample's
 *                             finalize; synchronises. */
#define BK_LINK_MAX_SITES 65536
#define BK_LINK_MAX_PAIRS (1u << 20)
#define BK_LINK_MAX_DIST 65519
typedef struct { uint32_t max_mismatches; uint64_t initial_rows; } bk_link_config;
typedef struct { uint32_t cell0; uint16_t n; uint8_t strand, n_mm; uint8_t mm[24]; } bk_link_row;   /* 32 bytes */
typedef struct { uint32_t site_a, site_b; uint32_t count[16]; } bk_link_pair;
typedef struct { uint64_t records, placed, unplaced, discordant, n_pairs; uint32_t n_sites, max_dist; } bk_link_summary;
int  bk_link_enable(bk_engine* e, const bk_link_config* cfg);
int  bk_sample_linkage(bk_engine* e, const uint32_t* cells, uint32_t n_sites, uint32_t max_dist);
int  bk_sample_download_linkage(bk_engine* e, bk_link_summary* summary, bk_link_pair* pairs, uint64_t cap);
int  bk_sample_download_link_rows(bk_engine* e, bk_link_row* rows, uint64_t cap);

/* ---- which triplets the reads carry at the codons of coding regions (`bronko call --codons`; additive, still v8) ------------------
 * Two substitutions inside one codon give another amino acid together than either gives alone, so amino-acid changes cannot be read
 * off the substitution calls; the rows of bk_link_enable's store can say it exactly.  A second consumer of that store: for every
 * codon of every region the caller names, how many rows carry each of the 64 triplets.  The terms row, covers and base at a cell are
 * those of bk_link_enable above: a placed record covers [cell0, cell0 + n), its base at cell c is its mismatch there, else the
 * reference's; rows of both mate files count alike, overlapping mates count twice.  The rule, all of it integer arithmetic:
 *   region     {cell0, n_codons}: the forward-strand cells [cell0, cell0 + 3 n_codons); n_codons >= 1, all cells inside one sequence and
 *              below bk_total_cells.  Regions come in any order and may overlap, nest, repeat and lie in different frames.  At most
 *              BK_CODON_MAX_REGIONS regions and BK_CODON_MAX_CODONS codons in total.
 *   codon      the codons of all regions are numbered consecutively in the order the regions were given; codon i of a region is the
 *              cells cell0 + 3 i .. cell0 + 3 i + 2.
 *   counters   count[codon][16 b0 + 4 b1 + b2], u32 = the rows that cover all three cells of the codon and have the bases b0, b1, b2
 *              (A C G T = 0 1 2 3) at them in ascending cell order.  A row that covers one or two cells of a codon counts nowhere for
 *              that codon.  The device counts forward-strand triplets only: a gene's strand is the host's business.  A reference
 *              cell that is not ACGT lies under no row: a codon that holds one has 64 zeros.
 *   bk_sample_codons          the row store is bk_link_enable's, there is no enable call of its own.  After the sample's
 *                             bk_sample_finalize (BK_ERR_STATE inside a sample, before any finalize, and when linkage was not
 *                             enabled as the sample began).  BK_ERR_INVALID: a region of no codon, one that ends beyond
 *                             bk_total_cells or crosses a sequence border (the message names the region's index), more than
 *                             BK_CODON_MAX_REGIONS regions or BK_CODON_MAX_CODONS codons (it names the count); nothing is launched.
 *                             n_regions = 0 is valid: an empty table.  Zeroes its buffers and counts (codon_count_kernel,
 *                             codon_finish_kernel); asynchronous on the engine's stream: the regions are staged in pinned memory,
 *                             and the host waits for nothing but an earlier count whose buffers the call replaces.  May be repeated
 *                             with other regions on the same sample.  Independent of bk_sample_linkage: either order, neither
 *                             disturbs the other's results.  Its buffers are made by the first call, grow and never shrink, and are
 *                             freed with the row store; an engine that never calls it allocates and launches nothing; a fork has
 *                             none of its parent's.
 *   bk_sample_download_codons after the sample's finalize; synchronises; the summary (rows = the store's placed rows) and
 *                             min(cap_codons, n_codons) counter rows of 64 in the caller's codon numbering.  counts may be NULL with
 *                             cap_codons 0; both pointers NULL is BK_ERR_INVALID.  Before the sample's first bk_sample_codons there
 *                             are the rows and no codons. */
#define BK_CODON_MAX_REGIONS 4096
#define BK_CODON_MAX_CODONS (1u << 18)
typedef struct { uint32_t cell0, n_codons; } bk_codon_region;
typedef struct { uint64_t rows, n_codons; uint32_t n_regions; } bk_codon_summary;   /* rows = the store's placed rows */
int  bk_sample_codons(bk_engine* e, const bk_codon_region* regions, uint32_t n_regions);
int  bk_sample_download_codons(bk_engine* e, bk_codon_summary* summary, uint32_t* counts /* [n_codons][64] */, uint64_t cap_codons);

/* ---- which haplotypes the reads carry across a region (`bronko call --haplotypes`; additive, still v8) ---------------------------
 * Given an amplicon, an epitope or a drug-resistance stretch: which combinations of substitutions do single reads carry across all of
 * it, and how often?  Pair tables cannot be folded into that answer; the rows of bk_link_enable's store hold it exactly.  A third
 * consumer of that store, and the first whose result size depends on the data: a table of the distinct haplotypes, not a dense
 * counter array.  The terms row, placed, covers and base at a cell are those of bk_link_enable above; rows of both mate files count
 * alike, overlapping mates count twice.  The rule, all of it integer arithmetic:
 *   region     {cell0, len}: the forward-strand cells [cell0, cell0 + len); len is 1..65520; all cells inside one sequence of the
 *              genome file and below bk_total_cells.  At most BK_HAP_MAX_REGIONS regions, in any order; they may overlap, nest and
 *              repeat -- two equal regions are two regions with equal results.
 *   spans      a row spans a region when row.cell0 <= cell0 and cell0 + len <= row.cell0 + row.n.  A row that covers only part of a
 *              region counts nowhere for that region.
 *   haplotype  of a spanning row in a region: the ascending list of (cell - cell0, base) over the row's substitutions whose cell
 *              lies in the region, 0 to 8 entries.  The empty list is the reference haplotype.  Substitutions outside the region do
 *              not belong to it, and neither does the row's strand: two rows that agree inside the region are one haplotype.
 *   results    per region: cover = the spanning rows; ref_count = the spanning rows whose list is empty; one count for each distinct
 *              non-empty list; cover = ref_count + the sum of the counts.  A reference cell that is not ACGT lies under no row: a
 *              region that holds one has cover 0.
 *   entry      bk_hap_entry: the region's index in the caller's order, the count, n_mm and the list in bk_link_row's packing --
 *              mm[3 i ..] = the offset from the region's first cell (16 bits, little endian) and the base (A C G T = 0 1 2 3); the
 *              entries from n_mm on and pad are zero.
 *   bk_sample_haplotypes      the row store is bk_link_enable's, there is no enable call of its own.  After the sample's
 *                             bk_sample_finalize (BK_ERR_STATE inside a sample, before any finalize, and when linkage was not
 *                             enabled as the sample began).  BK_ERR_INVALID: a region with len 0 or above 65520, one that ends beyond
 *                             bk_total_cells or crosses a sequence border (the message names the region's index), more than
 *                             BK_HAP_MAX_REGIONS regions (it names the count), table_log2 outside 10..24; nothing is launched.
 *                             n_regions = 0 is valid: no results.  The distinct non-empty haplotypes of all regions share one
 *                             open-addressing table of 2^table_log2 slots (12 bytes a slot, and room for an entry of 40 bytes per
 *                             slot); it stores no key -- a slot names the first row that claimed it -- and no lane of the kernel waits
 *                             for another.  Zeroes its buffers and counts (hap_count_kernel, hap_finish_kernel); asynchronous on the
 *                             engine's stream: the regions are staged in pinned memory, and the host waits for nothing but an earlier
 *                             count whose buffers the call replaces.  May be repeated on the same sample with other regions or a
 *                             larger table: the rows stay.  Independent of bk_sample_linkage and bk_sample_codons: any order, none
 *                             disturbs another's results.  Its buffers are made by the first call, grow and never shrink, and are
 *                             freed with the row store; an engine that never calls it allocates and launches nothing; a fork has
 *                             none of its parent's.
 *   bk_sample_download_haplotypes  after the sample's finalize; synchronises.  The summary (rows = the store's placed rows, entries =
 *                             the distinct non-empty haplotypes in the table, dropped = the (row, region) that found no slot) and
 *                             cover / ref_count of every region in the caller's order are always exact.  dropped > 0: the summary,
 *                             cover and ref_count are filled, no entry is copied and the call returns BK_ERR_RANGE; the message names
 *                             table_log2 and the count -- call bk_sample_haplotypes again with a larger table.  Otherwise
 *                             min(cap, entries) entries in a defined order: by region, then by list compared as a sequence of
 *                             (offset, base), a proper prefix first (the host sorts: the device's append order is not defined).
 *                             cover, ref_count and entries may be NULL (entries with cap 0); summary may not.  Before the sample's
 *                             first bk_sample_haplotypes there are the rows and no regions. */
#define BK_HAP_MAX_REGIONS 4096
#define BK_HAP_MAX_LEN 65520
typedef struct { uint32_t cell0, len; } bk_hap_region;
typedef struct { uint32_t region, count; uint8_t n_mm, pad[7]; uint8_t mm[24]; } bk_hap_entry;      /* 40 bytes */
typedef struct { uint64_t rows, entries, dropped; uint32_t n_regions, table_log2; } bk_hap_summary;
int  bk_sample_haplotypes(bk_engine* e, const bk_hap_region* regions, uint32_t n_regions, uint32_t table_log2 /* 10..24 */);
int  bk_sample_download_haplotypes(bk_engine* e, bk_hap_summary* summary, uint32_t* cover, uint32_t* ref_count /* [n_regions] each */,
                                   bk_hap_entry* entries, uint64_t cap);

/* ---- the pileup of whole reads: per position, which base the placed reads carry, by strand (`bronko call --read-pileup`; additive,
 * still v8) ---------------------------------------------------------------------------------------------------------------------------
 * The k-mer pileup's depth is approximate; the codon and haplotype tables count placed reads, but only inside their regions.  This is
 * the plain pileup those rest on: how many rows lie over a cell, which base each carries there, on which strand, and how many of them
 * have the cell within a few positions of one of their ends.  A fourth consumer of bk_link_enable's row store.  The terms row, placed
 * and strand are those of bk_link_enable above; rows of both mate files count alike, overlapping mates count twice.  The rule, all
 * of it integer arithmetic:
 *   covers     a row covers the cells [c0, end), c0 = its cell0, end = c0 + n.
 *   base       at a cell c of that range the row's base is its substitution at offset c - c0 if it has one, else the reference's
 *              base at c; bases are in the reference's orientation, as in the rows (A C G T = 0 1 2 3).  Placement guarantees that
 *              the reference's letter under a row is one of ACGT.
 *   near       for the end distance E (0..255) the row is near an end at c when min(c - c0, end - 1 - c) < E.  With n <= 2 E that is
 *              every cell of the row, with E = 0 none.
 *   counters   per cell of the genome file one bk_read_pileup_cell of twelve u32: fwd[b] / rev[b] = the rows of strand 0 / 1 that
 *              cover the cell and carry base b there; near[b] = the rows of either strand that carry b there and are near an end.
 *              A sample has fewer than 2^32 rows: nothing overflows.  A cell whose reference letter is not ACGT has twelve zeros.
 *   summary    rows = the store's placed rows; n_cells; end_dist = E; covered = the cells with at least one row; bases = the sum of
 *              all fwd and rev counters, which equals the sum of the rows' lengths.
 *   bk_sample_read_pileup     the row store is bk_link_enable's, there is no enable call of its own.  After the sample's
 *                             bk_sample_finalize (BK_ERR_STATE inside a sample, before any finalize, and when linkage was not
 *                             enabled as the sample began).  BK_ERR_INVALID: end_dist above 255.  BK_ERR_UNSUPPORTED: an index of
 *                             more than BK_READ_PILEUP_MAX_CELLS cells (the message names both numbers): the work arrays are 15 words
 *                             a cell and the result 12.  Nothing is launched in either case.  A row costs O(1 + n_mm) adds, not n:
 *                             read_pileup_count_kernel adds +1 / -1 to per-strand and near-end difference arrays and 1 per
 *                             substitution, equal destinations of a wave merged into one add; read_pileup_finish_kernel prefix-sums
 *                             the difference arrays over all cells and writes the cells.  Asynchronous on the engine's stream; the
 *                             host waits for nothing but an earlier count whose buffers the call replaces.  May be repeated on the
 *                             same sample with another E.  Independent of bk_sample_linkage, bk_sample_codons and
 *                             bk_sample_haplotypes: any order, none disturbs another's results.  Its buffers are made by the first
 *                             call and are freed with the row store; an engine that never calls it allocates and launches nothing; a
 *                             fork has none of its parent's.
 *   bk_sample_download_read_pileup  after this sample's bk_sample_read_pileup (BK_ERR_STATE before it); synchronises; the summary
 *                             and min(cap_cells, n_cells) cells from cell 0 on.  cells may be NULL with cap_cells 0; summary may
 *                             not. */
#define BK_READ_PILEUP_MAX_CELLS (1u << 22)
#define BK_READ_PILEUP_MAX_END 255
typedef struct { uint32_t fwd[4], rev[4], near[4]; } bk_read_pileup_cell;                          /* 48 bytes */
typedef struct { uint64_t rows, n_cells; uint32_t end_dist, pad; uint64_t covered, bases; } bk_read_pileup_summary;
int  bk_sample_read_pileup(bk_engine* e, uint32_t end_dist /* 0..255 */);
int  bk_sample_download_read_pileup(bk_engine* e, bk_read_pileup_summary* summary, bk_read_pileup_cell* cells, uint64_t cap_cells);

/* ---- pairwise distances of a cohort (`bronko call --distances`; additive, still v8) ----------------------------------------------
 * The consensus letters of many samples of one genome, compared pair by pair on the device.  No part of a sample: the three calls
 * come between samples (BK_ERR_STATE inside one) and touch nothing a sample reads or writes.  The rule, all of it integer arithmetic:
 *   input      n rows of `positions` bytes, row-major: the letters bk_sample_download_consensus returns (under
 *              bk_sample_consensus_indels with '-' at the applied deletions; inserted bases are not among them).
 *   base       a byte is a base iff it is exactly 'A', 'C', 'G' or 'T'.  Every other byte -- N, '-', the IUPAC ambiguity codes, lower
 *              case, anything else -- is not comparable.
 *   compared   compared[i][j] = the positions at which both letters are bases; diff[i][j] = those of them at which the two differ.
 *              Both u32, both symmetric; diff[i][i] = 0, compared[i][i] = the bases of sample i; a pair that shares no base has 0 / 0.
 *   bk_cohort_set        uploads the letters (host memory), packs them into three bit planes per sample (cohort_pack_kernel,
 *                        bk_cohort.hip) and keeps the planes: 24 bytes per 64 positions and sample.  Replaces an earlier cohort, of which
 *                        nothing stays (a call refused for its arguments or its state leaves the earlier cohort as it was; one that
 *                        fails later leaves none).  Synchronises: the letters may go when it returns.  BK_ERR_INVALID,
 *                        with the parameter named: a null pointer, n_samples = 0 or above BK_COHORT_MAX_SAMPLES, positions = 0 or
 *                        >= 2^32.  Per engine: a fork has none of its parent's.  An engine that never calls it allocates and launches
 *                        nothing.
 *   bk_cohort_distances  rows [row0, row0 + n_rows) against all n_samples columns (cohort_pairs_kernel); synchronises and copies
 *                        n_rows x n_samples values, row-major, into each output that is not NULL.  BK_ERR_STATE without a cohort;
 *                        BK_ERR_INVALID for n_rows = 0 and for a block that reaches beyond the cohort.  The device's output buffer grows
 *                        to the largest block asked for: a caller bounds its memory, and the device's, by the block it asks for.
 *   bk_cohort_clear      frees the cohort's device memory; BK_OK also without one. */
#define BK_COHORT_MAX_SAMPLES (1u << 20)
int  bk_cohort_set(bk_engine* e, const uint8_t* letters, uint64_t n_samples, uint64_t positions);
int  bk_cohort_distances(bk_engine* e, uint64_t row0, uint64_t n_rows, uint32_t* diff, uint32_t* compared);
int  bk_cohort_clear(bk_engine* e);

/* ---- the cohort's minimum spanning forest (`bronko call --distances --mst`; additive, still v8) ------------------------------------
 * Who is next to whom: the minimum spanning forest of the cohort bk_cohort_set holds, found on the device by Boruvka rounds over
 * row blocks; nothing of size n^2 leaves the device or is ever held.  The rule, all of it integer arithmetic, over diff[i][j] and
 * compared[i][j] as defined above and one parameter min_compared (u32):
 *   admissible  a pair {i, j}, i < j, is admissible iff compared[i][j] >= 1 and compared[i][j] >= min_compared.  The >= 1 is on
 *               purpose: a pair that shares no base is never "0 apart", even with min_compared = 0.
 *   edge order  edges are ordered by (diff, i, j), lexicographically: a strict total order, there are no ties.
 *   forest      the minimum spanning forest of the admissible graph under that order: the set Kruskal's algorithm keeps when it takes
 *               the admissible edges in ascending order and skips any edge whose ends are already connected.  It is unique, whatever
 *               algorithm finds it.
 *   nearest     nearest[i] is the admissible j != i with the least (diff[i][j], j), or none (sample = 0xffffffff, diff = compared = 0).
 *   rounds      the number of Boruvka rounds in which at least one edge was added: in a round every component picks its least
 *               outgoing admissible edge under the edge order and all picked edges are merged.  Deterministic given the order; at
 *               most ceil(log2 n) + 1.
 *   bk_cohort_mst  between samples only (BK_ERR_STATE inside one); BK_ERR_STATE without a cohort.  Writes the forest's edges, ascending
 *               in the edge order, lo < hi, and their number to *n_edges; nearest (n entries) and rounds where they are not NULL.
 *               BK_ERR_INVALID, with the parameter named: a null edges or n_edges; cap_edges < n - 1 (nothing is written).  n = 1
 *               gives 0 edges and 0 rounds.  Per round and block of rows (sized so that the block's two u32 arrays stay under
 *               256 MB): cohort_pairs_kernel into the cohort's output block, cohort_row_best_kernel over the block where it lies
 *               (per row the least diff << 32 | j over the admissible columns of another component), then two O(n) launches for
 *               every component's least edge; the host merges the O(n) component bests (a union-find) and uploads the new labels.
 *               One synchronise per round.  The cohort stays as it was: bk_cohort_distances afterwards gives the same blocks.
 *               Its buffers (28 bytes per sample) are allocated by the first call and freed with the cohort: an engine that never
 *               calls it allocates and launches nothing. */
typedef struct { uint32_t lo, hi, diff, compared; } bk_mst_edge;        /* lo < hi */
typedef struct { uint32_t sample, diff, compared; } bk_mst_nearest;     /* sample = 0xffffffff: none */
int  bk_cohort_mst(bk_engine* e, uint32_t min_compared, bk_mst_edge* edges, uint64_t cap_edges, uint64_t* n_edges,
                   bk_mst_nearest* nearest /* [n_samples] or NULL */, uint32_t* rounds /* or NULL */);

/* ---- which sample's alleles another carries (`bronko call --distances --contamination`; additive, still v8) -----------------------
 * A sample that holds a share of another one has that one's alleles as minor variants, at exactly the positions where the two
 * consensuses differ.  Over the cohort bk_cohort_set holds and one present mask per sample and position (bk_sample_minor_alleles;
 * only the low four bits of a byte count: A = 1, C = 2, G = 4, T = 8), all of it integer arithmetic.  For sample i and position p:
 *   cons_i(p)     its consensus letter if that is a base (exactly one of ACGT, as above), else none.
 *   minor_i(p)    empty if cons_i(p) is none; otherwise the mask's low four bits without the bit of cons_i(p).
 *   explained     explained[i][j] = the positions p at which cons_i(p) and cons_j(p) are both bases, differ, and the bit of
 *                 cons_j(p) is in minor_i(p).  Row i is the recipient, column j the source.  u32 and NOT symmetric;
 *                 explained[i][i] = 0, explained[i][j] <= diff[i][j].
 *   minor_sites   minor_sites[i] = the positions with minor_i(p) not empty; explained[i][j] <= minor_sites[i].
 *   best          best[i] = the j != i with the largest explained[i][j] >= 1; ties go to the smaller diff[i][j], then to the
 *                 earlier sample; there may be none.
 *   flagged       with two parameters S (u32) and P (double), an ordered pair (i, j), i != j, is flagged iff
 *                 explained[i][j] >= S and (double)explained[i][j] >= P * (double)diff[i][j].
 * best and flagged are the host's (bronko_amd/host/cohort.hpp, ContaminationScanner); the device counts.
 *   bk_cohort_set_minor  after bk_cohort_set, with the same n_samples and positions: uploads the masks (host memory, n rows of
 *                        `positions` bytes, in batches of at most 256 MB) and packs them with the letters' planes that are there
 *                        into four minor planes per sample (cohort_minor_pack_kernel, bk_cohort.hip): M_X = "X is present, the
 *                        sample's consensus is a base, and it is not X"; 32 more bytes per 64 positions and sample, and
 *                        minor_sites (4 bytes per sample), counted in the pack.  Synchronises: the masks may go when it returns.
 *                        A second call replaces the planes of the first.  A later bk_cohort_set or bk_cohort_clear drops them.
 *                        BK_ERR_STATE without a cohort or inside a sample; BK_ERR_INVALID, with the parameter named: a null
 *                        masks, n_samples or positions other than the cohort's.  bk_cohort_distances and bk_cohort_mst give the
 *                        same results before and after it.
 *   bk_cohort_explained  rows [row0, row0 + n_rows) against all n_samples columns (cohort_explained_kernel); synchronises and
 *                        copies n_rows x n_samples values, row-major, into `explained` and n_rows values into `minor_sites`, each
 *                        where it is not NULL (no launch without `explained`).  Blocks and their errors as for
 *                        bk_cohort_distances; BK_ERR_STATE without minor planes.  Its output block is its own: the block of the
 *                        last bk_cohort_distances stays. */
int  bk_cohort_set_minor(bk_engine* e, const uint8_t* masks, uint64_t n_samples, uint64_t positions);
int  bk_cohort_explained(bk_engine* e, uint64_t row0, uint64_t n_rows, uint32_t* explained, uint32_t* minor_sites);

/* ---- build_indexes on the device (optional) -----------------------------------------------------
 * build.rs:145-231 for the metadata sequences given like bk_index_desc gives them: one thread per k-mer writes its k
 * (bucket id, BucketInfo) pairs in generation order, a stable device radix sort groups them by bucket id (inside a bucket the
 * reference's order -- file, sequence, location -- survives), the host cuts the run into buckets.  The result is what
 * bk_index_desc takes: bucket ids ascending, bucket_off[n_buckets + 1], entries.  Arrays are malloc'ed; release them with
 * bk_built_index_free.  Message of a failure: bk_build_last_error(). */
typedef struct {
    uint64_t n_buckets, n_entries;
    uint64_t* bucket_ids;
    uint64_t* bucket_off;
    bk_bucket_info* entries;
} bk_built_index;
int  bk_build_index(int32_t k, int32_t n_files, const int32_t* n_seqs, const uint64_t* seq_lens, const uint8_t* const* seqs,
                    int32_t device, bk_built_index* out);
void bk_built_index_free(bk_built_index* ix);
const char* bk_build_last_error(void);

/* ---- K0: host-side read packer (the step KMC's FASTQ reader performs before counting) ---------------------
 * Splits each ASCII read at every non-ACGT/acgt symbol, drops runs shorter than k, cuts runs longer than
 * 16*stride_words into chunks overlapping by k-1 bases (so every k-mer occurrence is kept exactly once), and
 * writes fixed-stride 2-bit records.  Returns the number of records that the input produces; writes at most
 * `cap_records` of them (call with cap_records = 0 to size the buffers). */
uint64_t bk_pack_reads(const uint8_t* const* reads, const uint64_t* read_lens, uint64_t n_reads, int32_t k,
                       uint32_t stride_words, uint32_t* out_words, uint16_t* out_lens, uint64_t cap_records);
/* Same for reads stored back to back in one buffer: read i = buf[offsets[i] .. offsets[i+1]) */
uint64_t bk_pack_reads_flat(const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads, int32_t k,
                            uint32_t stride_words, uint32_t* out_words, uint16_t* out_lens, uint64_t cap_records);
/* ... and the records' end flags (bk_push_reads_packed_ends), out_ends[cap_records] (may be null) */
uint64_t bk_pack_reads_flat_ends(const uint8_t* buf, const uint64_t* offsets, uint64_t n_reads, int32_t k,
                                 uint32_t stride_words, uint32_t* out_words, uint16_t* out_lens, uint8_t* out_ends, uint64_t cap_records);

/* ---- measurement ------------------------------------------------------------------------------------------
 * When enabled, every kernel launch is bracketed by HIP events on the launch stream.  bk_timing_read
 * synchronises and returns accumulated milliseconds and launch counts since the last reset:
 *   [0] scan_count kernel, [1] finalize kernels, [2] memsets + H2D/D2H copies, [3] level2 + fold kernels.
 * on = 1 brackets all four kinds; on = 2 << kind (or-able) only the selected ones, e.g. 2 = the scan kernel alone
 * (two event records per launch instead of ten per sample).  Bits 8..15 of `on`, when not 0: only every N-th launch of a
 * kind is bracketed -- an event record makes the stream wait for the kernel before it and costs the GPU ~10 us of idle
 * time on that stream (rocprofv3 kernel trace), so a measurement that must not disturb what it measures samples. */
int bk_timing_enable(bk_engine* e, int on);
int bk_timing_read(bk_engine* e, double ms[4], uint64_t n[4], int reset);

#ifdef __cplusplus
}
#endif
#endif
