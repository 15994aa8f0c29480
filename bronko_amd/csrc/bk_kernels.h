// bk_kernels.h -- launch interface between the engine (host) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/bronko_hip.h"
#include "bk_device.h"
#include "bk_link_row.h"

namespace bk {

// The binned scan (bk_scan_items.hip).  scan_items_kernel settles the reads exactly as scan_count_kernel does, but instead of adding
// to a whole-genome difference array in LDS (slabs, fold) and to the V plane with global atomics it EMITS what it would have
// added as 16-bit items, grouped by region of the reference:
//   E item  a run of n <= 255 consecutive cells each seen once more, in the bin of 128 window cells its first cell lies in:
//           bits 0-6 first cell & 127, bits 7-14 n - 1 (never 255: 0xffff is the null item), bit 15 the read runs against the reference
//   V item  +1 / -1 at one counter of the V part of the plane, in the bin of (1 << vq_log2) row positions q it lies in:
//           bits 0-14 offset of the counter from the bin's first, bit 15 = -1
// A workgroup collects its items per bin in LDS buckets (cap_e / cap_v items: what 1/256 of a million reads at the benchmark's
// error rate puts there, and three to four standard deviations) and writes the bucket area out as it is when it ends; a bin that
// outgrows its bucket -- the V rows of a sample's true variants, a coverage spike, every bin of a sample with ten times the
// benchmark's error rate -- continues in its EXTENSION in device memory (gext[wg][bin][kItemGCap]: a plain 2-byte store, the
// slot is the bin's LDS count minus the bucket's capacity).  tab[wg][bin] = items of the bin in that workgroup, bucket and extension
// together.  bin_count_kernel, one workgroup per bin, adds them up in LDS (a 2 x 384-cell difference array or the bin's V rows)
// and adds what is not zero to the plane: no slab, no fold, no same-address global atomic.  An item that finds no room even in the
// extension goes to a device-wide overflow list (bin << 16 | item) every bin's workgroup looks through, and past that list's end
// to the plane directly.  (Until round 4's last build a bin that outgrew its bucket took one of 96 extension buckets in LDS and
// everything else went to the list: with 700 bins overflowing -- 5 % sequencing errors -- the list was a million entries that
// every workgroup of bin_count read through.)
struct ItemGeom {
    uint32_t n_ebins, n_vbins;      // bins [0, n_ebins) are E bins, [n_ebins, n_ebins + n_vbins) V bins; at most 2 * 1024 in all
    uint32_t cap_e, cap_v;          // multiples of 8, <= 64
    uint32_t vq_log2;               // V bin = rows of 1 << vq_log2 positions q: (6 << vq_log2) * (v_span + 1) <= 32767 counters
    uint32_t wg_items;              // = n_ebins * cap_e + n_vbins * cap_v: bucket slots of one workgroup
    uint32_t wg_stride;             // = wg_items: u16 items of one workgroup's bucket area in LDS
    uint32_t grid_max;              // scan workgroups the buffers are laid out for: items[bin][grid_max][cap] -- a bin's buckets of all workgroups are one stretch
                                    // (bin_count reads it front to back) --, tab[bin][grid_max]
};
constexpr uint32_t kEBinLog2 = 7;   // E bins of 128 cells
constexpr uint32_t kERunMax = 255;  // cells one E item covers at most
constexpr uint32_t kEBinSpan = (1u << kEBinLog2) + kERunMax;   // cells an E bin's items reach from its first: 383 (the difference array has one more)
// finalize_vbin_kernel's list of items in LDS (bk_finalize_lean.hip): 16-byte entries.  A region whose 64 reference k-mers are all repeats
// lists 128 E items and as many V items as its reads' errors give it; a sample of the benchmark has 57-76 items over all 467 regions.  4 KB
// of the 14 KB that two workgroups per CU leave at the longest rows; an item that finds it full is settled where it was found.
constexpr uint32_t kLeanListCap = 256;
constexpr uint32_t kItemGCap = 256;   // slots of a (scan workgroup, bin)'s extension in device memory (ScanArgs::gext): what its LDS bucket has no room for

struct ScanArgs {
    const IndexView* ixp;           // device copy of the index view: only the rare paths of scan_count read it
    // what the hot path needs (kept in kernel-argument registers)
    int32_t k, wstart, W, v_omin, v_span;   // v_*: IndexView::v_omin / v_span / v_off
    uint64_t v_off;
    uint32_t total_cells, n_u;
    const uint32_t* ref_words;      // IndexView::ref_words / cell_codes (both with scan_ref_pad_words() words of front padding)
    const uint32_t* cell_codes;
    const uint32_t* cell_has;       // IndexView::cell_has / cell_clean (scan_bit_pad_words() words of front padding)
    const uint32_t* cell_clean;
    const uint32_t* cell_clean3;    // IndexView::cell_clean3 (same padding)
    const uint32_t* cell_yf;        // IndexView::cell_yf / cell_yr (same padding) / id_at
    const uint32_t* cell_yr;
    const uint32_t* id_at;
    const uint32_t* cell_fast;      // IndexView::cell_fast (1 bit per cell, padded like cell_has) / cell_blk (one entry per 64 cells)
    const uint2* cell_blk;
    const uint32_t* cell_nat;       // IndexView::cell_nat (or null)
    const uint32_t* cell_natrow;    // IndexView::cell_natrow (or null)
    const uint2* seed_tab;          // IndexView::seed_tab / seed_log2
    uint32_t seed_log2;
    const uint2* seed_tab2;         // scan_items_kernel: [n_files << seed2_log2] seed tables keyed by the k-mer as a read shows it (bases in reading
    uint32_t seed2_log2;            //   order from bit 0), both strands of every reference k-mer: entry = cell | strand << 27 | tag << 28
    const uint32_t* rc_words;       // ... and the reference reverse-complemented: symbol J = complement of symbol total_cells - 1 - J (paddings of ref_words)
    const uint32_t* words;          // [n_records][stride_words] 2-bit packed, 16 bases per word, LSB first
    const uint16_t* lens;           // [n_records] valid bases
    uint64_t rec_base;              // this launch covers records [rec_base, rec_base + n_records)
    uint64_t n_records;             // upper bound when n_records_dev is set (sizes nothing but the tile loop)
    const unsigned long long* n_records_dev;   // optional: actual record count written by pack_reads_kernel
    uint32_t stride_words;
    unsigned long long* counters;   // u64 plane [E | V] (bk_device.h)
    unsigned int* slabs;            // [grid][n_lds_bins] packed (rc<<16 | fwd) per-cell bins of each workgroup
    // Level 2's work lists, per launch: one bit per k-mer of each record and one bit per record that has any -- all zero between
    // launches (launch_level2 clears what it takes) -- and the diagonal of every marked record.
    //   n_bits / n_any   set by the scan: the k-mers of the N runs it does not settle itself (several mismatches in reach of each
    //                    other, cells that are not "fast", reads off the LDS window or without a diagonal); level2's first pass
    //                    resolves them run by run (S runs, dead pairs) and marks what is left in
    //   l2_bits / l2_any the k-mers that are looked at one by one (level2's second pass).
    unsigned int* n_bits;           // [n_records][l2_words]
    unsigned int* n_any;            // [ceil(n_records / 32)]
    unsigned int* l2_bits;          // [n_records][l2_words]
    unsigned int* l2_any;           // [ceil(n_records / 32)]
    unsigned int* l2_plan;          // null, or one word launch_level2 fills before level2_kernel: how many of its workgroups work
    uint32_t l2_min_grid;           // (l2_plan_kernel: marked records / 256, at least this many) -- with four or more samples in flight
    uint2* l2_diag;                 // [n_records] {cell of the reference k-mer aligned with read k-mer 0, bit 0 same strand | bit 1 known}
    uint32_t l2_words;              // = scan_l2_words(stride_words, k)
    uint32_t n_lds_bins;            // exact hits at cells [win_lo, win_lo + n_lds_bins) are counted in LDS
    uint32_t win_lo;                // first cell of that window (a multiple of 32): the genome the sample looks like
    const uint32_t* win_dev;        // multi-genome index: {win_file, win_lo} chosen on the device per sample (overrides the two fields)
    const uint32_t* occ;            // [n_full][n_files] cell | rc << 31 of the k-mer's first occurrence in each genome file
                                    // (0xffffffff: none), or null; with win_file, seeds land on that genome's copy of a k-mer
    int32_t win_file, n_files;
    int ref_in_lds;                 // stage the packed reference + cell codes in LDS (they fit next to the bins)
    unsigned long long* kmer_total; // optional: += k-mer occurrences scanned
    // full_kmer_stats: k-mers that do not touch the index are counted in this open-addressing table (null = off)
    unsigned long long* ktab_keys;  // [1 << ktab_log2] canonical k-mer | orientation << 63 | mate << 62; ~0 = free
    unsigned int* ktab_cnt;
    uint32_t ktab_log2;
    unsigned long long* ktab_overflow;
    uint32_t mate;
    // Large indexes ("sparse finalize"): whoever adds to a counter also sets the bit of its V row / pseudo row / reference k-mer, so
    // that finalize walks the touched ones instead of a plane of which a thousandth is non-zero, and clears what it read (no
    // plane memset).  Null for small indexes (dense finalize).
    unsigned int* touch_v;          // [v_real_rows / 32 + 1] bit per V row of the reference k-mers
    unsigned int* touch_b;          // [cells / 64 / 32 + 2] scan_count_kernel: bit per block of 64 cells whose rows it counted into (expanded into touch_v)
    unsigned int* touch_p;          // [n_prows / 32 + 1]     bit per pseudo k-mer row (8 counters)
    unsigned int* touch_e;          // [n_u / 32 + 1]         bit per id (its two E counters)
    unsigned long long rl_recip;    // ceil(2^64 / (v_span + 1)): counter index -> row by __umul64hi
    // the binned scan (launch_scan_items): where the items go
    ItemGeom ig;
    unsigned short* items;          // [bin][ig.grid_max][cap_e or cap_v] (E bins first)
    unsigned short* tab;            // [n_bins][ig.grid_max] items of the bin in that workgroup: the first cap_e / cap_v in its bucket, the rest in its extension
    unsigned short* gext;           // [grid][n_bins][kItemGCap] the extensions
    unsigned int* ov;               // [ov_cap] overflow list
    unsigned long long* ov_n;       // [2] entries appended by the launches of even / odd parity (may run past ov_cap: those went to the
    uint32_t ov_cap;                //     plane); bin_count_kernel zeroes the other parity's for the next launch
    uint32_t ov_par;
    int n_direct;                   // the binned scan on one single-sequence genome that fits the window: a read it cannot settle has no usable diagonal
                                    // (none found, or taken away: kMaxChunkMismatches) -- nbatch_kernel would only hand its k-mers on, so the scan
                                    // marks them for level2_kernel itself and nbatch_kernel is not launched
    uint32_t stage_off;             // set by launch_scan_items: byte offset of the waves' record buffers in LDS (0: records are read from memory)
    int ablate;                     // measurement aid (-DBK_TESTING build only): 1 = Level 1 only, 2 = no V atomics, 3 = no slow path
    unsigned long long* dbg;        // -DBK_TESTING build, BK_L2_STATS=1: [32] tallies of what is left to Level 2 and why; null otherwise
};

struct FinalizeArgs {
    IndexView ix;
    const unsigned long long* counters;
    uint64_t elem_lo, elem_hi;      // finalize the counters [elem_lo, elem_hi) of the plane only (a whole number of V rows)
    unsigned long long ci, cs, cx;
    unsigned long long* pileup;     // 4 planes of `plane` u64: fwd depth, rev depth, fwd #kmers, rev #kmers
    size_t plane;                   // total_cells * 4
    unsigned long long* stats;      // [n_files][3]
    unsigned char* present;         // [n_files]
    unsigned long long* kept_total; // optional: += distinct k-mers that passed the thresholds
    unsigned long long* distinct_total; // optional: += distinct k-mers seen at all (non-zero counters)
    unsigned int* partials;         // [finalize_partial_rows()][n_files*3 + 2] per-workgroup tallies, or null: use atomics
    int row_exact, row_general;     // first partials row of K2e / K2b (set by launch_finalize)
    const uint32_t* file_cell_lo;   // [n_files] first cell of each genome file, and the cells of the largest one: pileup_selected_only's
    uint32_t max_file_cells;        // voting pass walks the selected genome's cells (finalize_exact_own_kernel); null / 0 = it does not
    unsigned int* deferred;         // [v_plane_len] V counter indices K2a hands to K2b
    unsigned long long* deferred_n; // ... and their counts (clear_v: K2b cannot read them from the plane any more); may be null
    int clear_v;                    // K2a zeroes every V counter it reads (dense planes, the whole plane in this call, last pass):
                                    // the plane needs no memset before the next sample
    unsigned int* deferred_mask;    // ... pileup_selected_only with file bitmaps: per deferred k-mer, the window positions at which the statistics
                                    // pass found a bucket (what the voting pass probes); may be null
    unsigned int* n_deferred;       // [1], zeroed before each finalize
    // full_kmer_stats: k-mers recorded in V rows that cannot touch the index join the statistics table (null = off)
    unsigned long long* ktab_keys;
    unsigned int* ktab_cnt;
    uint32_t ktab_log2;
    unsigned long long* ktab_overflow;
    uint32_t mate;
    // bk_params.pileup_selected_only: 0 = statistics and votes in one pass; 1 = statistics only (first pass); 2 = votes only, and
    // only for BucketInfos of genome file *sel (second pass, after the genome was selected from the statistics)
    // sparse finalize (see ScanArgs::touch_v): the touched rows / ids, listed by launch_compact_touched; null = walk the plane
    const unsigned int* v_list;     // V rows of the reference k-mers
    const unsigned int* p_list;     // pseudo rows
    const unsigned int* e_list;     // ids
    const unsigned int* n_list;     // their lengths: [0] v_list, [2] reference k-mer ids (front of e_list), [3] pseudo k-mer ids (its tail), [4] p_list
    int mode;
    const int* sel;
    int sel_file;                   // = *sel, read by each kernel of the second pass
    int no_lean;                    // testing aid (BK_NO_LEAN_FINALIZE): the general K2a / K2e even where the regional kernel of bk_finalize_lean.hip applies
    uint32_t lean_list_cap;         // testing aid (-DBK_TESTING build only, BK_LEAN_LIST_CAP): entries of finalize_vbin_kernel's item list, 1 ... kLeanListCap
    unsigned long long* zero_e;     // the plane's E part behind the sample, zero_e[0, zero_e_n), is left zeroed (or null): by launch_finalize's last kernel,
    size_t zero_e_n;                //   or, in the regional finalize, counter by counter by the workgroup that read it
    // The regional finalize fed from the scan's V items (a mate file whose reads were one launch: the V part of its plane is never
    // written).  A V bin of the binned scan is the 64 row positions one finalize_vbin workgroup owns: the workgroup adds the bin's
    // items up in LDS -- what bin_count_kernel does before it stores the bin -- and takes its counts from there.  What Level 2 added
    // to the plane meanwhile is found through f_touch (a bit per V row it wrote: the SPARSE form of level2_kernel); the rows read
    // are zeroed, the bits cleared.  f_items null: the counts are the plane's.
    // Gathered votes (bk_gather.hip; many genomes, sparse planes): mode 1 is the statistics pass as ever, except that
    // finalize_general_kernel notes the deferred k-mers' alias hits; the voting pass (mode 2: the selected genome, mode 3: every
    // genome) is gather_votes_kernel plus, with `gather` set, the general kernels restricted to what it cannot see: votes through
    // alias keys (IndexView::slot_alias) from the pseudo rows, the pseudo k-mers' E counters and the noted hits.
    int gather;
    int gather_ablate;              // measurement aid (-DBK_TESTING build, BK_GATHER_ABLATE): 1 no LDS atomics, 2 no counter loads, 3 no answers either
    unsigned long long* alias_hits; // [alias_cap][3]: canonical k-mer | isrc << 62, count, slot
    unsigned int* n_alias_hits;     // [1], zeroed before the statistics pass
    unsigned int alias_cap;
    const uint64_t* merged_slots;   // [n_merged_slots][2] the window slots of buckets that hold several keys (k = 31: reference buckets whose ids wrapped
    uint32_t n_merged_slots;        //   onto each other): slot | window position << 32, key.  What votes through one key also votes for the other keys' BucketInfos
    const unsigned short* f_items;  // BinArgs::items / tab / gext / ov / ov_n of the launch
    const unsigned short* f_tab;
    const unsigned short* f_gext;
    const unsigned int* f_ov;
    const unsigned long long* f_ov_n;
    uint32_t f_ov_cap, f_ov_par, f_n_wg;
    ItemGeom f_ig;
    unsigned int* f_touch;          // [v_real_rows / 32 + 1]
};

struct FoldArgs {
    const unsigned int* slabs;
    uint32_t n_slabs;               // = grid of the scan launch
    uint32_t n_lds_bins;
    const uint32_t* id_at;          // cell -> id (bins are per cell)
    uint32_t win_lo;                // slab cell i is cell win_lo + i
    const uint32_t* win_dev;        // ... or {win_file, win_lo} chosen on the device
    unsigned int* touch_e;          // sparse finalize: bit per id that received a count (null: dense)
    const uint32_t* cell_codes;     // IndexView::cell_codes + its front padding: symbol 0 = cell 0
    unsigned long long* counters;
};

struct PackArgs {
    const uint8_t* bases;           // sequence lines back to back (16-byte aligned: the caller's pointer rounded down)
    uint32_t shift;                 // ... and by how many bytes: line i starts at bases + shift + offsets[i]
    const unsigned long long* offsets;   // [n_reads + 1]
    uint64_t n_reads;
    int32_t k;
    uint32_t stride_words;
    uint32_t* words;                // out: [cap][stride_words]
    uint16_t* lens;                 // out: [cap]
    uint64_t cap;
    unsigned long long* n_records;  // out (device) [3]: record slots in use (read i's record in slot i, everything else appended behind
                                    // the n_reads slots), records that hold a run, reads on the work list; all set by the launcher
    unsigned long long* n_real;     // the tally of records that hold a run (set by the launcher: its `tally` argument)
    uint32_t* work;                 // [n_reads] scratch: the reads that are not one clean run that fits a record (or null: no word-per-thread kernel)
};
// --min-base-qual: the reads' quality lines, same offsets as the sequence lines (byte i of line r at quals + shift + offsets[r] + i;
// quals 16-byte aligned, like PackArgs::bases); a letter whose quality byte is below thr ('!' + Q) splits the read as an N does
struct QualArgs {
    const uint8_t* quals;
    uint32_t shift;
    uint32_t thr;                   // 34..126
};
// tally: the sample's count of records that hold a run (+= this batch's); q: null, or the quality-aware twins of the packer;
// ends: null, or [cap] out -- the end flags of every record written (the *_ends_kernel variants, launched only with primers set)
void launch_pack_reads(const PackArgs& a, unsigned long long* tally, hipStream_t stream, const QualArgs* q = nullptr, uint8_t* ends = nullptr);

// ---- primer trimming (bk_primers.hip) ----
// A record's end flags: its first base is its read's first letter / its last base is its read's last letter (a chunk of a run
// that was cut into several records carries neither).
constexpr uint32_t kEndFirst = 1u, kEndLast = 2u;
constexpr uint32_t kPrimerMinLen = BK_PRIMER_MIN_LEN, kPrimerMaxLen = BK_PRIMER_MAX_LEN, kMaxPrimers = BK_MAX_PRIMERS, kMaxPrimerMismatches = BK_PRIMER_MAX_MISMATCHES;   // (the limits of include/bronko_hip.h)
// A primer table entry: the primer's 2-bit codes at bases [0, len) of words 0..3, its reverse complement at positions
// [64 - len, 64) of words 4..7 (so that it ends where a window of a record's last 64 bases ends), len in word 8; unused bits 0.
constexpr uint32_t kPrimerEntryWords = 9;
struct TrimArgs {
    uint32_t* words;                // [n_records][stride_words], rewritten in place
    uint16_t* lens;                 // [n_records]
    const uint8_t* ends;            // [n_records] end flags
    uint64_t n_records;
    const unsigned long long* n_records_dev;   // null, or the device's count of record slots in use (K0)
    uint32_t stride_words;
    int32_t k;
    const uint32_t* table;          // [n_primers][kPrimerEntryWords]
    uint32_t n_primers;
    uint32_t max_mismatches;
    unsigned long long* stats;      // [3] += reads trimmed at 5', reads trimmed at 3', bases masked
    unsigned long long* n_real;     // the sample's tally of records that hold a run: -= records left with fewer than k bases
};
void launch_primer_trim(const TrimArgs& a, int n_cus, hipStream_t stream);

// ---- 3' adapter trimming (bk_adapters.hip) ----
// (the limits of include/bronko_hip.h)
constexpr uint32_t kAdapterMinLen = BK_ADAPTER_MIN_LEN, kAdapterMaxLen = BK_ADAPTER_MAX_LEN, kMaxAdapters = BK_MAX_ADAPTERS,
                   kAdapterMinOverlap = BK_ADAPTER_MIN_OVERLAP;
constexpr double kAdapterMaxErrorRate = BK_ADAPTER_MAX_ERROR_RATE;
static_assert(kAdapterMaxLen == 64 && kMaxAdapters <= 8, "AdapterEntry holds 64 bases, AdapterArgs eight entries");
constexpr uint32_t kNoCut = 0xFFFFFFFFu;   // cut[r]: no adapter found in record r
// The adapter table travels as kernel arguments (it is the same for every lane: scalar registers, no LDS, no table in memory).
struct AdapterEntry {
    uint32_t code[4];               // the adapter's 2-bit codes at bases [0, len); unused bits 0
    uint32_t mask[4];               // the even bits of bases [0, len)
    uint32_t len;                   // 8..64
    uint32_t allowed;               // floor(E * len): mismatches the whole adapter may have
};
struct AdapterArgs {
    uint32_t* words;                // [n_records][stride_words], cut in place
    uint16_t* lens;                 // [n_records]
    const uint8_t* ends;            // [n_records] end flags: only records with kEndLast are searched
    uint32_t* cut;                  // [n_records] scratch, kNoCut everywhere before and after: the leftmost match of each record
    uint64_t n_records;
    const unsigned long long* n_records_dev;   // null, or the device's count of record slots in use (K0)
    uint32_t stride_words;
    int32_t k;
    uint32_t n_adapters;
    uint32_t min_overlap;
    // floor(E * l) for l = 1..64, as the host computed it in double: it starts at 0 and grows by 0 or 1 a step (E < 1), so it
    // is held as its steps -- bit l - 1 set where allowed[l] = allowed[l - 1] + 1 -- and allowed[l] = popcount of the low l bits
    uint64_t allowed_steps;
    unsigned long long* stats;      // [2] += reads cut, bases removed
    unsigned long long* n_real;     // the sample's tally of records that hold a run: -= records left with fewer than k bases
    AdapterEntry adapters[kMaxAdapters];
};
void launch_adapter_trim(const AdapterArgs& a, int n_cus, hipStream_t stream);
// votes[f] += number of the first records' middle k-mers that occur in genome file f (which genome does the sample look like?)
void launch_pick_window(const ScanArgs& a, uint64_t n_probe, unsigned int* votes, const uint32_t* file_cell_lo, int forced, uint32_t* win,
                        hipStream_t stream);
void launch_count_kmers(const ScanArgs& a, hipStream_t stream);   // empty window: kmer_total += k-mer occurrences, nothing else
void launch_add_u64(unsigned long long* dst, const unsigned long long* src, hipStream_t stream);   // *dst += *src
void launch_add_const_u64(unsigned long long* dst, unsigned long long v, hipStream_t stream);        // *dst += v
uint32_t scan_grid(uint64_t n_records, int n_cus);
uint32_t scan_l2_words(uint32_t stride_words, int k);   // bitmap words per record (ScanArgs::l2_words)
uint64_t scan_max_records(uint32_t grid);   // most records one launch_scan_count may be given
int scan_ref_pad_words();
int scan_ref_back_words();
int scan_bit_pad_words();
int scan_bit_back_words();
size_t scan_lds_budget();   // bytes available for histogram bins (4 B each) + the staged reference
size_t scan_ref_lds_bytes(uint32_t total_cells);
size_t scan_lds_bytes(uint32_t n_lds_bins, bool ref_in_lds, uint32_t total_cells);
hipError_t launch_scan_count(const ScanArgs& a, uint32_t grid, hipStream_t stream);
void launch_fold(const FoldArgs& f, hipStream_t stream);
// ---- the binned scan (bk_scan_items.hip) ----
struct BinArgs {
    ItemGeom ig;
    const unsigned short* items;    // as ScanArgs
    const unsigned short* tab;
    const unsigned short* gext;
    uint32_t n_wg;                  // grid of the scan_items launch
    const unsigned int* ov;
    unsigned long long* ov_n;
    uint32_t ov_cap, ov_par;
    const uint32_t* id_at;          // cell -> id
    const uint32_t* cell_codes;     // IndexView::cell_codes past its front padding: symbol 0 = cell 0
    uint32_t win_lo;                // window cell i is cell win_lo + i
    const uint32_t* win_dev;        // ... or {win_file, win_lo} chosen on the device
    uint32_t total_cells;
    unsigned long long* counters;   // the plane
    uint64_t v_off, v_real_len;     // its V part (the reference k-mers' rows)
    uint32_t rl;                    // v_span + 1
    int v_mode;                     // how a V bin reaches the plane: 0 atomics, 1 plain read-modify-write, 2 plain stores (the V part is all zero)
    int part;                       // 0: every bin; 1: the E bins only (the V bins' items wait for the regional finalize, FinalizeArgs::f_items, or
                                    // for a launch with part = 2); 2: the V bins only (also: the E bins ride in the Level 2 launch, launch_level2)
    int ablate;                     // measurement aid (-DBK_TESTING build only): 1 no items read, 2 nothing written to the plane, 3 no E atomics, 4 no V writes
};
// can this index take the binned scan (window of win_cells cells in LDS, dense planes)?  Fills g.
bool item_geometry(uint32_t win_cells, uint32_t n_full, int v_span, ItemGeom* g);
uint32_t items_grid(uint64_t n_records, int n_cus);
uint32_t items_max_grid(int n_cus);
size_t items_lds_bytes(const ItemGeom& g, uint32_t win_cells);
hipError_t launch_scan_items(const ScanArgs& a, uint32_t grid, hipStream_t stream);
hipError_t launch_bin_count(const BinArgs& b, hipStream_t stream);
// Level 2, after launch_scan_count / launch_scan_items with the same arguments.  ride: null, or the BinArgs of the launch_scan_items
// it follows -- that launch's E bins are then counted by extra workgroups of level2_kernel's launch (both only add to the plane
// with atomics and read only what the scan wrote), and launch_bin_count is wanted for its V bins at most (part = 2, in front of this).
// zero: null, or what further workgroups of that launch zero (the engine's zero ride: a sample's outputs, which nothing reads or
// writes before its finalize, and the kstats set of the next sample) -- what launch_zero_small would have been given.
struct ZeroRide {
    unsigned long long* big; uint64_t n_big;      // 16-byte stores, shared by the ride's workgroups (the pileup arrays)
    unsigned long long* a; unsigned long long* b; // the small buffers: the ride's first workgroup
    unsigned char* c; unsigned int* d;
    uint32_t n_a, n_b, n_c, n_d;
    uint32_t first, n_wg;                         // (launch_level2 fills these) the ride's first workgroup in the grid, and how many
};
inline bool level2_launches(const ScanArgs& a) { return a.n_records != 0 && a.W > 0; }   // else launch_level2 launches nothing: no ride
hipError_t launch_level2(const ScanArgs& a, int n_cus, hipStream_t stream, const BinArgs* ride = nullptr, const ZeroRide* zero = nullptr);
void launch_ktab_stats(const unsigned long long* keys, const unsigned int* cnt, uint32_t log2n, unsigned long long ci,
                       unsigned long long cx, unsigned long long* out, hipStream_t stream);
void launch_ktab_rehash(const unsigned long long* okeys, const unsigned int* ocnt, uint32_t olog2, unsigned long long* nkeys, unsigned int* ncnt,
                        uint32_t nlog2, unsigned long long* overflow, hipStream_t stream);
void launch_ktab_count_parts(const unsigned long long* keys, uint32_t log2n, uint32_t n_parts, unsigned long long* counts, hipStream_t stream);
void launch_ktab_scatter_parts(const unsigned long long* keys, const unsigned int* cnt, uint32_t log2n, uint32_t n_parts, unsigned long long* cursors,
                               unsigned long long* out_keys, unsigned int* out_cnt, hipStream_t stream);
void launch_ktab_import(const unsigned long long* in_keys, const unsigned int* in_cnt, uint64_t n, unsigned long long* keys, unsigned int* cnt, uint32_t log2n,
                        unsigned long long* overflow, hipStream_t stream);
void launch_ktab_totals_to_kstats(unsigned long long* ktab_out, unsigned long long* kstats, int n_mates, hipStream_t stream);
uint32_t ktab_fill_words();   // tallies of new keys behind the overflow word: ktab_out[8 ..]
// What the kernels that ride behind a scan take of its batch and of the index (the k-mer dump, bk_indels.hip, bk_linkage.hip).
// A batch of records (Records of bk_engine.h); n_records_dev: null, or the ASCII paths' record count, known on the device only
struct RecordsView {
    const uint32_t* words; const uint16_t* lens;
    uint64_t n_records; const unsigned long long* n_records_dev;
    uint32_t stride_words;
};
// Placing a record by two anchor k-mers (bk_anchor.h): the perfect hash of the reference k-mers, one bit per id (it starts at exactly
// one cell), both references past their padding, and the genome file's geometry -- the engine's AnchorTables hold unique_bits, seq_lo
// and nruns
struct AnchorIndex {
    const KmerPos* kmer_pos; const uint16_t* pilots;
    uint32_t m, log2nb, log2p, n_full;
    const uint32_t* unique_bits;
    const uint32_t* ref_words; const uint32_t* rc_words;
    uint32_t total_cells; int32_t k;
    const uint32_t* seq_lo;              // [n_seqs + 1] first cell of each sequence, then total_cells
    uint32_t n_seqs;
    const uint2* nruns;                  // [n_nruns] {first cell, end} of the runs of letters that are not ACGT, ascending
    uint32_t n_nruns;
};
// the sample's k-mer count table (bk_kmer_dump.hip; bk_kmer_dump_enable): count every k-mer of a batch of records (n_records_dev: the
// ASCII paths' record count, known on the device only); per mate file, select ci <= count <= cx as (k-mer, min(count, cs)) into
// out_* (at most cap; res[0] = kept, res[1] = distinct); sort the pairs by k-mer (rocprim; tmp == nullptr: tmp_bytes is sized)
void launch_kmer_dump_count(const RecordsView& rec, int k, uint32_t mate, unsigned long long* keys, unsigned int* cnt, uint32_t log2n,
                            unsigned long long* overflow, int n_cus, hipStream_t stream);
void launch_kmer_dump_select(const unsigned long long* keys, const unsigned int* cnt, uint32_t log2n, uint32_t mate, unsigned long long ci,
                             unsigned long long cs, unsigned long long cx, unsigned long long* out_keys, unsigned int* out_cnt, uint64_t cap,
                             unsigned long long* res, hipStream_t stream);
hipError_t kmer_dump_sort(void* tmp, size_t& tmp_bytes, unsigned long long* keys_in, unsigned long long* keys_out, unsigned int* vals_in,
                          unsigned int* vals_out, uint64_t n, int k, hipStream_t stream);
void launch_finalize(const FinalizeArgs& a, hipStream_t stream);
// K2a / K2e organised by region of the reference (bk_finalize_lean.hip): one genome file, dense planes, one pass
bool finalize_lean_ok(const FinalizeArgs& a);
unsigned launch_finalize_lean_variant(const FinalizeArgs& a, hipStream_t stream);   // returns its grid (rows of FinalizeArgs::partials it writes)
// sparse finalize: touch bitmaps -> lists (the bitmaps are cleared on the way); lists -> their counters zeroed again
void launch_expand_touched_blocks(unsigned int* touch_b, uint32_t n_blocks, const uint2* cell_blk, unsigned int* touch_v, uint32_t span, uint64_t n_q, hipStream_t stream);
void launch_compact_touched(unsigned int* touch_v, uint64_t n_rows, unsigned int* touch_p, uint64_t n_prows, unsigned int* touch_e, uint64_t n_ids,
                            uint64_t n_full, unsigned int* v_list, unsigned int* p_list, unsigned int* e_list, unsigned int* n_list, hipStream_t stream);
void launch_clear_touched(unsigned long long* counters, uint64_t v_off, uint64_t v_real_len, uint32_t rl, const unsigned int* v_list,
                          const unsigned int* p_list, const unsigned int* e_list, const unsigned int* n_list, uint64_t n_ids, hipStream_t stream);
// one launch zeroes what a sample starts from: the engine's small per-sample buffers and the pileup arrays (`big`)
void launch_zero_small(unsigned long long* a, size_t na, unsigned long long* b, size_t nb, unsigned long long* c, size_t nc,
                       unsigned char* d, size_t nd, unsigned int* e, size_t ne, unsigned long long* big, size_t nbig, hipStream_t stream);
// shard_sums <-> {stats, present, kstats}: the small additive results of a sharded finalize as one u64 vector
void launch_pack_sums(unsigned long long* sums, const unsigned long long* stats, const unsigned char* present, const unsigned long long* kstats,
                      int n_files, unsigned long long* xflag, hipStream_t stream);
void launch_unpack_sums(const unsigned long long* sums, unsigned long long* stats, unsigned char* present, unsigned long long* kstats,
                        int n_files, unsigned long long* xflag, hipStream_t stream);
// sharded finalize: a counter plane packed for the reduce-scatter (16- or 32-bit elements, n_parts parts) and a received part
// widened again; xflag[0] is raised when an element does not fit (bk_kernels.hip, xport_pack_kernel)
uint64_t xport_part_bytes(uint64_t plane_len, uint64_t v_off, uint32_t n_parts, int width);
void launch_xport_measure(const unsigned long long* plane, uint64_t plane_len, uint64_t v_off, unsigned long long* out, hipStream_t stream);
void launch_xport_pack(const unsigned long long* plane, uint64_t plane_len, uint64_t v_off, uint32_t n_parts, int width, void* buf, unsigned long long* flag,
                       hipStream_t stream);
void launch_xport_unpack(const void* recv, uint64_t plane_len, uint64_t v_off, uint32_t n_parts, uint32_t shard, int width, unsigned long long* reduced,
                         hipStream_t stream);
// ---- after the pileup (bk_caller.hip) ----
typedef bk_call_params CallParamsDev;
typedef bk_call_record CallRecordDev;
typedef bk_call_summary CallSummaryDev;
struct CallArgs {
    CallParamsDev prm;
    int32_t n_files, n_mates;
    const unsigned long long* stats;     // [n_mates][n_files][3]
    const unsigned char* present;        // [n_mates][n_files]
    const uint64_t* genome_len;          // [n_files] sum of the file's sequence lengths
    const int32_t* seq_first;            // [n_files] index of the file's first sequence
    const int32_t* n_seqs;               // [n_files]
    const uint64_t* seq_cell;            // [sequences] first cell
    const uint64_t* seq_len;             // [sequences]
    const uint32_t* ref_words;           // IndexView::ref_words past its front padding: symbol 0 = cell 0
    const unsigned long long* pileup;    // 4 planes of `plane` u64
    size_t plane;
    double* noise;                       // [total_cells] Noise.max per position
    // get_baseline_noise with its two chains apart (bk_caller.hip): scratch of the selected genome -- [cells][3] sorted minor-allele
    // frequencies, [cells][10] the table / [cells][2] s, s2 / [cells] n after each position's step; null: the walk in one wave
    double* noise_maf;
    double* noise_tbl;                   // [cells + 64 sequences][10]: per sequence the list of the table's states (state 0: empty; one more per step that changed it)
    unsigned int* noise_state;           // [cells] the state after each position's step
    double* noise_sums;
    unsigned int* noise_cnt;
    int noise_serial;                    // testing aid (BK_NOISE_SERIAL): the serial kernel for every sequence
    CallRecordDev* records;
    uint64_t record_cap;
    CallSummaryDev* out;
};
void launch_call(const CallArgs& a, int max_seqs_per_file, uint64_t max_file_cells, hipStream_t stream);
void launch_select_genome(const CallArgs& a, hipStream_t stream);   // the first kernel of launch_call alone: a.out->file_id
// bk_sample_consensus: one letter per position of the genome bk_sample_call selected (consensus_kernel, bk_caller.hip)
typedef bk_consensus_params ConsensusParamsDev;
typedef bk_consensus_summary ConsensusSummaryDev;
struct ConsensusArgs {
    ConsensusParamsDev prm;
    const int32_t* seq_first;            // the geometry CallArgs has
    const int32_t* n_seqs;
    const uint64_t* seq_cell;
    const uint64_t* seq_len;
    const uint32_t* ref_words;
    const unsigned long long* pileup;    // the two depth planes are read
    size_t plane;
    const CallSummaryDev* out;           // bk_sample_call's: file_id
    uint8_t* letters;                    // [cells of the selected genome] in (sequence, position) order
    ConsensusSummaryDev* summary;        // tallies zeroed by the caller; the kernel writes file_id and adds
};
void launch_consensus(const ConsensusArgs& a, uint64_t max_file_cells, hipStream_t stream);
// bk_sample_minor_alleles: the present mask of every position of the genome bk_sample_call selected (minor_alleles_kernel, bk_caller.hip)
typedef bk_minor_params MinorParamsDev;
typedef bk_minor_summary MinorSummaryDev;
struct MinorArgs {
    MinorParamsDev prm;
    const int32_t* seq_first;            // the geometry CallArgs has
    const int32_t* n_seqs;
    const uint64_t* seq_cell;
    const uint64_t* seq_len;
    const unsigned long long* pileup;    // the two depth planes are read
    size_t plane;
    const CallSummaryDev* out;           // bk_sample_call's: file_id
    uint8_t* masks;                      // [cells of the selected genome] in (sequence, position) order
    MinorSummaryDev* summary;            // tallies zeroed by the caller; the kernel writes file_id and adds
};
void launch_minor_alleles(const MinorArgs& a, uint64_t max_file_cells, hipStream_t stream);
// bk_sample_region_depths: the depth numbers of every region of the genome bk_sample_call selected (region_depth_kernel, bk_regions.hip)
typedef bk_region_depth RegionDepthDev;
typedef bk_region_summary RegionSummaryDev;
struct RegionArgs {
    uint64_t min_depth;                  // covered: depth >= min_depth
    const uint2* table;                  // [regions] {first cell, L}, grouped by genome file (bk_regions_set resolved and checked them)
    const uint32_t* file_off;            // [n_files + 1] the file's slice of `table`
    const unsigned long long* pileup;    // the two depth planes are read
    size_t plane;
    const CallSummaryDev* out;           // bk_sample_call's: file_id
    RegionDepthDev* rows;                // [regions of the file with the most] row b: region b of the selected file's slice
    RegionSummaryDev* summary;           // zeroed by the caller; the kernel writes file_id and n_regions and adds the tallies
};
constexpr uint32_t kRegionLdsDepths = 2048;   // a region of at most this many positions is staged in LDS once (16 KB)
void launch_region_depths(const RegionArgs& a, uint32_t max_file_regions, hipStream_t stream);
// The event passes (bk_event_pass.h): what the six passes below are given alike.  `tallies` holds the pass's kScanTallies scan
// tallies, then candidates, reported, overflow (Args::kCandidates, kReported, kOverflow; kTallies words in all).  The members a scan
// kernel reads lie in the order its arguments have always had: these kernels sit at the SGPR limit, and another order of the
// argument block is another register allocation (profiles/README.md, the event pass).  So the word in front of max_mismatches is
// the pass's length limit under the pass's own name -- the indels' max_len, the junctions' and duplications' min_len, the
// breakends' min_clip; copy-backs and chimeras have none and leave it zero.  For the same reason what a pass adds to the sample's
// arrays (`more`: the breakends' site array; an empty struct, which lies in log2n's padding, for the others) keeps its place in
// front of span.
struct NoSampleArrays {};
template <class SampleArrays = NoSampleArrays>
struct EventPassArgsOf {
    RecordsView rec;                     // x_scan_kernel's batch
    AnchorIndex ix;
    union { uint32_t max_len, min_len, min_clip; };
    uint32_t max_mismatches;
    // the sample: event table (one key word, ~0 = free; two counters a slot), span, counters
    unsigned long long* keys;
    unsigned int* counts;                // [slots][2]
    uint32_t log2n;
    SampleArrays more;
    unsigned int* span;                  // [total_cells + 2]
    unsigned long long* tallies;         // [kTallies]
    // the report: x_report_kernel
    uint64_t min_reads, row_cap;
};
typedef EventPassArgsOf<> EventPassArgs;
struct BreakendSite { unsigned int* site; };   // [total_cells][2] L, R: the supporting reads of every (cell, side)
typedef EventPassArgsOf<BreakendSite> BreakendPassArgs;
// (the order above, held: the limit's word directly in front of max_mismatches, span behind log2n's word, behind `site` where there is one)
static_assert(offsetof(EventPassArgs, max_mismatches) == offsetof(EventPassArgs, min_len) + 4 && offsetof(EventPassArgs, keys) == offsetof(EventPassArgs, min_len) + 8 &&
              offsetof(EventPassArgs, span) == offsetof(EventPassArgs, log2n) + 8 && offsetof(EventPassArgs, tallies) == offsetof(EventPassArgs, log2n) + 16,
              "EventPassArgs: the scan kernels' argument order");
static_assert(offsetof(BreakendPassArgs, more) == offsetof(BreakendPassArgs, log2n) + 8 && offsetof(BreakendPassArgs, span) == offsetof(BreakendPassArgs, log2n) + 16,
              "BreakendArgs: site in front of span");
void launch_span_prefix(unsigned int* span, uint32_t n, hipStream_t stream);   // span[0 .. n) in place, once per sample (bk_event_pass.hip)
// bk_indels_enable: short insertions and deletions from the reads (bk_indels.hip; the rule: include/bronko_hip.h)
typedef bk_indel_record IndelRecordDev;
struct IndelArgs : EventPassArgs {       // (`keys` is not used: the table's key is two words, {fwd, rev})
    enum { kScanTallies = 5, kCandidates = 5, kReported, kOverflow, kTallies };   // records, anchored, ref_spanning, supporting, discordant
    uint32_t min_af_ppm;
    unsigned long long* key0; unsigned long long* key1;
    IndelRecordDev* rows;
};
void launch_indel_scan(const IndelArgs& a, int n_cus, hipStream_t stream);
void launch_indel_report(const IndelArgs& a, hipStream_t stream);
// bk_sample_consensus_indels: the sample's indel events applied to its consensus letters (bk_consensus_indels.hip; the rule:
// include/bronko_hip.h, DESIGN.md section CI).  Three passes over the indels' table, which none of them writes
typedef bk_consensus_indel_record ConsensusIndelRecordDev;
typedef bk_consensus_indel_summary ConsensusIndelSummaryDev;
struct ConsensusIndelArgs {
    ConsensusParamsDev prm;              // of the sample's last bk_sample_consensus
    const unsigned long long* key0;      // the indels' event table (IndelArgs)
    const unsigned long long* key1;
    const unsigned int* counts;
    uint32_t log2n;
    uint32_t total_cells;
    const unsigned int* span;            // prefix-summed (bk_sample_indels)
    const unsigned long long* table_overflow;   // the indels' overflow tally: a full table makes this result an error too
    const CallSummaryDev* out;           // bk_sample_call's: file_id
    const int32_t* seq_first;            // where the selected genome's letters begin (ConsensusArgs)
    const uint64_t* seq_cell;
    unsigned int* best;                  // [total_cells + 1] per boundary: the largest s of an accepted event; zeroed by the caller
    unsigned int* ties;                  // [total_cells + 1] ... and how many accepted events have it; zeroed by the caller
    uint8_t* letters;                    // the consensus letters (ConsensusArgs::letters): '-' is stored at the applied deletions
    uint64_t n_letters;                  // the room of `letters`
    ConsensusIndelRecordDev* rows;       // [BK_CONSENSUS_INDEL_MAX] the accepted events, in no order
    ConsensusIndelSummaryDev* summary;   // zeroed by the caller; the last pass writes file_id and adds the tallies
};
void launch_consensus_indels(const ConsensusIndelArgs& a, hipStream_t stream);
// bk_junctions_enable: long deletions and subgenomic-RNA junctions from the reads (bk_junctions.hip; the rule: include/bronko_hip.h,
// DESIGN.md section J)
typedef bk_junction_record JunctionRecordDev;
struct JunctionArgs : EventPassArgs {    // key pos | D << 32, {fwd, rev}
    enum { kScanTallies = 7, kCandidates = 7, kReported, kOverflow, kTallies };   // records, anchored, ref_spanning, supporting, short, backward, discordant
    JunctionRecordDev* rows;
};
void launch_junction_scan(const JunctionArgs& a, int n_cus, hipStream_t stream);
void launch_junction_report(const JunctionArgs& a, hipStream_t stream);
// bk_copybacks_enable: strand-switch (copy-back, snap-back) junctions from the reads (bk_copybacks.hip; the rule: include/bronko_hip.h,
// DESIGN.md section B)
typedef bk_copyback_record CopybackRecordDev;
struct CopybackArgs : EventPassArgs {    // key lo | kind << 31 | hi << 32, {lo_first, hi_first}
    enum { kScanTallies = 6, kCandidates = 6, kReported, kOverflow, kTallies };   // records, same_strand, ref_spanning, switched, supporting, discordant
    uint32_t min_dist;
    CopybackRecordDev* rows;
};
void launch_copyback_scan(const CopybackArgs& a, int n_cus, hipStream_t stream);
void launch_copyback_report(const CopybackArgs& a, hipStream_t stream);
// bk_chimeras_enable: junctions between two sequences of the genome file from the reads (bk_chimeras.hip; the rule: include/bronko_hip.h,
// DESIGN.md section X)
typedef bk_chimera_record ChimeraRecordDev;
struct ChimeraArgs : EventPassArgs {     // key lo | sides << 28 | hi << 32, {lo_first, hi_first}
    enum { kScanTallies = 6, kCandidates = 6, kReported, kOverflow, kTallies };   // records, same_strand, ref_spanning, crossed, supporting, discordant
    ChimeraRecordDev* rows;
};
void launch_chimera_scan(const ChimeraArgs& a, int n_cus, hipStream_t stream);
void launch_chimera_report(const ChimeraArgs& a, hipStream_t stream);
// bk_breakends_enable: reads that leave the reference -- records with an anchor at one end only (bk_breakends.hip; the rule:
// include/bronko_hip.h)
typedef bk_breakend_record BreakendRecordDev;
struct BreakendArgs : BreakendPassArgs {    // key cell | side << 27 | tag << 32, {fwd, rev}
    enum { kScanTallies = 8, kCandidates = 8, kReported, kOverflow, kTallies };   // records, one_anchor, ref_spanning, supporting, short, through, discordant, unplaced
    BreakendRecordDev* rows;
};
void launch_breakend_scan(const BreakendArgs& a, int n_cus, hipStream_t stream);
void launch_breakend_report(const BreakendArgs& a, hipStream_t stream);
// bk_duplications_enable: tandem duplications and circular-origin reads (bk_duplications.hip; the rule: include/bronko_hip.h,
// DESIGN.md section V)
typedef bk_duplication_record DuplicationRecordDev;
struct DuplicationArgs : EventPassArgs { // key pos | E << 32, {fwd, rev}
    enum { kScanTallies = 7, kCandidates = 7, kReported, kOverflow, kTallies };   // records, anchored, ref_spanning, supporting, short, forward, discordant
    DuplicationRecordDev* rows;
};
void launch_duplication_scan(const DuplicationArgs& a, int n_cus, hipStream_t stream);
void launch_duplication_report(const DuplicationArgs& a, hipStream_t stream);
// bk_link_enable: which substitutions the same records carry (bk_linkage.hip; the rule: include/bronko_hip.h)
struct LinkArgs {
    RecordsView rec;                     // link_scan_kernel's batch
    AnchorIndex ix;
    uint32_t max_mismatches;
    // the sample: its row store (bk_link_row.h) and tallies
    RowStoreView store;
    unsigned long long* tallies;         // [4] records, placed (= the rows in the store: store.placed), unplaced, discordant
    // the count: link_count_kernel
    const uint32_t* sites;               // [n_sites] cells, strictly ascending
    const uint32_t* pair_lo;             // [n_sites] index of the pair (i, i + 1); the pair (i, j) is pair_lo[i] + (j - i - 1)
    uint32_t n_sites, max_dist;
    uint64_t n_pairs;
    unsigned int* counts;                // [n_pairs][16] the record's base at A x its base at B
};
constexpr uint32_t kLinkLdsPairs = 512;  // a counter table of at most this many pairs is privatised in LDS (32 KiB a workgroup)
void launch_link_scan(const LinkArgs& a, int n_cus, hipStream_t stream);
void launch_link_count(const LinkArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream);   // rows_upper: a bound on the rows (the grid)
// bk_sample_codons: how many rows of bk_link_enable's store carry each of the 64 triplets at every codon of the caller's coding regions
// (bk_codons.hip; the rule: include/bronko_hip.h)
struct CodonArgs {
    const uint32_t* ref_words;           // AnchorIndex's
    uint32_t total_cells;
    RowStoreView store;                  // the sample's row store: LinkArgs'
    const uint4* sorted;                 // [n_regions] by first cell: {cell0, n_codons, index of its first codon, max end cell of the regions up to here}
    const uint2* regions;                // [n_regions] the caller's order: {cell0, index of its first codon}
    uint32_t n_regions, n_codons;
    unsigned int* cover_diff;            // [n_codons + 1] +1 at a row's first wholly covered codon of a region, -1 one behind its last
    unsigned int* counts;                // [n_codons][64] the caller's codon numbering; triplet 16 b0 + 4 b1 + b2
};
constexpr uint32_t kCodonLdsCodons = 16384;   // a cover_diff of at most this many entries is privatised in LDS (64 KiB a workgroup)
void launch_codon_count(const CodonArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream);   // rows_upper: a bound on the rows (the grid)
void launch_codon_finish(const CodonArgs& a, hipStream_t stream);
// bk_sample_haplotypes: which lists of substitutions the rows of bk_link_enable's store carry across each of the caller's regions
// (bk_haplotypes.hip; the rule: include/bronko_hip.h)
typedef bk_hap_entry HapEntryDev;
struct HapArgs {
    RowStoreView store;                  // the sample's row store: LinkArgs'
    const uint2* sorted;                 // [n_regions] by first cell: {cell0, len | the caller's index << 16}
    const uint2* regions;                // [n_regions] the caller's order: {cell0, len}
    uint32_t n_regions, table_log2;
    unsigned int* hot;                   // [n_regions][2] cover, ref_count
    unsigned long long* owner;           // [2^table_log2] 0 = free, else ((row << 12) | region) + 1 of the row that claimed the slot
    unsigned int* count;                 // [2^table_log2]
    unsigned long long* tallies;         // [2] entries (hap_finish_kernel), dropped (hap_count_kernel)
    HapEntryDev* entries; uint64_t entry_cap;
};
void launch_hap_count(const HapArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream);   // rows_upper: a bound on the rows (the grid)
void launch_hap_finish(const HapArgs& a, hipStream_t stream);
// bk_sample_read_pileup: per cell, the rows of bk_link_enable's store that cover it by the base they carry there, by strand and near
// their ends (bk_read_pileup.hip; the rule: include/bronko_hip.h)
typedef bk_read_pileup_cell ReadPileupCellDev;
struct ReadPileupArgs {
    const uint32_t* ref_words;           // AnchorIndex's
    uint32_t total_cells;
    uint32_t end_dist;                   // E: 0..255
    RowStoreView store;                  // the sample's row store: LinkArgs'
    unsigned int* diff;                  // [3][total_cells + 1] difference arrays: cover of strand 0, of strand 1, near-end cover
    unsigned int* mm;                    // [total_cells][4][2] substitutions by cell, base, strand
    unsigned int* mm_near;               // [total_cells][4] ... of them the ones near an end of their row
    ReadPileupCellDev* cells;            // [total_cells] the result
    unsigned long long* tallies;         // [2] covered, bases (read_pileup_finish_kernel writes both)
};
void launch_read_pileup_count(const ReadPileupArgs& a, uint64_t rows_upper, int n_cus, hipStream_t stream);   // rows_upper: a bound on the rows (the grid)
void launch_read_pileup_finish(const ReadPileupArgs& a, hipStream_t stream);
size_t finalize_lds_bytes(int n_files);
size_t finalize_partial_rows();
void launch_prefix_rows(unsigned long long* counters, const IndexView& ix, const unsigned int* v_list, const unsigned int* n_list, unsigned int* row_bits, hipStream_t stream);   // bk_gather.hip
void launch_gather_votes(const FinalizeArgs& a, const unsigned long long* counters1, hipStream_t stream);
bool vote_table_fits(const FinalizeArgs& a);        // every genome's rows and -cs small enough for the table of voters (bk_gather.hip)
size_t vote_table_words(const IndexView& ix);
void launch_gather_votes_table(const FinalizeArgs& a, const unsigned long long* counters1, uint32_t* tab, const unsigned int* row_bits, hipStream_t stream);
void launch_alias_votes(const FinalizeArgs& a, hipStream_t stream);
void launch_merged_votes(const FinalizeArgs& a, hipStream_t stream);
void launch_zero_genome_rows(unsigned long long* pileup, size_t plane, const uint32_t* file_cell_lo, int n_files, uint32_t total_cells, const int* last_sel,
                             hipStream_t stream);
void launch_copy_int(int* dst, const int* src, hipStream_t stream);
// bk_build.hip: order[i] = index of the i-th smallest of n u64 keys (radix sort on the device over bits [0, end_bit), stable); h_sorted_keys may be null
hipError_t device_sort_order(const unsigned long long* h_keys, size_t n, int end_bit, unsigned int* h_order, unsigned long long* h_sorted_keys);
// bk_build.hip (bk_engine_create): out[i * W + t] = window bucket (slot) of keys[i] at window position t, `empty` where there is none (device buffer),
// valid[i] = the positions found (host); dst[id_of[i] * W + t] = src[i * W + t] (device buffers)
hipError_t device_lookup_slots(const TableSlot* d_table, uint32_t log2s, const unsigned long long* h_keys, size_t n, int W, int wstart, int k, uint32_t empty,
                               uint32_t* d_out, uint32_t* h_valid);
hipError_t device_build_table(TableSlot* d_table, size_t n_table, uint32_t log2s, const unsigned long long* h_keys, const unsigned char* h_ts, size_t n, bool* dup);
hipError_t device_permute_rows(const uint32_t* d_src, const uint32_t* h_id_of, size_t n, int W, uint32_t* d_dst);
bool finalize_runs_by_region(const FinalizeArgs& a);   // launch_finalize will take the regional kernel of bk_finalize_lean.hip (one genome file, whole dense planes, ...)
hipError_t raise_lds_limit(const void* fn, size_t lds);   // the dynamic-LDS limit of a kernel, raised once per process and device

}  // namespace bk
