// bk_index_tables.cpp -- bk_engine_create's table construction: from a decoded BronkoIndex to the device-resident tables of
// IndexTables (window-bucket tables, the set U of reference k-mers and its perfect hash, the per-cell arrays, the dirty answers,
// the half-key directories, the seed tables, ...).  One stage per member function of IndexBuilder, in the order of
// build_index_tables; the PhaseClock laps (BK_CREATE_TIMING) mark the same stages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../host/lcb.hpp"
#include "bk_engine.h"

namespace {

// std::sort on `nt` host threads: sorted chunks, then pairwise merges level by level
template <typename T, typename Cmp>
void parallel_sort(std::vector<T>& v, Cmp cmp, unsigned nt) {
    if (nt < 2 || v.size() < (size_t)nt * 65536) { std::sort(v.begin(), v.end(), cmp); return; }
    std::vector<size_t> cut(nt + 1);
    for (unsigned i = 0; i <= nt; i++) cut[i] = v.size() * i / nt;
    {
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nt; i++) th.emplace_back([&, i] { std::sort(v.begin() + cut[i], v.begin() + cut[i + 1], cmp); });
        for (auto& t : th) t.join();
    }
    for (unsigned step = 1; step < nt; step *= 2) {
        std::vector<std::thread> th;
        for (unsigned i = 0; i + step < nt; i += 2 * step)
            th.emplace_back([&, i, step] { std::inplace_merge(v.begin() + cut[i], v.begin() + cut[i + step], v.begin() + cut[std::min(i + 2 * step, nt)], cmp); });
        for (auto& t : th) t.join();
    }
}

// assign_buckets (lcb.rs:1-45) is the 1-based lexicographic rank of (V, position) where V is the k-mer with the
// wildcard position set to A: ranks are ordered by V, then by position, and V contributes one rank per A it contains
// (verified exhaustively for small k against the reference's known answers).  In exact arithmetic the rank of a k = 31
// bucket reaches 31 * 4^30 ~ 1.94 * 2^64, and the reference keeps it modulo 2^64: two different (position, k-mer)
// pairs whose ranks differ by 2^64 share a bucket.  rank128 / unrank128 are the exact map and its inverse.
using u128 = unsigned __int128;

u128 rank128(uint64_t v /* wildcard position already A */, int pos, int k) {
    u128 cum = 0;   // sum of (number of A digits) over all k-digit strings < v
    int a_pre = 0;
    for (int i = 0; i < k; i++) {
        const int d = (int)((v >> (2 * (k - 1 - i))) & 3);
        const int rest = k - 1 - i;
        const u128 pw = (u128)1 << (2 * rest);                  // 4^rest strings below each smaller digit
        const u128 free_a = rest ? (u128)rest * (pw >> 2) : 0;  // A digits inside the free suffix, summed over them
        for (int x = 0; x < d; x++) cum += (u128)(a_pre + (x == 0)) * pw + free_a;
        a_pre += d == 0;
    }
    int before = 0;
    for (int i = 0; i < pos; i++) before += ((v >> (2 * (k - 1 - i))) & 3) == 0;
    return cum + (u128)before + 1;
}

bool unrank128(u128 r1, int k, uint64_t* v_out, int* pos_out) {
    if (r1 == 0) return false;
    u128 r = r1 - 1;
    uint64_t v = 0;
    int a_pre = 0;
    for (int i = 0; i < k; i++) {
        const int rest = k - 1 - i;
        const u128 pw = (u128)1 << (2 * rest);
        const u128 free_a = rest ? (u128)rest * (pw >> 2) : 0;
        int x = 0;
        for (; x < 4; x++) {
            const u128 c = (u128)(a_pre + (x == 0)) * pw + free_a;
            if (r < c) break;
            r -= c;
        }
        if (x == 4) return false;   // rank beyond k * 4^(k-1)
        v |= (uint64_t)x << (2 * rest);
        a_pre += x == 0;
    }
    // r-th A position of v
    for (int i = 0; i < k; i++)
        if (((v >> (2 * (k - 1 - i))) & 3) == 0) { if (r == 0) { *v_out = v; *pos_out = i; return true; } r -= 1; }
    return false;
}

// Perfect hash of distinct keys (bk_device.h phf_*): buckets of ~4 keys, largest first, smallest free pilot.  Large key sets are
// cut into 2^log2p sub-tables by the leading bits of the bucket index and built on as many host threads; every sub-table has
// msub positions.  On success pos[i] is the position of keys[i] in a table of (msub << log2p) positions.
bool build_phf(const std::vector<uint64_t>& keys, std::vector<uint16_t>& pilots, uint32_t& log2nb, uint32_t& msub_out, uint32_t& log2p_out,
               std::vector<uint32_t>& pos) {
    const size_t n = keys.size();
    uint32_t log2nb0 = 0;
    while ((4ull << log2nb0) < n) log2nb0++;
    pos.assign(n, 0);
    // A construction can fail only when a bucket finds no pilot among 65536: first the tables grow (msub), then the buckets
    // shrink (twice as many, half the keys each) -- the device reads all sizes from the view, so any outcome is a valid
    // table; an index is never refused because of its hash.
    for (uint32_t extra = 0; extra <= 6; extra++) {
        log2nb = log2nb0 + extra;
        if (log2nb > 30) break;
        const uint32_t log2p = n >= (1u << 20) && log2nb >= 10 ? 5u : 0u;
        const size_t P = (size_t)1 << log2p;
        const size_t nb = (size_t)1 << log2nb, nb_sub = nb >> log2p;
        // keys by bucket (counting sort), buckets by sub-table
        std::vector<uint32_t> b_of(n), b_cnt(nb + 1, 0u), by_bucket(n);
        for (size_t i = 0; i < n; i++) { b_of[i] = bk::phf_bucket(keys[i], log2nb); b_cnt[b_of[i] + 1]++; }
        for (size_t x = 0; x < nb; x++) b_cnt[x + 1] += b_cnt[x];
        { std::vector<uint32_t> at(b_cnt.begin(), b_cnt.end() - 1); for (size_t i = 0; i < n; i++) by_bucket[at[b_of[i]]++] = (uint32_t)i; }
        uint64_t max_sub = 0;
        for (size_t sp = 0; sp < P; sp++) max_sub = std::max<uint64_t>(max_sub, b_cnt[(sp + 1) * nb_sub] - b_cnt[sp * nb_sub]);
        uint64_t msub = std::max<uint64_t>(64, (uint64_t)((double)max_sub / 0.97) + 1);
        for (int attempt = 0; attempt <= 8 && (msub << log2p) < (1ull << 31); attempt++, msub += msub / 8 + 1) {
            pilots.assign(nb, 0);
            std::atomic<bool> ok{true};
            auto build_sub = [&](size_t sp) {
                std::vector<uint32_t> order(nb_sub);
                for (size_t x = 0; x < nb_sub; x++) order[x] = (uint32_t)(sp * nb_sub + x);
                std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return b_cnt[x + 1] - b_cnt[x] > b_cnt[y + 1] - b_cnt[y]; });
                std::vector<uint8_t> used(msub, 0);
                std::vector<uint32_t> trial;
                for (uint32_t bkt : order) {
                    const uint32_t m0 = b_cnt[bkt], m1 = b_cnt[bkt + 1];
                    if (m0 == m1) break;
                    uint32_t pilot = 0;
                    for (; pilot < 65536; pilot++) {
                        trial.clear();
                        bool good = true;
                        for (uint32_t q = m0; q < m1; q++) {
                            const uint32_t p = bk::phf_pos(keys[by_bucket[q]], pilot, (uint32_t)msub, log2nb, 0u);   // position inside the sub-table
                            if (used[p] || std::find(trial.begin(), trial.end(), p) != trial.end()) { good = false; break; }
                            trial.push_back(p);
                        }
                        if (good) break;
                    }
                    if (pilot == 65536) { ok = false; return; }
                    pilots[bkt] = (uint16_t)pilot;
                    for (uint32_t q = m0; q < m1; q++) { pos[by_bucket[q]] = (uint32_t)(sp * msub) + trial[q - m0]; used[trial[q - m0]] = 1; }
                }
            };
            if (P == 1) build_sub(0);
            else {
                std::vector<std::thread> th;
                for (size_t sp = 0; sp < P; sp++) th.emplace_back(build_sub, sp);
                for (auto& t : th) t.join();
            }
            if (ok) { msub_out = (uint32_t)msub; log2p_out = log2p; return true; }
        }
    }
    return false;
}


// The buckets are taken in contiguous chunks by host threads, each filling its own output; the chunks are then joined in
// order, so the result is the one a single pass over all buckets gives.
struct ChunkOut {
    std::vector<uint64_t> h_slot_key, h_u, pseudo, per_t;
    std::vector<uint8_t> h_slot_t, h_slot_alias;
    std::vector<uint32_t> h_off, h_len;   // h_off: relative to this chunk's h_ent
    std::vector<bk::DevEntry> h_ent;
    std::vector<uint32_t> merged;   // slots (relative to this chunk's) of buckets that hold more than one key (k = 31: two reference buckets whose ids wrapped onto each other)
    uint64_t n_merged = 0;    // ... the number of such buckets
    uint64_t n_dup = 0;       // buckets that hold one BucketInfo twice
    uint64_t n_real_ent = 0;  // BucketInfos of the window's buckets (each once)
    int code = BK_OK;
    std::string err;
    bool fail(int c, const char* fmt, ...) {
        char buf[512];
        va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
        code = c; err = buf;
        return false;
    }
};

// The locals that bk_engine_create's stages hand to each other, and the stages.
struct IndexBuilder {
    const bk_index_desc* ix;
    const bk_params* prm;
    IndexTables& tab;
    PhaseClock& pc;
    IndexBuilder(const bk_index_desc* ix_, const bk_params* prm_, IndexTables& tab_, PhaseClock& pc_) : ix(ix_), prm(prm_), tab(tab_), pc(pc_) {}
    const int k = ix->k;
    static constexpr uint32_t kNone = 0xffffffffu;
    const unsigned sort_threads = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 64u);

    // sequence_geometry: cell offsets in (file, seq) order
    std::vector<std::vector<uint64_t>> cell_off;
    std::vector<size_t> seq_base;
    uint64_t cells = 0;   // = tab.total_cells
    // buckets_to_slots
    std::vector<uint64_t> h_slot_key;
    std::vector<uint8_t> h_slot_t, h_slot_alias;   // h_slot_alias: the slot's key is the OTHER exact rank that wraps onto its bucket's id (k = 31)
    uint64_t n_merged_buckets = 0, n_dup_entries = 0, n_window_entries = 0;
    std::vector<uint32_t> h_merged_slots;   // the window slots of buckets that hold more than one key
    std::vector<uint32_t> h_off, h_len;
    std::vector<bk::DevEntry> h_ent;
    std::vector<uint64_t> per_t;
    std::vector<uint64_t> h_u;   // canonical reference k-mers that own at least one window bucket (with repeats)
    // k = 31 only: "pseudo" k-mers u*.  A read k-mer equal to u* except possibly at one window position can reach an
    // index bucket through the u64 wrap of its bucket id (see rank128): u* stands for the alias key (j', V') of a
    // real bucket (j, V) with the base of the real k-mer at j' filled in.  The wrap is structured (changing a few
    // leading bases shifts every rank of a k-mer by exactly 2^64), so the W buckets of a reference k-mer usually
    // share one pseudo k-mer.  Which window positions of u* really lead to a bucket is read back from the table.
    std::vector<uint64_t> pseudo;
    // window_tables
    size_t S = 0;
    bool table_on_device = false;
    HostVec<bk::TableSlot> h_table;
    uint32_t empty_slot = 0;
    // reference_set
    std::vector<uint64_t> extra;   // the pseudo k-mers that are not reference k-mers (sorted)
    std::vector<uint32_t> h_valid;   // by index into h_u: the window positions at which the k-mer has a bucket
    std::vector<uint8_t> h_is_pseudo;
    bool slots_on_device = false;
    DevBuf<uint32_t> d_slot_by_index;
    HostVec<uint32_t> slot_by_index;
    // reference_walk
    std::vector<uint32_t> id_of, first_cell;
    std::vector<uint8_t> first_rc;
    std::vector<uint32_t> h_id_at;
    const size_t pad_w = (size_t)bk::scan_ref_pad_words();   // front padding of the two 2-bit arrays
    std::vector<uint32_t> h_refw, h_brc;
    uint64_t n_occurrences = 0;   // cells at which a k-mer of U starts
    std::vector<uint32_t> row_base;
    std::vector<uint32_t> h_nat, h_natrow;   // (dirty_answers)
    // dirty_flags
    std::vector<uint8_t> h_amb;   // by id
    std::vector<uint8_t> h_amb3, h_far23;
    std::vector<uint64_t> h_near;                     // (canonical form's index << 32 | near form), sorted: the near lists
    std::vector<uint8_t> h_no_list;    // by index: in a group too large to enumerate -- no near list
    // cell_arrays
    std::vector<uint8_t> rc_of_id;   // the k-mer's first occurrence was reverse-complemented to become canonical
    std::vector<uint32_t> h_codes, h_yf, h_yr;   // bk_device.h
    std::vector<uint8_t> h_needs_ans;   // by id: some cell of this reference k-mer is not clean
    std::vector<uint8_t> h_cflags;   // bk_device.h kCellClean
    const size_t bpad_w = (size_t)bk::scan_bit_pad_words();
    std::vector<uint32_t> h_has, h_clean, h_clean3, h_fast;
    std::vector<uint2> h_blk;
    // perfect_hash_and_uploads
    std::vector<uint64_t> h_kmer_of;
    // slot_of
    HostVec<uint32_t> h_slot_of;

    bool process_buckets(uint64_t b0, uint64_t b1, ChunkOut& o);
    int sequence_geometry();
    int buckets_to_slots();
    int window_tables();
    int reference_set();
    int reference_walk();
    int dirty_flags();
    int cell_arrays();
    int dirty_answers();
    int perfect_hash_and_uploads();
    int seed_tables();
    int genome_occurrences();
    int half_key_directories();
    int slot_of();
    int slot_rec();
    int estat();
    int lds_policy();
    int table_uploads();
};

int IndexBuilder::sequence_geometry() {
    tab.k = k;
    tab.n_files = ix->n_files;
    // window slice of call.rs:1291-1300
    if (prm->use_full_kmer) { tab.wstart = 0; tab.W = k; }
    else if (prm->n_fixed * 2 + 1 >= k) { tab.wstart = 0; tab.W = 0; }
    else { tab.wstart = prm->n_fixed; tab.W = k - 2 * prm->n_fixed - 1; }

    // cell offsets in (file, seq) order = layout of initialize_output_maps (call.rs:1437-1480)
    cell_off.resize(ix->n_files);
    seq_base.resize(ix->n_files);
    size_t q = 0;
    for (int f = 0; f < ix->n_files; f++) {
        if (ix->n_seqs[f] < 0 || ix->n_seqs[f] > 256) return fail(BK_ERR_INVALID, "file %d: n_seqs out of range (seq_id is u8)", f);
        seq_base[f] = q;
        cell_off[f].resize(ix->n_seqs[f]);
        for (int s = 0; s < ix->n_seqs[f]; s++, q++) { cell_off[f][s] = cells; cells += ix->seq_lens[q]; }
    }
    if (cells >= (1ull << 32)) return fail(BK_ERR_UNSUPPORTED, "more than 2^32 reference positions");
    tab.total_cells = cells;
    {   // sequence geometry for the device caller
        std::vector<uint64_t> g_len(ix->n_files, 0), s_cell, s_len;
        std::vector<int32_t> s_first(ix->n_files, 0), n_s(ix->n_files, 0);
        size_t sq = 0;
        for (int f = 0; f < ix->n_files; f++) {
            s_first[f] = (int32_t)sq; n_s[f] = ix->n_seqs[f];
            tab.max_seqs_per_file = std::max(tab.max_seqs_per_file, (int)ix->n_seqs[f]);
            for (int s2 = 0; s2 < ix->n_seqs[f]; s2++, sq++) { s_cell.push_back(cell_off[f][s2]); s_len.push_back(ix->seq_lens[sq]); g_len[f] += ix->seq_lens[sq]; }
            tab.max_file_cells = std::max(tab.max_file_cells, g_len[f]);
        }
        if (s_cell.empty()) { s_cell.push_back(0); s_len.push_back(0); }
        BK_HIP(tab.genome_len.upload(g_len)); BK_HIP(tab.seq_cell.upload(s_cell)); BK_HIP(tab.seq_len_d.upload(s_len));
        BK_HIP(tab.seq_first.upload(s_first)); BK_HIP(tab.n_seqs_d.upload(n_s));
        tab.h_seq_cell = std::move(s_cell); tab.h_seq_len = std::move(s_len); tab.h_seq_first = std::move(s_first); tab.h_n_seqs = std::move(n_s);
    }
    return BK_OK;
}

bool IndexBuilder::process_buckets(uint64_t b0, uint64_t b1, ChunkOut& o) {
    uint64_t ids[32];
    o.per_t.assign(tab.W > 0 ? tab.W : 1, 0);
    std::vector<std::pair<int, uint64_t>> keys;   // (one allocation per chunk, not per bucket: 37 M mallocs from 256 threads with a hundred strains)
    for (uint64_t b = b0; b < b1; b++) {
        const uint64_t lo = ix->bucket_off[b], hi = ix->bucket_off[b + 1];
        if (hi <= lo) continue;
        if (hi > ix->n_entries) return o.fail(BK_ERR_INVALID, "bucket_off out of range");
        // distinct (j, masked) keys present in this bucket: exactly one unless k = 31 ids wrapped onto each other
        keys.clear();
        uint64_t first_kmer = 0;
        bool any_in_window = false;
        for (uint64_t i = lo; i < hi; i++) {
            const bk_bucket_info& bi = ix->entries[i];
            if (bi.file_id >= ix->n_files || bi.seq_id >= ix->n_seqs[bi.file_id]) return o.fail(BK_ERR_INVALID, "entry %llu references a missing sequence", (unsigned long long)i);
            const size_t sq = seq_base[bi.file_id] + bi.seq_id;
            if ((uint64_t)bi.location + k > ix->seq_lens[sq] || bi.idx >= k) return o.fail(BK_ERR_INVALID, "entry %llu lies outside its sequence", (unsigned long long)i);
            const bronko::Canon cn = bronko::canonical_kmer(ix->seqs[sq] + bi.location, k);
            if (cn.rc != (bi.canonical != 0)) return o.fail(BK_ERR_INVALID, "entry %llu: canonical flag disagrees with the metadata sequence", (unsigned long long)i);
            const int j = bi.idx;
            const uint64_t masked = cn.kmer & ~(3ull << (2 * (k - 1 - j)));
            if (std::find(keys.begin(), keys.end(), std::make_pair(j, masked)) == keys.end()) {
                bronko::assign_buckets(cn.kmer, k, ids);
                if (ids[j] != ix->bucket_ids[b]) return o.fail(BK_ERR_INVALID, "bucket %llu: id does not match assign_buckets of its entries", (unsigned long long)ix->bucket_ids[b]);
                if (keys.empty()) first_kmer = cn.kmer;
                keys.emplace_back(j, masked);
            }
            if (j >= tab.wstart && j < tab.wstart + tab.W) {
                any_in_window = true;
                if (o.h_u.empty() || o.h_u.back() != cn.kmer) o.h_u.push_back(cn.kmer);   // (a bucket of a many-genome index names one k-mer again and again)
            }
        }
        // the other exact rank that wraps onto this bucket's id, if the reference did not already put a k-mer there
        int alias_j = -1;
        uint64_t alias_masked = 0;
        if (k == 31 && keys.size() == 1) {
            const u128 own = rank128(keys[0].second, keys[0].first, k);
            if ((uint64_t)own != ix->bucket_ids[b]) return o.fail(BK_ERR_INVALID, "internal: exact bucket rank disagrees with assign_buckets");
            const u128 two64 = (u128)1 << 64;
            const u128 other = own >= two64 ? own - two64 : own + two64;
            uint64_t av; int aj;
            if (unrank128(other, k, &av, &aj) && aj >= tab.wstart && aj < tab.wstart + tab.W) { alias_j = aj; alias_masked = av; }
        }
        if (!any_in_window && alias_j < 0) continue;
        // every entry of the bucket is voted for by a probe of any of its keys (call.rs:1307-1309 iterates the
        // whole Vec<BucketInfo>), using each entry's own idx (call.rs:1329)
        const uint32_t off = (uint32_t)o.h_ent.size();
        for (uint64_t i = lo; i < hi; i++) {
            const bk_bucket_info& bi = ix->entries[i];
            bk::DevEntry de;
            de.cell = (uint32_t)(cell_off[bi.file_id][bi.seq_id] + bi.location + bi.idx);
            de.file = bi.file_id; de.idx = bi.idx; de.canonical = bi.canonical ? 1 : 0;
            o.h_ent.push_back(de);
        }
        // finalize_variant counts hits per file as run lengths: keep each bucket grouped by file (build_indexes
        // already appends file by file, build.rs:223-228; votes are order-independent)
        std::stable_sort(o.h_ent.begin() + off, o.h_ent.end(), [](const bk::DevEntry& x, const bk::DevEntry& y) { return x.file < y.file; });
        // (what the gathered votes of bk_gather.hip rest on: one key per bucket, every BucketInfo once)
        if (keys.size() > 1) o.n_merged++;
        for (uint64_t i = lo; i < hi; i++) o.n_real_ent += ix->entries[i].idx >= tab.wstart && ix->entries[i].idx < tab.wstart + tab.W;
        if (any_in_window) {
            for (size_t x = off; x < o.h_ent.size(); x++)
                for (size_t y = x + 1; y < o.h_ent.size() && o.h_ent[y].file == o.h_ent[x].file; y++)
                    if (o.h_ent[y].cell == o.h_ent[x].cell && o.h_ent[y].idx == o.h_ent[x].idx) o.n_dup++;
        }
        for (auto& kv : keys) {
            if (kv.first < tab.wstart || kv.first >= tab.wstart + tab.W) continue;
            if (keys.size() > 1) o.merged.push_back((uint32_t)o.h_slot_key.size());
            o.h_slot_key.push_back(kv.second);
            o.h_slot_alias.push_back(0);
            o.h_slot_t.push_back((uint8_t)(kv.first - tab.wstart));
            o.h_off.push_back(off);
            o.h_len.push_back((uint32_t)(hi - lo));
            o.per_t[kv.first - tab.wstart]++;
        }
        if (alias_j >= 0) {
            o.h_slot_key.push_back(alias_masked);
            o.h_slot_alias.push_back(1);
            o.h_slot_t.push_back((uint8_t)(alias_j - tab.wstart));
            o.h_off.push_back(off);
            o.h_len.push_back((uint32_t)(hi - lo));
            o.per_t[alias_j - tab.wstart]++;
            o.pseudo.push_back(alias_masked | (first_kmer & (3ull << (2 * (k - 1 - alias_j)))));
        }
        if (o.h_ent.size() >= (1ull << 32)) return o.fail(BK_ERR_UNSUPPORTED, "more than 2^32 index entries in the window");
    }
    // a reference k-mer is named by every window bucket it owns: each chunk hands over its own distinct ones
    std::sort(o.h_u.begin(), o.h_u.end());
    o.h_u.erase(std::unique(o.h_u.begin(), o.h_u.end()), o.h_u.end());
    return true;
}

int IndexBuilder::buckets_to_slots() {
    // ---- window buckets -> device slots ------------------------------------------------------------------
    // Device key of a bucket = (wildcard position j, canonical reference k-mer with position j zeroed).  It is
    // recomputed from the metadata sequence at (file, seq, location) and checked against the stored bucket id
    // with assign_buckets, so an index that disagrees with its own metadata is rejected instead of miscounted.
    per_t.assign(tab.W > 0 ? tab.W : 1, 0);
    {
        const uint64_t nbk = tab.W > 0 ? ix->n_buckets : 0;
        const unsigned nt = nbk < 65536 ? 1u : std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 256u);
        std::vector<ChunkOut> outs(nt);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) {
            const uint64_t b0 = nbk * t / nt, b1 = nbk * (t + 1) / nt;
            if (nt == 1) process_buckets(b0, b1, outs[0]);
            else th.emplace_back([&, t, b0, b1] { process_buckets(b0, b1, outs[t]); });
        }
        for (auto& t : th) t.join();
        for (auto& o : outs) if (o.code != BK_OK) return fail(o.code, "%s", o.err.c_str());
        pc.lap("  buckets: chunks");
        uint64_t n_ent = 0;
        for (auto& o : outs) n_ent += o.h_ent.size();
        if (n_ent >= (1ull << 32)) return fail(BK_ERR_UNSUPPORTED, "more than 2^32 index entries in the window");
        // the chunks' lists back to back, in chunk order: where each goes is a prefix sum, the copies run side by side
        std::vector<size_t> e0(nt + 1, h_ent.size()), s0(nt + 1, h_slot_key.size()), u0(nt + 1, h_u.size()), p0(nt + 1, pseudo.size());
        for (unsigned t = 0; t < nt; t++) {
            e0[t + 1] = e0[t] + outs[t].h_ent.size(); s0[t + 1] = s0[t] + outs[t].h_slot_key.size();
            u0[t + 1] = u0[t] + outs[t].h_u.size(); p0[t + 1] = p0[t] + outs[t].pseudo.size();
            for (size_t w = 0; w < per_t.size() && w < outs[t].per_t.size(); w++) per_t[w] += outs[t].per_t[w];
        }
        for (auto& o : outs) { n_merged_buckets += o.n_merged; n_dup_entries += o.n_dup; n_window_entries += o.n_real_ent; }
        for (unsigned t = 0; t < nt; t++) for (uint32_t rel : outs[t].merged) h_merged_slots.push_back((uint32_t)(s0[t] + rel));
        h_ent.resize(e0[nt]); h_slot_key.resize(s0[nt]); h_slot_t.resize(s0[nt]); h_slot_alias.resize(s0[nt]); h_len.resize(s0[nt]); h_off.resize(s0[nt]);
        h_u.resize(u0[nt]); pseudo.resize(p0[nt]);
        {
            std::vector<std::thread> cp;
            for (unsigned t = 0; t < nt; t++) cp.emplace_back([&, t] {
                ChunkOut& o = outs[t];
                std::copy(o.h_ent.begin(), o.h_ent.end(), h_ent.begin() + (ptrdiff_t)e0[t]);
                std::copy(o.h_slot_key.begin(), o.h_slot_key.end(), h_slot_key.begin() + (ptrdiff_t)s0[t]);
                std::copy(o.h_slot_t.begin(), o.h_slot_t.end(), h_slot_t.begin() + (ptrdiff_t)s0[t]);
                std::copy(o.h_slot_alias.begin(), o.h_slot_alias.end(), h_slot_alias.begin() + (ptrdiff_t)s0[t]);
                std::copy(o.h_len.begin(), o.h_len.end(), h_len.begin() + (ptrdiff_t)s0[t]);
                for (size_t i = 0; i < o.h_off.size(); i++) h_off[s0[t] + i] = (uint32_t)e0[t] + o.h_off[i];
                std::copy(o.h_u.begin(), o.h_u.end(), h_u.begin() + (ptrdiff_t)u0[t]);
                std::copy(o.pseudo.begin(), o.pseudo.end(), pseudo.begin() + (ptrdiff_t)p0[t]);
                o = ChunkOut();   // free
            });
            for (auto& t : cp) t.join();
        }
    }
    pc.lap("buckets -> slots (+aliases)");
    tab.n_slots = h_slot_key.size();
    if (tab.n_slots >= (1ull << 31)) return fail(BK_ERR_UNSUPPORTED, "too many window buckets");
    return BK_OK;
}

int IndexBuilder::window_tables() {
    uint64_t max_t = 1;
    for (uint64_t c : per_t) max_t = std::max(max_t, c);
    tab.log2s = 4;
    while ((1ull << tab.log2s) < 2 * max_t) tab.log2s++;   // load factor <= 0.5
    S = (size_t)1 << tab.log2s;
    // (a large index: built on the device, where the probes of U below run too -- the host never holds it)
    table_on_device = tab.n_slots >= (1u << 18) && tab.W > 0;
    if (table_on_device) {
        bool dup = false;
        BK_HIP(tab.table.alloc((size_t)tab.W * S));
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
        BK_HIP(bk::device_build_table(tab.table.p, (size_t)tab.W * S, tab.log2s, reinterpret_cast<const unsigned long long*>(h_slot_key.data()), h_slot_t.data(), tab.n_slots, &dup));
        if (dup && k != 31) return fail(BK_ERR_INVALID, "duplicate window bucket in the index");
    } else {
    h_table = filled((size_t)std::max(tab.W, 1) * S, bk::TableSlot{bk::kEmptyKey, 0u, 0u});
    pc.lap("  window tables: allocation");
    {
        // one sub-table per window position: each is filled by its own host thread, in slot order (the first of equal keys stays)
        std::atomic<bool> dup{false};
        auto fill = [&](int t0, int t1) {
            for (uint64_t s = 0; s < tab.n_slots; s++) {
                const int t = h_slot_t[s];
                if (t < t0 || t >= t1) continue;
                bk::TableSlot* sub = h_table.data() + (size_t)t * S;
                uint32_t h = bk::hash_key(h_slot_key[s], tab.log2s);
                while (sub[h].key != bk::kEmptyKey) {
                    if (sub[h].key == h_slot_key[s]) {
                        if (k != 31) dup = true;   // (k = 31: an alias key that coincides with a real key -- same wrapped id, same bucket: keep the first)
                        break;
                    }
                    h = (h + 1) & (uint32_t)(S - 1);
                }
                if (sub[h].key == bk::kEmptyKey) { sub[h].key = h_slot_key[s]; sub[h].slot = (uint32_t)s; }
            }
        };
        const int nth = tab.n_slots < 262144 ? 1 : std::max(1, std::min<int>(tab.W, (int)std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        for (int q = 1; q < nth; q++) th.emplace_back(fill, tab.W * q / nth, tab.W * (q + 1) / nth);
        fill(0, tab.W / nth > 0 ? tab.W / nth : tab.W);
        for (auto& t : th) t.join();
        if (dup) return fail(BK_ERR_INVALID, "duplicate window bucket in the index");
    }
    }
    pc.lap("window tables");
    // a slot with no entries: "this k-mer has no bucket at that window position" (pseudo k-mers)
    empty_slot = (uint32_t)h_off.size();
    h_off.push_back(0);
    h_len.push_back(0);
    return BK_OK;
}

int IndexBuilder::reference_set() {
    // ---- reference k-mer set U ------------------------------------------------------------------------------
    // ids in order of first occurrence in reference order; perfect hash (membership + diagonal seeding);
    // half-key directories (neighbour search); the reference in reference order (diagonal walk); per-id tables.
    parallel_sort(h_u, std::less<uint64_t>(), sort_threads);
    h_u.erase(std::unique(h_u.begin(), h_u.end()), h_u.end());
    pc.lap("  U: sort");
    // pseudo k-mers join U (so that the membership / neighbour machinery finds the read k-mers that alias), but they
    // own only the window positions at which the table holds a key for them.  A pseudo value that is a real
    // reference k-mer needs nothing: its alias key is that k-mer's own bucket key.
    parallel_sort(pseudo, std::less<uint64_t>(), sort_threads);
    pseudo.erase(std::unique(pseudo.begin(), pseudo.end()), pseudo.end());
    {
        std::vector<uint8_t> keep(pseudo.size(), 0);
        parallel_for(pseudo.size(), [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) keep[i] = std::binary_search(h_u.begin(), h_u.end(), pseudo[i]) ? 0 : 1;
        });
        for (size_t i = 0; i < pseudo.size(); i++) if (keep[i]) extra.push_back(pseudo[i]);   // (sorted, like pseudo)
    }
    {
        const size_t mid = h_u.size();
        h_u.insert(h_u.end(), extra.begin(), extra.end());
        std::inplace_merge(h_u.begin(), h_u.begin() + (ptrdiff_t)mid, h_u.end());   // two sorted, disjoint runs
    }
    pc.lap("  U: pseudo k-mers sorted, merged");
    // bucket (slot) of every k-mer of U at every window position, by table lookup; h_valid = positions with a bucket
    h_valid.assign(h_u.size(), 0u);
    h_is_pseudo.assign(h_u.size(), 0);
    // (a large index: the probes run on the device, against the tables where they will stay -- 400 M of them with a hundred strains
    // at k = 31, DRAM latency on the host; the slots stay on the device until they are laid out by id, slot_of below)
    slots_on_device = (h_u.size() >= (1u << 18) || table_on_device) && tab.W > 0;
    std::atomic<bool> lacks{false};
    if (slots_on_device) {
        if (!table_on_device) BK_HIP(tab.table.upload(h_table));
        BK_HIP(d_slot_by_index.alloc(h_u.size() * (size_t)tab.W));
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
        BK_HIP(bk::device_lookup_slots(tab.table.p, tab.log2s, reinterpret_cast<const unsigned long long*>(h_u.data()), h_u.size(), tab.W, tab.wstart, k, empty_slot,
                                       d_slot_by_index.p, h_valid.data()));
        const uint32_t all = tab.W >= 32 ? 0xffffffffu : (1u << tab.W) - 1u;
        parallel_for(h_u.size(), [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                h_is_pseudo[i] = std::binary_search(extra.begin(), extra.end(), h_u[i]) ? 1 : 0;
                if (!h_is_pseudo[i] && h_valid[i] != all) lacks = true;
            }
        });
    } else {
    slot_by_index = filled((size_t)std::max<size_t>(h_u.size(), 1) * std::max(tab.W, 1), empty_slot);
    pc.lap("  U: slot_by_index allocation");
    parallel_for(h_u.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            h_is_pseudo[i] = std::binary_search(extra.begin(), extra.end(), h_u[i]) ? 1 : 0;
            for (int t = 0; t < tab.W; t++) {
                const uint64_t key = h_u[i] & ~(3ull << (2 * (k - 1 - (tab.wstart + t))));
                const bk::TableSlot* sub = h_table.data() + (size_t)t * S;
                uint32_t h = bk::hash_key(key, tab.log2s);
                while (sub[h].key != key && sub[h].key != bk::kEmptyKey) h = (h + 1) & (uint32_t)(S - 1);
                if (sub[h].key == key) { slot_by_index[i * tab.W + t] = sub[h].slot; h_valid[i] |= 1u << t; }
                else if (!h_is_pseudo[i]) lacks = true;
            }
        }
    });
    }
    if (lacks) return fail(BK_ERR_INVALID, "index lacks a window bucket of one of its own reference k-mers");
    pc.lap("U + slot lookup");
    tab.lo_bases = k / 2;
    if (h_u.size() >= (1ull << 31)) return fail(BK_ERR_UNSUPPORTED, "too many distinct reference k-mers");
    tab.n_u = (uint32_t)h_u.size();
    return BK_OK;
}

int IndexBuilder::reference_walk() {
    // walk the metadata sequences: ids, first occurrences, packed bases and the per-cell flag bits
    id_of.assign(h_u.size(), kNone); first_cell.assign(h_u.size(), kNone);
    first_rc.assign(h_u.size(), 0);
    h_id_at.assign(std::max<uint64_t>(cells, 1), kNone);
    h_refw.assign(pad_w + (cells + 15) / 16 + (size_t)bk::scan_ref_back_words(), 0u); h_brc.assign((cells + 31) / 32 + 1, 0u);
    uint32_t next_id = 0;
    // first every cell's k-mer is looked up in U (the sequences side by side on host threads; h_id_at holds the index into
    // h_u for the moment), then the ids are handed out in reference order
    std::vector<uint8_t> cell_rc(std::max<uint64_t>(cells, 1), 0);
    {
        struct SeqJob { const uint8_t* seq; uint64_t len, c0; };
        std::vector<SeqJob> jobs;
        size_t sq = 0;
        for (int f = 0; f < ix->n_files; f++)
            for (int sidx = 0; sidx < ix->n_seqs[f]; sidx++, sq++) {
                const uint64_t len = ix->seq_lens[sq], c0 = cell_off[f][sidx];
                const uint8_t* seq = ix->seqs[sq];
                // (on the way: the runs of letters that are not ACGT, which this packing reads as A -- bk_indels_enable keeps records off them)
                uint64_t run0 = len;   // first letter of the open run; len: none is open
                for (uint64_t i = 0; i < len; i++) {
                    h_refw[pad_w + ((c0 + i) >> 4)] |= (uint32_t)bronko::nt_to_bits(seq[i]) << (2 * ((c0 + i) & 15));
                    const bool other = bronko::acgt_code(seq[i]) < 0;
                    if (other && run0 == len) run0 = i;
                    else if (!other && run0 != len) { tab.h_nonacgt.push_back(make_uint2((uint32_t)(c0 + run0), (uint32_t)(c0 + i))); run0 = len; }
                }
                if (run0 != len) tab.h_nonacgt.push_back(make_uint2((uint32_t)(c0 + run0), (uint32_t)(c0 + len)));
                // long sequences in pieces (every piece re-reads the k - 1 bases before it)
                for (uint64_t a = 0; a + k <= len; a += 8192) jobs.push_back(SeqJob{seq + a, std::min<uint64_t>(len - a, 8192 + (uint64_t)k - 1), c0 + a});
            }
        std::atomic<size_t> next_job{0};
        auto work = [&] {
            const uint64_t mask = bronko::kmer_mask(k);
            for (size_t j = next_job++; j < jobs.size(); j = next_job++) {
                const SeqJob& jb = jobs[j];
                uint64_t fwd = 0;
                for (int i = 0; i < k - 1; i++) fwd = (fwd << 2) | bronko::nt_to_bits(jb.seq[i]);
                for (uint64_t i = 0; i + k <= jb.len; i++) {
                    fwd = ((fwd << 2) | bronko::nt_to_bits(jb.seq[i + k - 1])) & mask;
                    const bronko::Canon cn = bronko::canonical_u64(fwd, k);
                    const auto it = std::lower_bound(h_u.begin(), h_u.end(), cn.kmer);   // h_u is sorted
                    if (it == h_u.end() || *it != cn.kmer) continue;   // not in the index: never predicted, never counted
                    h_id_at[jb.c0 + i] = (uint32_t)(it - h_u.begin());
                    cell_rc[jb.c0 + i] = cn.rc ? 1 : 0;
                }
            }
        };
        const unsigned nt = jobs.size() < 4 ? 1u : std::min<unsigned>(sort_threads, (unsigned)jobs.size());
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
    }
    n_occurrences = 0;
    for (uint64_t cell = 0; cell < cells; cell++) {
        const uint32_t ui = h_id_at[cell];
        if (ui == kNone) continue;
        ++n_occurrences;
        if (id_of[ui] == kNone) { id_of[ui] = next_id++; first_cell[ui] = (uint32_t)cell; first_rc[ui] = cell_rc[cell]; }
        h_id_at[cell] = id_of[ui];
        if (cell_rc[cell]) h_brc[cell >> 5] |= 1u << (cell & 31);
    }
    for (size_t i = 0; i < h_u.size(); i++)   // k-mers known only through index entries: ids after the others
        if (id_of[i] == kNone && !h_is_pseudo[i]) id_of[i] = next_id++;
    tab.n_full = next_id;
    for (size_t i = 0; i < h_u.size(); i++)   // pseudo k-mers last: they own V rows only where they own a bucket
        if (id_of[i] == kNone) id_of[i] = next_id++;
    // NbEntry::p (bk_device.h): the id of a reference k-mer; n_full + first pseudo V row of a pseudo k-mer (rows in id order)
    row_base.assign(h_u.size(), 0u);
    // with full_kmer_stats the rows keep every offset, so that k-mers differing outside the window are not lost to the statistics
    tab.v_omin = bk::v_layout_omin(k, tab.wstart, tab.W, prm->full_kmer_stats != 0);
    tab.v_span = bk::v_layout_span(k, tab.wstart, tab.W, prm->full_kmer_stats != 0);
    {
        std::vector<uint32_t> idx_by_id(h_u.size());
        for (size_t i = 0; i < h_u.size(); i++) idx_by_id[id_of[i]] = (uint32_t)i;
        uint64_t rows = 0;
        std::vector<uint32_t> h_prow_id;
        std::vector<uint8_t> h_prow_t;
        for (size_t id = 0; id < h_u.size(); id++) {
            const uint32_t i = idx_by_id[id];
            if (id < tab.n_full) { row_base[i] = (uint32_t)id; continue; }
            row_base[i] = (uint32_t)(tab.n_full + rows);
            for (int t = 0; t < tab.W; t++)
                if ((h_valid[i] >> t) & 1u) { h_prow_id.push_back((uint32_t)id); h_prow_t.push_back((uint8_t)t); rows++; }
            if (tab.n_full + rows >= (1ull << 31)) return fail(BK_ERR_UNSUPPORTED, "index too large: too many pseudo k-mer buckets");
        }
        tab.n_prows = rows;
        if (bk::v_plane_len(tab.n_full, tab.v_span, rows) >= (1ull << 32)) return fail(BK_ERR_UNSUPPORTED, "index too large: variant counter plane exceeds 2^32 counters");
        bk::counter_plane_layout(tab.n_u, tab.n_full, tab.v_span, rows, tab.v_off, tab.plane_len);
        if (h_prow_id.empty()) { h_prow_id.push_back(0); h_prow_t.push_back(0); }
        BK_HIP(tab.prow_id.upload(h_prow_id));
        BK_HIP(tab.prow_t.upload(h_prow_t));
    }

    pc.lap("reference walk + ids");
    return BK_OK;
}

int IndexBuilder::dirty_flags() {
    // dirty flags (bk_device.h amb): another reference k-mer, on either strand, within Hamming distance 2, or
    // the k-mer within distance 2 of its own reverse complement.  Any two 2k-bit words at distance <= 2 agree
    // on at least one of three parts, so group all forms (u and rc(u)) by each part and compare inside groups.
    h_amb.assign(h_u.size(), 0);
    // amb3: the same with distance 3 (four parts); lets Level 2 discard k-mers with two differences on the spot.  The
    // groups grow with |U| (a quarter of a k-mer distinguishes little): above kAmb3MaxKmers everything is flagged.
    h_amb3.assign(h_u.size(), 0);
    // far23: another reference k-mer form at distance 2 or 3 (forms one base away do not count): where there is none, a read k-mer
    // two bases from u can only equal or neighbour the two k-mers "u with one of its two differences" (Level 2, kCellIso23)
    h_far23.assign(h_u.size(), 0);
    constexpr size_t kAmb3MaxKmers = 300000;
    h_no_list.assign(h_u.size(), 0);
    {
        struct Form { uint64_t w; uint32_t id; uint32_t fi; };   // fi = 2 * (index into h_u) + (1: the reverse complement)
        std::vector<Form> forms(h_u.size() * 2);
        parallel_for(h_u.size(), [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                forms[2 * i] = Form{h_u[i], id_of[i], (uint32_t)(2 * i)};
                forms[2 * i + 1] = Form{bronko::reverse_complement_u64(h_u[i], k), id_of[i], (uint32_t)(2 * i + 1)};
            }
        });
        // collect: for every canonical form, the forms within `dist` of it (the near lists the dirty answers are worked out from)
        // out_far (optional): the same for pairs at distance 2 or more only -- what kCellIso23 is made of (bk_device.h)
        std::vector<uint8_t>* out_far = nullptr;
        auto flag_within = [&](int dist, std::vector<uint8_t>& out, std::vector<std::vector<uint64_t>>* collect) {
            const int parts = dist + 1;   // words at distance <= dist agree on at least one of dist + 1 parts
            if (collect) collect->assign(parts, {});
            std::vector<std::thread> th;
            const unsigned per_part = std::max(1u, std::min(64u, std::thread::hardware_concurrency() / (unsigned)parts));
            for (int part = 0; part < parts; part++) th.emplace_back([&, part] {   // (flags are only ever set to 1: benign races)
                std::vector<uint64_t>* near = collect ? &(*collect)[part] : nullptr;
                const int c0 = (part * k) / parts, c1 = ((part + 1) * k) / parts;
                const uint64_t mask = (((1ull << (2 * (c1 - c0))) - 1ull) << (2 * c0));
                // the forms grouped by this part: a radix sort of the part's bits on the device, the forms gathered in that order
                // (std::sort of 30 M forms on 24 host threads per part was 1.4 s of a 100-strain create)
                std::vector<Form> fs;
                bool on_device = false;
                if (forms.size() >= (1u << 16) && hipSetDevice(prm->device) == hipSuccess) {
                    std::vector<unsigned long long> keys(forms.size());
                    std::vector<unsigned int> order(forms.size());
                    parallel_for(forms.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) keys[i] = (forms[i].w & mask) >> (2 * c0); });
                    if (bk::device_sort_order(keys.data(), keys.size(), 2 * (c1 - c0), order.data(), nullptr) == hipSuccess) {
                        fs.resize(forms.size());
                        parallel_for(forms.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) fs[i] = forms[order[i]]; });
                        on_device = true;
                    }
                }
                if (!on_device) {
                    fs = forms;
                    parallel_sort(fs, [&](const Form& x, const Form& y) { return (x.w & mask) < (y.w & mask); }, per_part);
                }
                // the groups (equal parts), dealt to threads in runs of whole groups; every thread collects its own near pairs
                const unsigned nt = fs.size() < 262144 ? 1u : per_part;
                std::vector<size_t> cut(nt + 1, fs.size());
                cut[0] = 0;
                for (unsigned t = 1; t < nt; t++) {
                    size_t a = std::max(fs.size() * t / nt, cut[t - 1]);
                    while (a < fs.size() && a > 0 && (fs[a].w & mask) == (fs[a - 1].w & mask)) a++;
                    cut[t] = a;
                }
                std::vector<std::vector<uint64_t>> mine(nt);
                auto scan_groups = [&](size_t lo, size_t hi, std::vector<uint64_t>& out_near) {
                    for (size_t a0 = lo; a0 < hi;) {
                        size_t a1 = a0 + 1;
                        while (a1 < hi && (fs[a1].w & mask) == (fs[a0].w & mask)) a1++;
                        if (a1 - a0 > 4096) {   // pathological low-complexity group: flag all, skip the quadratic pass
                            for (size_t x = a0; x < a1; x++) { out[fs[x].id] = 1; if (out_far) (*out_far)[fs[x].id] = 1; if (near) h_no_list[fs[x].fi >> 1] = 1; }
                        } else {
                            // (pseudo k-mers -- 95 % of U with a hundred strains at k = 31 -- are flagged dirty whatever their neighbours
                            // and own no near list: a pair of two of them says nothing, and only a reference k-mer's list is kept)
                            for (size_t x = a0; x < a1; x++) {
                                const bool px = h_is_pseudo[fs[x].fi >> 1] != 0;
                                for (size_t y = x + 1; y < a1; y++) {
                                    const bool py = h_is_pseudo[fs[y].fi >> 1] != 0;
                                    if (px && py) continue;
                                    const uint64_t d = fs[x].w ^ fs[y].w;
                                    const int nd = __builtin_popcountll((d | (d >> 1)) & 0x5555555555555555ull);
                                    if (nd <= dist) {
                                        out[fs[x].id] = out[fs[y].id] = 1;   // also catches u vs rc(u) (same id)
                                        if (out_far && nd >= 2) (*out_far)[fs[x].id] = (*out_far)[fs[y].id] = 1;
                                        if (near) {   // (owner canonical form << 32) | the other form
                                            if (!(fs[x].fi & 1u) && !px) out_near.push_back(((uint64_t)(fs[x].fi >> 1) << 32) | fs[y].fi);
                                            if (!(fs[y].fi & 1u) && !py) out_near.push_back(((uint64_t)(fs[y].fi >> 1) << 32) | fs[x].fi);
                                        }
                                    }
                                }
                            }
                        }
                        a0 = a1;
                    }
                };
                {
                    std::vector<std::thread> gt;
                    for (unsigned t = 1; t < nt; t++) gt.emplace_back([&, t] { scan_groups(cut[t], cut[t + 1], mine[t]); });
                    scan_groups(cut[0], cut[1], mine[0]);
                    for (auto& t : gt) t.join();
                }
                if (near) for (auto& v : mine) { near->insert(near->end(), v.begin(), v.end()); std::vector<uint64_t>().swap(v); }
            });
            for (auto& t : th) t.join();
        };
        std::vector<std::vector<uint64_t>> near_parts;
        flag_within(2, h_amb, &near_parts);
        pc.lap("  dirty: distance 2");
        if (h_u.size() <= kAmb3MaxKmers) { out_far = &h_far23; flag_within(3, h_amb3, nullptr); out_far = nullptr; }
        else { std::fill(h_amb3.begin(), h_amb3.end(), (uint8_t)1); std::fill(h_far23.begin(), h_far23.end(), (uint8_t)1); }
        pc.lap("  dirty: distance 3");
        size_t tot = 0;
        for (auto& v : near_parts) tot += v.size();
        h_near.reserve(tot);
        for (auto& v : near_parts) { h_near.insert(h_near.end(), v.begin(), v.end()); std::vector<uint64_t>().swap(v); }
        {
            bool on_device = false;
            if (h_near.size() >= (1u << 20) && h_near.size() < (1ull << 32) && hipSetDevice(prm->device) == hipSuccess) {
                std::vector<unsigned int> order(h_near.size());
                std::vector<unsigned long long> sorted(h_near.size());
                static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
                if (bk::device_sort_order(reinterpret_cast<const unsigned long long*>(h_near.data()), h_near.size(), 64, order.data(), sorted.data()) == hipSuccess) {
                    parallel_for(h_near.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) h_near[i] = sorted[i]; });
                    on_device = true;
                }
            }
            if (!on_device) parallel_sort(h_near, std::less<uint64_t>(), sort_threads);
        }
        pc.lap("  dirty: near lists sorted");
        h_near.erase(std::unique(h_near.begin(), h_near.end()), h_near.end());
    }
    for (size_t i = 0; i < h_u.size(); i++) if (h_is_pseudo[i]) { h_amb3[id_of[i]] = 1; h_far23[id_of[i]] = 1; }
    if (test_env("BK_NO_ISO23")) std::fill(h_far23.begin(), h_far23.end(), (uint8_t)1);
    for (size_t i = 0; i < h_u.size(); i++) if (h_is_pseudo[i]) h_amb[id_of[i]] = 1;
    pc.lap("dirty flags (dist 2, 3)");
    return BK_OK;
}

int IndexBuilder::cell_arrays() {
    rc_of_id.assign(h_u.size(), 0);
    for (size_t i = 0; i < h_u.size(); i++) rc_of_id[id_of[i]] = first_rc[i];
    h_codes.assign(h_refw.size(), 0u); h_yf.assign(h_refw.size(), 0u); h_yr.assign(h_refw.size(), 0u);
    h_needs_ans.assign(h_u.size(), 0);
    h_cflags.assign(std::max<uint64_t>(cells, 1), 0);
    h_has.assign(bpad_w + (cells + 31) / 32 + (size_t)bk::scan_bit_back_words(), 0u); h_clean.assign(h_has.size(), 0u); h_clean3.assign(h_has.size(), 0u);
    for (uint64_t c = 0; c < cells; c++) {
        if (h_id_at[c] == kNone) continue;
        const size_t wi = pad_w + (c >> 4);
        const int sh = 2 * (int)(c & 15);
        h_codes[wi] |= (((h_brc[c >> 5] >> (c & 31)) & 1u) ? 2u : 1u) << sh;
        // clean also promises the orientation of the k-mer's first occurrence (the V layout is built on it): an
        // occurrence on the other strand of a reverse-complement repeat is resolved by the general path
        const uint32_t rc_here = (h_brc[c >> 5] >> (c & 31)) & 1u;
        const uint32_t clean = (h_amb[h_id_at[c]] || rc_here != rc_of_id[h_id_at[c]]) ? 0u : 1u;
        const bool from_prev = c > 0 && h_id_at[c - 1] != kNone && h_id_at[c] == h_id_at[c - 1] + 1;
        const bool to_next = c + 1 < cells && h_id_at[c + 1] != kNone && h_id_at[c + 1] == h_id_at[c] + 1;
        h_has[bpad_w + (c >> 5)] |= 1u << (c & 31);
        if (clean) h_clean[bpad_w + (c >> 5)] |= 1u << (c & 31);
        else h_needs_ans[h_id_at[c]] = 1;
        h_cflags[c] = (uint8_t)((rc_here ? 2u : 1u) | (clean ? bk::kCellClean : 0u) | (h_amb3[h_id_at[c]] ? 0u : bk::kCellClean3) |
                                (rc_here == rc_of_id[h_id_at[c]] ? bk::kCellFirstOri : 0u) | (h_far23[h_id_at[c]] ? 0u : bk::kCellIso23));
        if (!h_amb3[h_id_at[c]]) h_clean3[bpad_w + (c >> 5)] |= 1u << (c & 31);
        h_yf[wi] |= (clean | (from_prev ? 2u : 0u)) << sh;
        h_yr[wi] |= (clean | (to_next ? 2u : 0u)) << sh;
    }

    // what the scan needs to count an isolated mismatch on the spot (bk_device.h cell_fast / cell_blk): per block of 64 cells the
    // constant id - cell of its clean cells and the end of the stretch of cells that carry a reference k-mer
    h_fast.assign(h_has.size(), 0u);
    h_blk.assign((cells + 63) / 64 + 3, make_uint2(0u, (uint32_t)cells));
    {
        uint32_t next_none = (uint32_t)cells;
        for (uint64_t c = cells; c-- > 0;) {
            if (h_id_at[c] == kNone) next_none = (uint32_t)c;
            if ((c & 63) == 0) h_blk[c >> 6].y = next_none;
        }
        // x: the most common id - cell among the block's cells that stand in their k-mer's first orientation (clean or not:
        // with many related genomes no cell is clean, and cell_nat below still wants the constant)
        for (uint64_t b0 = 0; b0 < cells; b0 += 64) {
            uint32_t best = 0u, best_n = 0u;
            const uint64_t b1 = std::min<uint64_t>(b0 + 64, cells);
            for (uint64_t c = b0; c < b1; c++) {
                if (!(h_cflags[c] & bk::kCellFirstOri)) continue;
                const uint32_t delta = h_id_at[c] - (uint32_t)c;
                if (best_n && delta == best) continue;
                uint32_t n = 0;
                for (uint64_t q = c; q < b1; q++) n += (h_cflags[q] & bk::kCellFirstOri) && h_id_at[q] - (uint32_t)q == delta;
                if (n > best_n) { best_n = n; best = delta; }
            }
            h_blk[b0 >> 6].x = best;
        }
        for (uint64_t c = 0; c < cells; c++)
            if ((h_cflags[c] & bk::kCellClean) && h_id_at[c] - (uint32_t)c == h_blk[c >> 6].x) h_fast[bpad_w + (c >> 5)] |= 1u << (c & 31);
    }
    pc.lap("per-cell arrays");
    return BK_OK;
}

int IndexBuilder::dirty_answers() {
    // ---- dirty answers (bk_device.h DirtyAns): for every reference k-mer with a cell that is not clean, what "this k-mer with
    // base bb at position j" is -- worked out from its near list (every reference k-mer form within Hamming distance 2: a
    // k-mer one base away from u can only equal, or neighbour, forms within distance 2 of u).  Same rule as the neighbour
    // search of Level 2's slow pipeline: a reference k-mer if it equals one, else the smallest (window position, NbEntry::p)
    // among the reference k-mers one base away in the window that own a bucket there, else nothing.
    {
        std::vector<uint32_t> idx_by_id(h_u.size());
        for (size_t i = 0; i < h_u.size(); i++) idx_by_id[id_of[i]] = (uint32_t)i;
        // rows are indexed by id (no indirection: Level 2 reads an answer with one load); only the rows of k-mers with a
        // cell that is not clean are filled in -- the others are never read
        std::vector<uint32_t> owners;   // index into h_u of each filled row
        for (size_t id = 0; id < tab.n_full; id++)
            if (h_needs_ans[id] || h_amb[id]) owners.push_back(idx_by_id[id]);   // (a dirty k-mer without a cell: finalize still asks)
        const bool build = tab.W > 0 && bk::ans_table_len(tab.n_full, k) * sizeof(bk::DirtyAns) <= ((size_t)16 << 30);
        if (build && !owners.empty()) {
            std::vector<bk::DirtyAns> h_ans(bk::ans_table_len(tab.n_full, k), bk::DirtyAns{0u, 0u});
            // entry of "reference k-mer id (index i into h_u) with base bb at position j of its canonical form" (bk_device.h ans_index)
            auto ans_at = [&](uint32_t i, int j, uint32_t bb) -> bk::DirtyAns& {
                const bool rc1 = first_rc[i] != 0;
                return h_ans[bk::ans_index(id_of[i], (uint32_t)(rc1 ? k - 1 - j : j), rc1 ? 3u - bb : bb, k)];
            };
            const uint64_t vreal = bk::v_real_len(tab.n_full, tab.v_span);
            auto diff1 = [&](uint64_t a, uint64_t b) -> int {   // position (from the left) of the single differing base, or -1
                const uint64_t x = a ^ b, y = (x | (x >> 1)) & 0x5555555555555555ull;
                if (y == 0 || (y & (y - 1)) != 0) return -1;
                return k - 1 - (__builtin_ctzll(y) >> 1);
            };
            parallel_for(owners.size(), [&](size_t r0, size_t r1) {
                std::vector<std::pair<uint64_t, uint32_t>> fl;   // (form word, form index) of u itself and its near forms
                for (size_t r = r0; r < r1; r++) {
                    const uint32_t i = owners[r];
                    const uint64_t u = h_u[i];
                    if (h_no_list[i]) {   // a low-complexity group too large to enumerate: no near list, no answers
                        for (int j = 0; j < k; j++) for (uint32_t bb = 0; bb < 4; bb++) ans_at(i, j, bb) = bk::DirtyAns{0u, bk::kAnsNone};
                        continue;
                    }
                    fl.clear();
                    fl.emplace_back(u, (uint32_t)(2 * i));
                    for (auto it = std::lower_bound(h_near.begin(), h_near.end(), (uint64_t)i << 32); it != h_near.end() && (*it >> 32) == i; ++it) {
                        const uint32_t fi = (uint32_t)*it;
                        fl.emplace_back((fi & 1u) ? bronko::reverse_complement_u64(h_u[fi >> 1], k) : h_u[fi >> 1], fi);
                    }
                    for (int j = 0; j < k; j++) {
                        const int sh = 2 * (k - 1 - j);
                        for (uint32_t bb = 0; bb < 4; bb++) {
                            if (((u >> sh) & 3ull) == bb) continue;
                            bk::DirtyAns& A = ans_at(i, j, bb);
                            const uint64_t z = (u & ~(3ull << sh)) | ((uint64_t)bb << sh);
                            const uint64_t zr = bronko::reverse_complement_u64(z, k);
                            const bool flip = zr < z;              // the canonical form of z is its reverse complement
                            const uint64_t c = flip ? zr : z;
                            bool member = false;
                            uint64_t best = ~0ull; uint32_t best_fi = 0, jmask = 0;
                            for (auto& f : fl) {
                                // a form says something about c (the canonical form of z) only in c's orientation: c vs u' is z vs u', or
                                // rc(z) vs u' = z vs rc(u').  (k = 31 pseudo k-mers are not canonical values: the other pairing does occur.)
                                if (((f.second & 1u) != 0) != flip) continue;
                                if (f.first == z) { A.idx = 2u * id_of[f.second >> 1]; A.meta = 1u; member = true; break; }
                                const int pp = diff1(f.first, z);
                                if (pp < 0) continue;
                                const int jn = flip ? k - 1 - pp : pp;            // position in c (= in the neighbour's canonical form)
                                if (jn < tab.wstart || jn >= tab.wstart + tab.W || !((h_valid[f.second >> 1] >> (jn - tab.wstart)) & 1u)) continue;
                                const uint64_t key = ((uint64_t)jn << 32) | row_base[f.second >> 1];
                                jmask |= 1u << (jn - tab.wstart);
                                if (key < best) { best = key; best_fi = f.second; }
                            }
                            if (member || best == ~0ull) continue;
                            const uint32_t multi = (jmask & (jmask - 1u)) ? bk::kAnsMulti : 0u;
                            const int jn = (int)(best >> 32);
                            const uint32_t pnb = (uint32_t)best, ni = best_fi >> 1;
                            const uint32_t bc = (uint32_t)(c >> (2 * (k - 1 - jn))) & 3u;
                            if (pnb < tab.n_full) {
                                const uint32_t rcu = first_rc[ni] ? 1u : 0u;
                                const int oo = (rcu ? k - 1 - jn : jn) - tab.v_omin;
                                if (oo < 0 || oo >= tab.v_span) continue;            // (v_point's guard)
                                const uint32_t nbc = (uint32_t)(h_u[ni] >> (2 * (k - 1 - jn))) & 3u;   // the neighbour's own base there
                                A.idx = (uint32_t)(bk::v_row_base(pnb + (uint32_t)oo, bk::v_alt(bc, nbc), 0u, tab.v_span) + (uint32_t)oo);
                                A.meta = 2u | (rcu << 2) | ((oo + 1 < tab.v_span) ? 8u : 0u) | multi;
                            } else {
                                const uint32_t row = pnb - tab.n_full + (uint32_t)__builtin_popcount(h_valid[ni] & ((1u << (jn - tab.wstart)) - 1u));
                                A.idx = (uint32_t)(vreal + ((uint64_t)row * 4 + bc) * 2);
                                A.meta = 3u | multi;
                            }
                        }
                    }
                }
            });
            if (test_env("BK_VERIFY_ANSWERS")) {
                // testing build: every answer against the definition -- membership in U and the neighbour search spelled out
                // (all 3 W substitutions inside the window), no near lists involved
                std::atomic<uint64_t> bad{0};
                parallel_for(owners.size(), [&](size_t r0, size_t r1) {
                    for (size_t r = r0; r < r1; r++) {
                        const uint64_t u = h_u[owners[r]];
                        if (h_no_list[owners[r]]) continue;
                        for (int j = 0; j < k; j++) for (uint32_t bb = 0; bb < 4; bb++) {
                            const int sh = 2 * (k - 1 - j);
                            if (((u >> sh) & 3ull) == bb) continue;
                            const uint64_t z = (u & ~(3ull << sh)) | ((uint64_t)bb << sh), zr = bronko::reverse_complement_u64(z, k), c = zr < z ? zr : z;
                            bk::DirtyAns want{0u, 0u};
                            const auto it = std::lower_bound(h_u.begin(), h_u.end(), c);
                            if (it != h_u.end() && *it == c) { want.idx = 2u * id_of[it - h_u.begin()]; want.meta = 1u; }
                            else {
                                uint64_t best = ~0ull; size_t bi = 0; uint32_t jm = 0;
                                for (int jn = tab.wstart; jn < tab.wstart + tab.W; jn++) for (uint64_t alt = 0; alt < 4; alt++) {
                                    const int s2 = 2 * (k - 1 - jn);
                                    if (((c >> s2) & 3ull) == alt) continue;
                                    const uint64_t cand = (c & ~(3ull << s2)) | (alt << s2);
                                    const auto ct = std::lower_bound(h_u.begin(), h_u.end(), cand);
                                    if (ct == h_u.end() || *ct != cand) continue;
                                    const size_t ci = ct - h_u.begin();
                                    if (!((h_valid[ci] >> (jn - tab.wstart)) & 1u)) continue;
                                    const uint64_t key = ((uint64_t)jn << 32) | row_base[ci];
                                    jm |= 1u << (jn - tab.wstart);
                                    if (key < best) { best = key; bi = ci; }
                                }
                                const uint32_t multi = (jm & (jm - 1u)) ? bk::kAnsMulti : 0u;
                                if (best != ~0ull) {
                                    const int jn = (int)(best >> 32);
                                    const uint32_t pnb = (uint32_t)best, bc = (uint32_t)(c >> (2 * (k - 1 - jn))) & 3u;
                                    if (pnb < tab.n_full) {
                                        const uint32_t rcu = first_rc[bi] ? 1u : 0u;
                                        const int oo = (rcu ? k - 1 - jn : jn) - tab.v_omin;
                                        if (oo >= 0 && oo < tab.v_span) {
                                            const uint32_t nbc = (uint32_t)(h_u[bi] >> (2 * (k - 1 - jn))) & 3u;
                                            want.idx = (uint32_t)(bk::v_row_base(pnb + (uint32_t)oo, bk::v_alt(bc, nbc), 0u, tab.v_span) + (uint32_t)oo);
                                            want.meta = 2u | (rcu << 2) | ((oo + 1 < tab.v_span) ? 8u : 0u) | multi;
                                        }
                                    } else {
                                        want.idx = (uint32_t)(vreal + ((uint64_t)(pnb - tab.n_full + (uint32_t)__builtin_popcount(h_valid[bi] & ((1u << (jn - tab.wstart)) - 1u))) * 4 + bc) * 2);
                                        want.meta = 3u | multi;
                                    }
                                }
                            }
                            const bk::DirtyAns& got = ans_at(owners[r], j, bb);
                            if (got.idx != want.idx || got.meta != want.meta) {
                                if (bad++ < 5) fprintf(stderr, "[bk] dirty answer differs: id %u j %d bb %u: table (%u, %u) definition (%u, %u)\n", id_of[owners[r]], j, bb, got.idx, got.meta, want.idx, want.meta);
                            }
                        }
                    }
                });
                if (bad) return fail(BK_ERR_INVALID, "internal: %llu dirty answers disagree with their definition", (unsigned long long)bad.load());
            }
            // cell_nat (bk_device.h): per reference position q and alternative a, bit o = "the k-mer that starts at q - o, with
            // that other base at q, takes its own V row" -- its cell is clean, or its answer says exactly that (or says that it
            // touches nothing, which is what finalize makes of the own row's count then: position outside the window or
            // canonical form on the other strand)
            // Which id a bit promises: with touch lists (large planes: the scan notes touched rows per block of cells) the one
            // cell_blk gives, id = cell + block constant; otherwise whatever row most of the k-mers over q agree on --
            // cell_natrow[q] = id + o -- which also covers the cells whose ids leave the block's sequence (a later genome's own
            // k-mers around its differences from an earlier one)
            const bool lists = tab.W > 0 && (tab.plane_len >= (16ull << 20) || test_env("BK_SPARSE_FINALIZE") != nullptr);   // (= bk_engine::sparse, set later)
            h_nat.assign(((size_t)cells + (size_t)k) * 3u, 0u);
            if (!lists) h_natrow.assign((size_t)cells + (size_t)k, 0u);
            parallel_for((size_t)cells + (size_t)k, [&](size_t q0, size_t q1) {
                for (size_t q = q0; q < q1; q++) {
                    const uint32_t rb = q < cells ? (h_refw[pad_w + (q >> 4)] >> (2 * (q & 15))) & 3u : 0u;
                    uint32_t row = 0u;
                    if (!lists) {   // the most common id + o among the first-orientation cells q - o
                        uint32_t best_n = 0u;
                        for (int o = 0; o < k; o++) {
                            if (q < (size_t)o || q - (size_t)o >= cells) continue;
                            const size_t c = q - (size_t)o;
                            if (h_id_at[c] == kNone || !(h_cflags[c] & bk::kCellFirstOri)) continue;
                            const uint32_t r = h_id_at[c] + (uint32_t)o;
                            if (best_n && r == row) continue;
                            uint32_t n = 0u;
                            for (int o2 = o; o2 < k; o2++) {
                                if (q < (size_t)o2 || q - (size_t)o2 >= cells) continue;
                                const size_t c2 = q - (size_t)o2;
                                n += h_id_at[c2] != kNone && (h_cflags[c2] & bk::kCellFirstOri) && h_id_at[c2] + (uint32_t)o2 == r;
                            }
                            if (n > best_n) { best_n = n; row = r; }
                        }
                        h_natrow[q] = row;
                    }
                    for (int o = 0; o < k; o++) {
                        if (q < (size_t)o || q - (size_t)o >= cells) continue;
                        const size_t c = q - (size_t)o;
                        const uint32_t id = h_id_at[c];
                        if (id == kNone || !(h_cflags[c] & bk::kCellFirstOri)) continue;
                        if (lists ? id - (uint32_t)c != h_blk[c >> 6].x : id + (uint32_t)o != row) continue;
                        for (uint32_t al = 0; al < 3; al++) {
                            bool nat = (h_cflags[c] & bk::kCellClean) != 0;
                            if (!nat) {
                                const bk::DirtyAns& A = h_ans[bk::ans_index(id, (uint32_t)o, rb ^ (al + 1u), k)];
                                const uint32_t kind = A.meta & 3u;
                                const int oo = o - tab.v_omin;
                                if (A.meta & bk::kAnsNone) nat = false;
                                else if (kind == 0u) nat = true;
                                else if (kind == 2u && oo >= 0 && oo < tab.v_span)
                                    nat = A.idx == (uint32_t)(bk::v_row_base(id + (uint32_t)oo, al, 0u, tab.v_span) + (uint32_t)oo) && ((A.meta >> 2) & 1u) == rc_of_id[id];
                            }
                            if (nat) h_nat[q * 3u + al] |= 1u << o;
                        }
                    }
                }
            });
            BK_HIP(tab.dirty_ans.upload(h_ans));
            // Votes gathered cell by cell (bk_gather.hip) replace the walk over BucketInfo lists when a genome's BucketInfos ARE the
            // occurrences of its k-mers: every window bucket under one key (no two reference buckets merged by the k = 31 wrap),
            // holding each occurrence once and nothing else (an index built by `bronko build` does; a .bkdb from elsewhere might
            // not), every reference k-mer with a cell, and an answer for every dirty one
            bool all_listed = true, all_cells = true;
            for (uint32_t i : owners) if (h_no_list[i]) { all_listed = false; break; }
            for (size_t i = 0; i < h_u.size() && all_cells; i++) if (!h_is_pseudo[i] && first_cell[i] == kNone) all_cells = false;
            if (test_env("BK_L2_STATS") || test_env("BK_CREATE_TIMING"))
                fprintf(stderr, "[bk] gathered votes: answers for all %d, cells for all %d, merged buckets %llu, doubled BucketInfos %llu, window BucketInfos %llu for %llu occurrences x %d\n",
                        (int)all_listed, (int)all_cells, (unsigned long long)n_merged_buckets, (unsigned long long)n_dup_entries, (unsigned long long)n_window_entries,
                        (unsigned long long)n_occurrences, tab.W);
            tab.gather_ok = all_listed && all_cells && n_dup_entries == 0 && n_window_entries == n_occurrences * (uint64_t)tab.W &&
                           !test_env("BK_NO_GATHER");
        }
        std::vector<uint64_t>().swap(h_near);
    }
    pc.lap("dirty answers");
    return BK_OK;
}

int IndexBuilder::perfect_hash_and_uploads() {
    // perfect hash over U
    std::vector<uint16_t> h_pilots;
    std::vector<uint32_t> u_pos;
    if (!build_phf(h_u, h_pilots, tab.log2nb, tab.m, tab.log2p, u_pos)) return fail(BK_ERR_HIP, "internal error: perfect hash construction failed after every fallback");
    pc.lap("  perfect hash of U");
    std::vector<bk::KmerPos> t_pos((size_t)tab.m << tab.log2p, bk::KmerPos{bk::kEmptyKey, kNone, 0u});
    h_kmer_of.assign(std::max<size_t>(h_u.size(), 1), bk::kEmptyKey);
    for (size_t i = 0; i < h_u.size(); i++) {
        t_pos[u_pos[i]] = bk::KmerPos{h_u[i], first_cell[i], id_of[i] | (first_rc[i] ? 0x80000000u : 0u)};
        h_kmer_of[id_of[i]] = h_u[i];
    }
    BK_HIP(tab.pilots.upload(h_pilots));
    BK_HIP(tab.kmer_pos.upload(t_pos));
    BK_HIP(tab.kmer_of.upload(h_kmer_of));
    BK_HIP(tab.ref_words.upload(h_refw));
    BK_HIP(tab.cell_has.upload(h_has));
    BK_HIP(tab.cell_clean.upload(h_clean));
    BK_HIP(tab.cell_clean3.upload(h_clean3));
    BK_HIP(tab.cell_yf.upload(h_yf));
    BK_HIP(tab.cell_yr.upload(h_yr));
    BK_HIP(tab.cell_fast.upload(h_fast));
    BK_HIP(tab.cell_blk.upload(h_blk));
    if (!h_nat.empty()) BK_HIP(tab.cell_nat.upload(h_nat));
    if (!h_natrow.empty()) BK_HIP(tab.cell_natrow.upload(h_natrow));
    BK_HIP(tab.cell_codes.upload(h_codes));
    BK_HIP(tab.cell_flags.upload(h_cflags));
    BK_HIP(tab.id_at.upload(h_id_at));
    pc.lap("  tables of U filled, uploaded");
    tab.file_cell_lo.assign((size_t)ix->n_files, 0u);
    // (a file without sequences starts where the next file does, so that [file_cell_lo[f], file_cell_lo[f + 1]) is file f's cells
    // for every f: with `cells` in its place a file in front of it took every later file's cells as its own, and its own range
    // came out negative -- seed_tables() then looked for a power of two above 2^64 - n and never returned)
    uint64_t next_lo = cells;
    for (int f = ix->n_files - 1; f >= 0; f--) {
        if (ix->n_seqs[f]) next_lo = cell_off[f][0];
        tab.file_cell_lo[f] = (uint32_t)next_lo;
    }
    return BK_OK;
}

int IndexBuilder::seed_tables() {
    // the scan's seed tables (bk_device.h seed_hash): per genome file, where each of its reference k-mers starts
    if (cells > 0 && cells < (1ull << bk::kSeedCellBits) && tab.n_full > 0) {
        uint64_t max_file_cells = 1;
        for (int f = 0; f < ix->n_files; f++) tab.max_file_cells_idx = std::max<uint64_t>(tab.max_file_cells_idx, (f + 1 < ix->n_files ? tab.file_cell_lo[f + 1] : cells) - tab.file_cell_lo[f]);
        for (int f = 0; f < ix->n_files; f++)
            max_file_cells = std::max<uint64_t>(max_file_cells, (f + 1 < ix->n_files ? tab.file_cell_lo[f + 1] : cells) - tab.file_cell_lo[f]);
        uint32_t L = 6;
        while ((1ull << L) < max_file_cells) L++;
        if (((uint64_t)ix->n_files << L) * sizeof(uint2) <= (8ull << 30)) {
            tab.seed_log2 = L;
            std::vector<uint2> h_seed((size_t)ix->n_files << L, make_uint2(0xffffffffu, 0xffffffffu));
            parallel_for((size_t)ix->n_files, [&](size_t f0, size_t f1) {
                for (size_t f = f0; f < f1; f++) {
                    const uint64_t c_lo = tab.file_cell_lo[f], c_hi = f + 1 < (size_t)ix->n_files ? tab.file_cell_lo[f + 1] : cells;
                    for (uint64_t c = c_lo; c < c_hi; c++) {
                        const uint32_t id = h_id_at[c];
                        if (id == kNone || id >= tab.n_full) continue;
                        const uint32_t h = bk::seed_hash(h_kmer_of[id]);
                        const uint32_t ent = (uint32_t)c | (((h_brc[c >> 5] >> (c & 31)) & 1u) << bk::kSeedCellBits) | ((h & 15u) << 28);
                        uint2& b = h_seed[(f << L) + (h >> (32 - L))];
                        auto same = [&](uint32_t o) { return o != 0xffffffffu && h_id_at[o & ((1u << bk::kSeedCellBits) - 1u)] == id; };   // (a repeat: one entry does)
                        if (same(b.x) || same(b.y)) continue;
                        if (b.x == 0xffffffffu) b.x = ent; else if (b.y == 0xffffffffu) b.y = ent;   // (else: not in the table)
                    }
                }
            });
            BK_HIP(tab.seed_tab.upload(h_seed));
        }
        // ... and, for the binned scan, the reference reverse-complemented (symbol J = complement of symbol cells - 1 - J, same
        // paddings) with seed tables keyed by the k-mer AS A READ SHOWS IT -- bases in reading order, 2 bits each from bit 0 -- on
        // either strand: two entries per reference k-mer (along the reference: strand 0; against it: strand 1), four times the
        // buckets (a k-mer that finds its bucket full is no seed: 9% of them at twice the buckets, 3% at four times -- every
        // lost seed is a second round of seeds for its tile).  A read's k-mer is hashed as it stands -- no reverse complement, no canonical form -- and verified against the
        // reference (strand 0) or its reverse complement (strand 1) with one comparison.
        if (((uint64_t)ix->n_files << (L + 2)) * sizeof(uint2) <= (8ull << 30) && cells >= (uint64_t)k) {
            std::vector<uint32_t> h_rcw(h_refw.size() + 1, 0u);   // (+ 1: a window's slice starts inside a word, scan_items_kernel stages one word more)
            parallel_for((size_t)((cells + 15) / 16), [&](size_t w0, size_t w1) {
                for (size_t w = w0; w < w1; w++) {
                    uint32_t acc = 0;
                    for (uint64_t J = (uint64_t)w * 16; J < std::min<uint64_t>((uint64_t)w * 16 + 16, cells); J++) {
                        const uint64_t c = cells - 1 - J;
                        acc |= (3u - ((h_refw[pad_w + (c >> 4)] >> (2 * (c & 15))) & 3u)) << (2 * (J & 15));
                    }
                    h_rcw[pad_w + w] = acc;
                }
            });
            auto syms = [&](const std::vector<uint32_t>& a, uint64_t pos) -> uint64_t {   // k symbols from symbol `pos`, the first at bit 0
                uint64_t g = 0;
                for (int t = 0; t < k; t++) g |= (uint64_t)((a[pad_w + ((pos + t) >> 4)] >> (2 * ((pos + t) & 15))) & 3u) << (2 * t);
                return g;
            };
            const uint32_t L2 = L + 2;
            tab.seed2_log2 = L2;
            std::vector<uint2> h_seed2((size_t)ix->n_files << L2, make_uint2(0xffffffffu, 0xffffffffu));
            // Only the k-mers that start at ONE cell of their genome file are seeds: a repeat's entry would name one of its cells
            // for a read from any of them -- a diagonal that passes the verification (the k-mer is there) and is wrong; the scan
            // would then see a read of mismatches, all of them Level 2's to sort out.  Reads in repeats have other seeds.
            parallel_for((size_t)ix->n_files, [&](size_t f0, size_t f1) {
                std::vector<uint8_t> seen(tab.n_full, 0);   // per worker: occurrences of each id in the file at hand (saturating at 2)
                for (size_t f = f0; f < f1; f++) {
                    const uint64_t c_lo = tab.file_cell_lo[f], c_hi = f + 1 < (size_t)ix->n_files ? tab.file_cell_lo[f + 1] : cells;
                    for (uint64_t c = c_lo; c < c_hi; c++) {
                        const uint32_t id = h_id_at[c];
                        if (id != kNone && id < tab.n_full && seen[id] < 2) seen[id]++;
                    }
                    for (uint64_t c = c_lo; c < c_hi; c++) {
                        const uint32_t id = h_id_at[c];
                        if (id == kNone || id >= tab.n_full || seen[id] != 1) continue;
                        for (uint32_t strand = 0; strand < 2u; strand++) {
                            const uint64_t g = strand ? syms(h_rcw, cells - (uint64_t)k - c) : syms(h_refw, c);
                            const uint32_t h = bk::seed_hash(g);
                            const uint32_t ent = (uint32_t)c | (strand << bk::kSeedCellBits) | ((h & 15u) << 28);
                            uint2& b = h_seed2[(f << L2) + (h >> (32 - L2))];
                            if (b.x == 0xffffffffu) b.x = ent; else if (b.y == 0xffffffffu) b.y = ent;   // (else: not in the table)
                        }
                    }
                    for (uint64_t c = c_lo; c < c_hi; c++) {   // (back to zero for the worker's next file: the cells, not the whole array)
                        const uint32_t id = h_id_at[c];
                        if (id != kNone && id < tab.n_full) seen[id] = 0;
                    }
                }
            });
            BK_HIP(tab.rc_words.upload(h_rcw));
            BK_HIP(tab.seed_tab2.upload(h_seed2));
        }
    }
    return BK_OK;
}

int IndexBuilder::genome_occurrences() {
    // (round 6: up to 2^31 entries -- 8 GB of the 288 --: 250 strains are 0.47 G; at 2^28 the window stayed on the first genome
    // and every strain difference of a sample went to Level 2)
    if (ix->n_files > 1 && (uint64_t)tab.n_full * (uint64_t)ix->n_files <= (1ull << 31)) {
        std::vector<uint32_t> h_occ((size_t)tab.n_full * ix->n_files, 0xffffffffu);
        for (int f = 0; f < ix->n_files; f++) {
            const uint64_t c_lo = tab.file_cell_lo[f], c_hi = f + 1 < ix->n_files ? tab.file_cell_lo[f + 1] : cells;
            for (uint64_t c = c_lo; c < c_hi; c++) {
                const uint32_t id = h_id_at[c];
                if (id == kNone || id >= tab.n_full) continue;
                uint32_t& o = h_occ[(size_t)id * ix->n_files + f];
                if (o == 0xffffffffu) o = (uint32_t)c | (((h_brc[c >> 5] >> (c & 31)) & 1u) << 31);
            }
        }
        BK_HIP(tab.occ.upload(h_occ));
        BK_HIP(tab.file_cell_lo_d.upload(tab.file_cell_lo));
    }
    {
        std::vector<uint8_t> h_amb2(h_amb);
        for (size_t id = 0; id < h_amb2.size(); id++) h_amb2[id] = (h_amb[id] ? 1 : 0) | (rc_of_id[id] ? 2 : 0);
        BK_HIP(tab.amb.upload(h_amb2));
    }

    pc.lap("perfect hash of U + uploads");
    return BK_OK;
}

int IndexBuilder::half_key_directories() {
    // half-key directories (neighbour search)
    const int lo_bits = 2 * tab.lo_bases;
    const uint64_t lo_mask = (1ull << lo_bits) - 1ull;
    {
        // both halves at once (host threads); the low half needs a sort of its own, the high half is h_u's order
        struct HalfHost { std::vector<uint16_t> hp; std::vector<bk::HalfDir> dir; std::vector<bk::NbEntry> cand; std::vector<uint32_t> bits; bool ok = true; };
        HalfHost hh[2];
        auto build_half = [&](int which) {
            auto half_of = [&](uint64_t u) { return which == 0 ? (u & lo_mask) : (u >> lo_bits); };
            PhaseClock hc;
            hc.on = hc.on && which == 0;
            std::vector<uint32_t> order(h_u.size());
            for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
            if (which == 0) {
                // by low half, then by value (= by high half): one radix sort on the device of the k-mers with their halves swapped
                // (an indirect std::sort on 32 host threads was 1.5 s of a 100-strain create); which == 1: h_u is sorted by value,
                // hence by its high half, then by value
                bool on_device = false;
                if (order.size() >= (1u << 16) && hipSetDevice(prm->device) == hipSuccess) {
                    const int hi_bits = 2 * k - lo_bits;
                    std::vector<unsigned long long> keys(h_u.size());
                    parallel_for(h_u.size(), [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; i++) keys[i] = ((h_u[i] & lo_mask) << hi_bits) | (h_u[i] >> lo_bits); });
                    on_device = bk::device_sort_order(keys.data(), keys.size(), 2 * k, order.data(), nullptr) == hipSuccess;
                }
                if (!on_device)
                    parallel_sort(order, [&](uint32_t x, uint32_t y) {
                        const uint64_t hx = half_of(h_u[x]), hy = half_of(h_u[y]);
                        return hx != hy ? hx < hy : h_u[x] < h_u[y];
                    }, sort_threads);
            }
            hc.lap("  half 0: order sorted");
            std::vector<bk::NbEntry>& cand = hh[which].cand;
            cand.resize(order.size());
            parallel_for(order.size(), [&](size_t i0, size_t i1) {   // (the gather through `order` is what costs: host threads)
                for (size_t i = i0; i < i1; i++)
                    cand[i] = bk::NbEntry{h_u[order[i]], row_base[order[i]], (h_valid[order[i]] & 0x7fffffffu) | (first_rc[order[i]] ? 0x80000000u : 0u)};
            });
            std::vector<uint64_t> halves;
            std::vector<uint32_t> first, count;
            for (size_t i = 0; i < order.size(); i++) {
                const uint64_t hf = half_of(cand[i].u);
                if (halves.empty() || halves.back() != hf) { halves.push_back(hf); first.push_back((uint32_t)i); count.push_back(0); }
                count.back()++;
            }
            hc.lap("  half 0: candidates gathered, halves listed");
            IndexTables::HalfBufs& hb = which == 0 ? tab.half_lo : tab.half_hi;
            {   // the presence filter of this half (bk_device.h HalfView::bits): exact up to 24 bits, hashed above (16 bits per half-key: 6 % false "present")
                const int half_bits = which == 0 ? lo_bits : 2 * k - lo_bits;
                hb.bits_exact = half_bits <= 24 ? 1u : 0u;
                uint32_t l2 = (uint32_t)half_bits;
                if (!hb.bits_exact) { l2 = 16; while (l2 < 28 && (1ull << l2) < 16ull * halves.size()) l2++; }
                hb.bits_log2 = std::max<uint32_t>(l2, 5);
                hh[which].bits.assign((size_t)1 << (hb.bits_log2 - 5), 0u);
                for (uint64_t hf : halves) { const uint32_t b = bk::half_bit_index(hf, hb.bits_log2, hb.bits_exact); hh[which].bits[b >> 5] |= 1u << (b & 31u); }
            }
            std::vector<uint32_t> hpos;
            if (!build_phf(halves, hh[which].hp, hb.log2nb, hb.m, hb.log2p, hpos)) { hh[which].ok = false; return; }
            hh[which].dir.assign((size_t)hb.m << hb.log2p, bk::HalfDir{0u, 0u, 0u, 0u});
            hc.lap("  half 0: perfect hash");
            for (size_t i = 0; i < halves.size(); i++) hh[which].dir[hpos[i]] = bk::HalfDir{(uint32_t)halves[i], first[i], count[i], 0u};
            hc.lap("  half 0: directory");
        };
        std::thread t0(build_half, 0);
        build_half(1);
        t0.join();
        pc.lap("  halves built");
        for (int which = 0; which < 2; which++) {
            if (!hh[which].ok) return fail(BK_ERR_HIP, "internal error: perfect hash construction failed after every fallback");
            IndexTables::HalfBufs& hb = which == 0 ? tab.half_lo : tab.half_hi;
            BK_HIP(hb.pilots.upload(hh[which].hp));
            BK_HIP(hb.dir.upload(hh[which].dir));
            BK_HIP(hb.cand.upload(hh[which].cand));
            BK_HIP(hb.bits.upload(hh[which].bits));
        }
    }

    pc.lap("half-key directories");
    return BK_OK;
}

int IndexBuilder::slot_of() {
    // slot_of[id*W + t]: the window bucket (wstart+t, u masked) of reference k-mer id -- every reference k-mer
    // owns all of its buckets, so finalize needs no table probe for them (pseudo k-mers: empty_slot where none).
    if (slots_on_device) {   // laid out by id on the device, where the table stays; the host phases below read a copy
        BK_HIP(tab.slot_of.alloc(h_u.size() * (size_t)tab.W));
        BK_HIP(bk::device_permute_rows(d_slot_by_index.p, id_of.data(), h_u.size(), tab.W, tab.slot_of.p));
        BK_HIP(d_slot_by_index.alloc(0));   // (freed)
        h_slot_of = HostVec<uint32_t>(h_u.size() * (size_t)tab.W);
        BK_HIP(hipMemcpy(h_slot_of.data(), tab.slot_of.p, h_slot_of.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    } else {
    h_slot_of = filled((size_t)std::max<size_t>(h_u.size(), 1) * std::max(tab.W, 1), empty_slot);
    parallel_for(h_u.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++)
            for (int t = 0; t < tab.W; t++) h_slot_of[(size_t)id_of[i] * tab.W + t] = slot_by_index[i * tab.W + t];
    });
    HostVec<uint32_t>().swap(slot_by_index);
    BK_HIP(tab.slot_of.upload(h_slot_of));
    }
    pc.lap("  slot_of filled, uploaded");
    return BK_OK;
}

int IndexBuilder::slot_rec() {
    {
        std::vector<uint8_t> h_all_own, h_own_mirror;   // by id (file bitmaps only)
        std::vector<bk::SlotRec> h_rec((size_t)std::max<size_t>(tab.n_full, 1) * std::max(tab.W, 1));
        parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
            for (size_t id = id0; id < id1; id++)
                for (int t = 0; t < tab.W; t++) {
                    const uint32_t sl = h_slot_of[id * tab.W + t];
                    bk::SlotRec r{};
                    r.off = h_off[sl]; r.len = h_len[sl];
                    if (r.len) r.first = h_ent[r.off];
                    h_rec[id * tab.W + t] = r;
                }
        });
        BK_HIP(tab.slot_rec.upload(h_rec));
        pc.lap("  slot_rec");
        // Which genome files a bucket holds, as a bitmap (IndexView::ent_files / slot_files): with up to 128 files, for buckets
        // that hold at most one BucketInfo per file -- the rule with many related genomes.  The statistics pass of
        // pileup_selected_only then tallies a k-mer's genomes without reading its ~100 entries, and the voting pass finds the
        // selected genome's entry by a popcount instead of a bisection.  All zero = look at the entries.
        if (ix->n_files > 1 && ix->n_files <= 128 && tab.W > 1 && !h_len.empty()) {
            std::vector<uint4> h_ef(h_len.size(), make_uint4(0u, 0u, 0u, 0u));
            parallel_for(h_len.size(), [&](size_t s0, size_t s1) {
                for (size_t sl = s0; sl < s1; sl++) {
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    bool ok = h_len[sl] > 0;
                    for (uint32_t q = 0; q < h_len[sl] && ok; q++) {
                        const uint32_t f = h_ent[h_off[sl] + q].file;
                        ok = f < 128u && (q == 0 || f > h_ent[h_off[sl] + q - 1].file);   // sorted by file, one entry each
                        w[(f >> 5) & 3u] |= 1u << (f & 31u);
                    }
                    if (ok) h_ef[sl] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            });
            std::vector<uint4> h_sf((size_t)std::max<size_t>(tab.n_full, 1) * tab.W, make_uint4(0u, 0u, 0u, 0u));
            parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
                for (size_t id = id0; id < id1; id++)
                    for (int t = 0; t < tab.W; t++) {
                        const uint32_t sl = h_slot_of[id * tab.W + t];
                        if (sl != empty_slot) h_sf[id * tab.W + t] = h_ef[sl];
                    }
            });
            BK_HIP(tab.ent_files.upload(h_ef));
            BK_HIP(tab.slot_files.upload(h_sf));
            pc.lap("  file bitmaps");
            // id_own_files (IndexView): bit f of id = in every one of the k-mer's W buckets genome f's only BucketInfo is the k-mer's
            // own occurrence in f -- cell, idx and orientation of bucket t are those of bucket 0, t further on.  The voting pass
            // for the selected genome then needs bucket 0 alone (one load shared by the W lanes of a counter).
            std::vector<uint4> h_own(std::max<size_t>(tab.n_full, 1), make_uint4(0u, 0u, 0u, 0u));
            h_own_mirror.assign(tab.n_full, 0);
            parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
                for (size_t id = id0; id < id1; id++) {
                    const uint32_t s0 = h_slot_of[id * tab.W];
                    if (s0 == empty_slot || !bk::files_any(h_ef[s0])) continue;
                    // along the reference or against it (an occurrence that was reverse-complemented to become canonical): bucket
                    // t's BucketInfo is bucket 0's with cell and idx t further on, or t further back -- one direction per k-mer,
                    // that of its first genome's entries
                    const int dir = h_ent[h_off[s0]].idx == (uint8_t)tab.wstart ? 1 : -1;
                    const int idx0 = dir > 0 ? tab.wstart : k - 1 - tab.wstart;
                    uint32_t w[4] = {h_ef[s0].x, h_ef[s0].y, h_ef[s0].z, h_ef[s0].w};
                    for (uint32_t q0 = 0; q0 < h_len[s0]; q0++) {   // bucket 0's BucketInfo of f is the occurrence of this very k-mer at cell - idx
                        const bk::DevEntry& a0 = h_ent[h_off[s0] + q0];
                        const bool ok = a0.idx == (uint8_t)idx0 && a0.cell >= (uint32_t)idx0 && a0.cell - (uint32_t)idx0 < cells &&
                                        h_id_at[a0.cell - (uint32_t)idx0] == (uint32_t)id;
                        if (!ok) w[(a0.file >> 5) & 3u] &= ~(1u << (a0.file & 31u));
                    }
                    for (int t = 1; t < tab.W; t++) {
                        const uint32_t st = h_slot_of[id * tab.W + t];
                        if (st == empty_slot || !bk::files_any(h_ef[st])) { w[0] = w[1] = w[2] = w[3] = 0u; break; }
                        w[0] &= h_ef[st].x; w[1] &= h_ef[st].y; w[2] &= h_ef[st].z; w[3] &= h_ef[st].w;
                        // both lists hold one entry per file, sorted: walk them together
                        uint32_t q0 = 0, qt = 0;
                        const uint32_t n0 = h_len[s0], nt_ = h_len[st];
                        while (q0 < n0 && qt < nt_) {
                            const bk::DevEntry& a0 = h_ent[h_off[s0] + q0];
                            const bk::DevEntry& at = h_ent[h_off[st] + qt];
                            if (a0.file < at.file) { ++q0; continue; }
                            if (at.file < a0.file) { ++qt; continue; }
                            if (at.cell != a0.cell + (uint32_t)(dir * t) || at.idx != (uint8_t)(a0.idx + dir * t) || at.canonical != a0.canonical)
                                w[(a0.file >> 5) & 3u] &= ~(1u << (a0.file & 31u));
                            ++q0; ++qt;
                        }
                    }
                    h_own[id] = make_uint4(w[0], w[1], w[2], w[3]);
                    h_own_mirror[id] = dir < 0 ? 1 : 0;
                }
            });
            BK_HIP(tab.id_own_files.upload(h_own));
            pc.lap("  own files");
            if (test_env("BK_L2_STATS")) {
                uint64_t n_own = 0, n_b0 = 0, n_mir = 0, n_any = 0;
                auto pc4 = [](const uint4& b) { return (uint64_t)(__builtin_popcount(b.x) + __builtin_popcount(b.y) + __builtin_popcount(b.z) + __builtin_popcount(b.w)); };
                for (size_t id = 0; id < tab.n_full; id++) {
                    n_own += pc4(h_own[id]); n_any += bk::files_any(h_own[id]); n_mir += h_own_mirror[id];
                    const uint32_t s0 = h_slot_of[id * tab.W];
                    if (s0 != empty_slot) n_b0 += h_len[s0];
                }
                fprintf(stderr, "[bk] own files: %llu (k-mer, genome) pairs of %llu in bucket 0; %llu of %llu k-mers with any, %llu against the reference\n",
                        (unsigned long long)n_own, (unsigned long long)n_b0, (unsigned long long)n_any, (unsigned long long)tab.n_full, (unsigned long long)n_mir);
            }
            // id_rest (IndexView): per k-mer, the BucketInfos of its W buckets that are NOT its own occurrences -- other k-mers of
            // other genomes that differ at the bucket's position -- as indices into `entries`; what every-genome votes have
            // left to do for a k-mer after finalize_exact_own_kernel.  (k-mers without file bitmaps: no list, own is all zero.)
            {
                std::vector<uint32_t> h_roff((size_t)tab.n_full + 1, 0u);
                parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
                    for (size_t id = id0; id < id1; id++) {
                        uint32_t n = 0;
                        if (bk::files_any(h_own[id]))
                            for (int t = 0; t < tab.W; t++) {
                                const uint4& f = h_sf[id * tab.W + t];
                                n += (uint32_t)(__builtin_popcount(f.x & ~h_own[id].x) + __builtin_popcount(f.y & ~h_own[id].y) + __builtin_popcount(f.z & ~h_own[id].z) + __builtin_popcount(f.w & ~h_own[id].w));
                            }
                        h_roff[id + 1] = n;
                    }
                });
                for (size_t id = 0; id < tab.n_full; id++) h_roff[id + 1] += h_roff[id];
                std::vector<uint32_t> h_rest(std::max<size_t>(h_roff[tab.n_full], 1), 0u);
                parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
                    for (size_t id = id0; id < id1; id++) {
                        if (!bk::files_any(h_own[id])) continue;
                        uint32_t at = h_roff[id];
                        for (int t = 0; t < tab.W; t++) {
                            const uint32_t sl = h_slot_of[id * tab.W + t];
                            for (uint32_t q = 0; q < h_len[sl]; q++)
                                if (!bk::files_has(h_own[id], h_ent[h_off[sl] + q].file)) h_rest[at++] = h_off[sl] + q;
                        }
                    }
                });
                BK_HIP(tab.id_rest_off.upload(h_roff));
                BK_HIP(tab.id_rest.upload(h_rest));
                pc.lap("  rest lists");
            }
            // kIdAllOwn: nothing else in any of the k-mer's buckets
            h_all_own.assign(tab.n_full, 0);
            parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
                for (size_t id = id0; id < id1; id++) {
                    bool all = bk::files_any(h_own[id]);
                    for (int t = 0; t < tab.W && all; t++) {
                        const uint4& f = h_sf[id * tab.W + t];
                        all = f.x == h_own[id].x && f.y == h_own[id].y && f.z == h_own[id].z && f.w == h_own[id].w;
                    }
                    h_all_own[id] = all ? 1 : 0;
                }
            });
        }
        // (which genome file a cell belongs to.  Round 6: for any number of genome files -- the gathered votes of bk_gather.hip need
        // no file bitmap, and with more than 128 files, where there is none, they are what keeps every genome's rows affordable:
        // 250 strains, 68 ms a sample through the BucketInfo lists)
        if (ix->n_files > 1 && ix->n_files <= 65535 && tab.W > 1 && !h_len.empty()) {
            std::vector<uint16_t> h_cf(std::max<uint64_t>(cells, 1), 0);
            size_t sq2 = 0;
            for (int f = 0; f < ix->n_files; f++)
                for (int s2 = 0; s2 < ix->n_seqs[f]; s2++, sq2++) {
                    const uint64_t lo = cell_off[f][s2], hi = lo + ix->seq_lens[sq2];
                    for (uint64_t c = lo; c < hi && c < cells; c++) h_cf[c] = (uint16_t)f;
                }
            BK_HIP(tab.cell_file.upload(h_cf));
        }
        // IdRec: k-mer, first cell, flags; "simple" = each of the W buckets holds the k-mer's own single occurrence and nothing else
        HostVec<bk::IdRec> h_idrec = filled(std::max<size_t>(h_u.size(), 1), bk::IdRec{bk::kEmptyKey, 0u, 0u});
        parallel_for(h_u.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const uint32_t id = id_of[i];
            bk::IdRec r{h_u[i], first_cell[i] == kNone ? 0u : first_cell[i], (h_amb[id] ? bk::kIdDirty : 0u) | (first_rc[i] ? bk::kIdRc : 0u)};
            if (id < tab.n_full && first_cell[i] != kNone && tab.W > 0) {
                bool simple = true;
                for (int t = 0; t < tab.W && simple; t++) {
                    const bk::SlotRec& sr = h_rec[(size_t)id * tab.W + t];
                    simple = sr.len == 1 && sr.first.cell == first_cell[i] + (uint32_t)(tab.wstart + t) && sr.first.idx == (uint8_t)(tab.wstart + t) &&
                             sr.first.canonical == (first_rc[i] ? 1 : 0);
                }
                if (simple) r.flags |= bk::kIdSimple | ((uint32_t)h_rec[(size_t)id * tab.W].first.file << 16);
            }
            if (id < h_all_own.size() && h_all_own[id]) r.flags |= bk::kIdAllOwn;
            if (id < h_own_mirror.size() && h_own_mirror[id]) r.flags |= bk::kIdOwnMirror;
            h_idrec[id] = r;
        }
        });
        BK_HIP(tab.id_rec.upload(h_idrec));
    }

    pc.lap("slot_of + slot_rec");
    return BK_OK;
}

int IndexBuilder::estat() {
    // estat: per reference k-mer, its per-genome hit totals over its W window buckets (call.rs:1316-1318) and
    // hence perfect (== W) / variant -- a property of the index alone
    std::vector<uint32_t> h_estat_off(h_u.size() + 1, 0u), h_estat;
    {
        // per id, independently: chunks on host threads, each with its own list, joined in id order
        const size_t n_ids = h_u.size();
        const unsigned nt = n_ids < 65536 ? 1u : std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 256u);
        // (the reference k-mers -- ids below n_full, each with W buckets of ~70 BucketInfos -- and the pseudo k-mers -- twenty times as
        // many, nearly nothing each -- are cut into nt chunks EACH: a thread takes one of either kind.  Cut as one range, the first
        // twentieth of the threads did all the work.)
        const size_t n_real = std::min<size_t>(tab.n_full, n_ids);
        auto cut = [&](unsigned c) -> size_t { return c <= nt ? n_real * c / nt : n_real + (n_ids - n_real) * (c - nt) / nt; };   // chunk c = [cut(c), cut(c + 1)), c < 2 nt
        std::vector<std::vector<uint32_t>> part(2 * nt);
        std::vector<uint32_t> n_of(n_ids, 0u);
        auto work = [&](unsigned t) {
            std::vector<uint32_t> hits(tab.n_files, 0u), touched;
            for (unsigned c : {t, nt + t})
            for (size_t id = cut(c); id < cut(c + 1); id++) {
                touched.clear();
                for (int w = 0; w < tab.W; w++) {
                    const uint32_t sl = h_slot_of[id * tab.W + w];
                    for (uint32_t q = 0; q < h_len[sl]; q++) {
                        const uint32_t file = h_ent[h_off[sl] + q].file;
                        if (hits[file]++ == 0) touched.push_back(file);
                    }
                }
                for (uint32_t file : touched) {
                    part[c].push_back((file << 1) | (hits[file] == (uint32_t)tab.W ? 1u : 0u));
                    hits[file] = 0;
                }
                n_of[id] = (uint32_t)touched.size();
            }
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t);
        work(0);
        for (auto& t : th) t.join();
        for (size_t id = 0; id < n_ids; id++) h_estat_off[id + 1] = h_estat_off[id] + n_of[id];
        h_estat.resize(h_estat_off[n_ids]);
        {   // the chunks' lists back to back (chunk t starts where its first id's list starts), copied side by side
            std::vector<std::thread> cp;
            for (unsigned t = 0; t < nt; t++) cp.emplace_back([&, t] {
                for (unsigned c : {t, nt + t}) { if (!part[c].empty()) std::copy(part[c].begin(), part[c].end(), h_estat.begin() + (ptrdiff_t)h_estat_off[cut(c)]); std::vector<uint32_t>().swap(part[c]); }
            });
            for (auto& t : cp) t.join();
        }
    }
    BK_HIP(tab.estat_off.upload(h_estat_off));
    BK_HIP(tab.estat.upload(h_estat));
    if (tab.n_files > 1 && tab.n_files <= 128 && tab.W > 1 && tab.n_full > 0) {
        // the same as two bitmaps per reference k-mer (IndexView::estat_files): genomes in which it is perfect, ... a variant
        std::vector<uint4> h_esf((size_t)tab.n_full * 2, make_uint4(0u, 0u, 0u, 0u));
        parallel_for(tab.n_full, [&](size_t id0, size_t id1) {
            for (size_t id = id0; id < id1; id++)
                for (uint32_t q = h_estat_off[id]; q < h_estat_off[id + 1]; q++) {
                    const uint32_t f = h_estat[q] >> 1;
                    uint4& b = h_esf[id * 2 + ((h_estat[q] & 1u) ? 0 : 1)];
                    (f < 32u ? b.x : f < 64u ? b.y : f < 96u ? b.z : b.w) |= 1u << (f & 31u);
                }
        });
        BK_HIP(tab.estat_files.upload(h_esf));
    }
    return BK_OK;
}

int IndexBuilder::lds_policy() {
    hipDeviceProp_t prop;
    BK_HIP(hipGetDeviceProperties(&prop, prm->device));
    tab.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const size_t budget = bk::scan_lds_budget();
    // LDS holds, for the first n_lds_bins cells (the first genome(s) of the index): the difference array (4 B per cell) and
    // Level 1's copies of the per-cell arrays (2 + 1 bits per cell).  As many cells as fit.
    tab.ref_in_lds = true;
    if (const char* rl = test_env("BK_REF_IN_LDS")) tab.ref_in_lds = atoi(rl) != 0;
    uint64_t nb = std::min<uint64_t>(tab.total_cells, budget / sizeof(unsigned int));
    if (tab.ref_in_lds) {
        nb = std::min<uint64_t>(tab.total_cells, budget * 32 / 141);   // 4 + 1/4 + 1/8 + 1/32 bytes per cell ...
        while (nb > 0 && nb * sizeof(unsigned int) + bk::scan_ref_lds_bytes((uint32_t)nb) > budget) nb -= std::min<uint64_t>(nb, 64);   // ... and the paddings
    }
    tab.n_lds_bins = (uint32_t)nb;
    if (const char* nl = test_env("BK_LDS_BINS")) tab.n_lds_bins = std::min<uint32_t>(tab.n_lds_bins, (uint32_t)atol(nl));
    if (tab.n_lds_bins < tab.total_cells) tab.n_lds_bins &= ~63u;   // (a window is a whole number of 64-cell blocks unless it holds everything)
    pc.lap("estat + LDS policy");
    return BK_OK;
}

int IndexBuilder::table_uploads() {
    if (bk::finalize_lds_bytes(tab.n_files) > 160 * 1024) return fail(BK_ERR_UNSUPPORTED, "more than ~8000 genome files are not supported by the finalize kernel");

    if (!tab.table.p) BK_HIP(tab.table.upload(h_table));
    {
        bool any = false;
        std::vector<uint32_t> bits(h_slot_alias.size() / 32 + 2, 0u);
        for (size_t sl = 0; sl < h_slot_alias.size(); sl++) if (h_slot_alias[sl]) { bits[sl >> 5] |= 1u << (sl & 31); any = true; }
        if (any) BK_HIP(tab.slot_alias.upload(bits));
        // the merged buckets' window slots: slot, window position and key of each (bk_gather.hip merged_votes_kernel)
        std::vector<uint64_t> mg;
        for (uint32_t sl : h_merged_slots) { mg.push_back(((uint64_t)h_slot_t[sl] << 32) | sl); mg.push_back(h_slot_key[sl]); }
        tab.n_merged_slots = (uint32_t)h_merged_slots.size();
        if (!mg.empty()) BK_HIP(tab.merged_slots.upload(mg));
    }
    BK_HIP(tab.ent_off.upload(h_off));
    BK_HIP(tab.ent_len.upload(h_len));
    BK_HIP(tab.entries.upload(h_ent));
    if (const char* ab = test_env("BK_SCAN_ABLATE")) tab.ablate = atoi(ab);
    if (const char* vm = test_env("BK_ITEM_V_MODE")) tab.item_v_mode = atoi(vm);
    if (const char* ml = test_env("BK_MAX_LAUNCH_RECORDS")) tab.max_launch_records = strtoull(ml, nullptr, 10);
    return BK_OK;
}

}  // namespace

int build_index_tables(const bk_index_desc* ix, const bk_params* prm, IndexTables& tab, PhaseClock& pc) {
    IndexBuilder b(ix, prm, tab, pc);
    if (int rc = b.sequence_geometry()) return rc;
    pc = PhaseClock();   // (the laps start after the sequence geometry)
    for (auto stage : {&IndexBuilder::buckets_to_slots, &IndexBuilder::window_tables, &IndexBuilder::reference_set, &IndexBuilder::reference_walk,
                       &IndexBuilder::dirty_flags, &IndexBuilder::cell_arrays, &IndexBuilder::dirty_answers, &IndexBuilder::perfect_hash_and_uploads,
                       &IndexBuilder::seed_tables, &IndexBuilder::genome_occurrences, &IndexBuilder::half_key_directories, &IndexBuilder::slot_of,
                       &IndexBuilder::slot_rec, &IndexBuilder::estat, &IndexBuilder::lds_policy, &IndexBuilder::table_uploads})
        if (int rc = (b.*stage)()) return rc;
    return BK_OK;
}
