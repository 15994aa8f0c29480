// bk_engine.cpp -- host side of the C ABI declared in include/bronko_hip.h: the engine's life and the sample path.
//
// Owns the HBM buffers of a sample (counter planes, pileups) and sequences the kernels of bk_kernels.hip on one HIP stream, from the
// scan of a batch of records (push_device) to the pileup's download; the index tables an engine reads are built by bk_index_tables.cpp
// and shared with its forks; how a caller's reads become records (the bk_push_reads_* entry points, K0, the trimming stage) is
// bk_ingest.cpp; the passes that ride behind every scan (k-mer dump, indels, linkage) are bk_riders.cpp, the reports made of the pileup
// (calls, consensus, regions) bk_reports.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "bk_engine.h"

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// everything a sample writes (counter planes, scan scratch, outputs) and the engine's stream: per engine, never shared by forks
static int alloc_sample_state(bk_engine* e) {
    const bk_params* prm = &e->params;
    const IndexTables& ix = *e->ix;
    for (MatePlane& p : e->mate) BK_HIP(p.counters.alloc(ix.plane_len));
    // A plane of a large index is a thousandth full after a sample: above 16 M counters (128 MB) the writers note what they touch
    // and finalize walks lists and clears what it read instead of scanning and zeroing planes (BK_SPARSE_FINALIZE forces it in
    // the testing build)
    e->sparse = ix.W > 0 && (ix.plane_len >= (16ull << 20) || test_env("BK_SPARSE_FINALIZE") != nullptr);
    if (e->sparse) {
        const uint64_t n_rows = bk::v_real_rows(ix.n_full, ix.v_span);
        for (MatePlane& p : e->mate) {
            BK_HIP(hipMemset(p.counters.p, 0, p.counters.n * sizeof(unsigned long long)));
            BK_HIP(p.touch_v.alloc(n_rows / 32 + 1)); BK_HIP(p.touch_p.alloc(ix.n_prows / 32 + 1)); BK_HIP(p.touch_e.alloc((size_t)ix.n_u / 32 + 1));
            BK_HIP(hipMemset(p.touch_v.p, 0, p.touch_v.n * 4)); BK_HIP(hipMemset(p.touch_p.p, 0, p.touch_p.n * 4));
            BK_HIP(hipMemset(p.touch_e.p, 0, p.touch_e.n * 4));
            BK_HIP(p.touch_b.alloc((size_t)ix.total_cells / 64 / 32 + 2)); BK_HIP(hipMemset(p.touch_b.p, 0, p.touch_b.n * 4));
            BK_HIP(p.v_list.alloc(n_rows)); BK_HIP(p.p_list.alloc(ix.n_prows)); BK_HIP(p.e_list.alloc(ix.n_u));
            BK_HIP(p.n_list.alloc(8));
        }
    }
    BK_HIP(e->shard_sums.alloc((size_t)2 * ix.n_files * 5 + 9));
    BK_HIP(e->xport_flag.alloc(4));
    BK_HIP(hipMemset(e->xport_flag.p, 0, 4 * sizeof(unsigned long long)));
    if (prm->full_kmer_stats) {
        if (prm->kmer_table_log2 < 10 || prm->kmer_table_log2 > 31) return fail(BK_ERR_INVALID, "kmer_table_log2 out of range");
        BK_HIP(e->ktab.keys.alloc((size_t)1 << prm->kmer_table_log2));
        BK_HIP(e->ktab.cnt.alloc((size_t)1 << prm->kmer_table_log2));
        e->ktab.log2 = prm->kmer_table_log2;
        BK_HIP(e->ktab.h_fill.grow(bk::ktab_fill_words())); BK_HIP(e->ktab.fill_ev.create());
    }
    BK_HIP(e->ktab_out.alloc(8 + bk::ktab_fill_words()));
    // one row of per-genome tallies per finalize workgroup (8192 rows: 10 MB at 100 genomes); without it every workgroup adds its
    // tallies to the same few cache lines of `stats` with global atomics -- 2 ms per kernel at 100 genomes
    if (ix.n_files <= 2048) BK_HIP(e->fin_partials.alloc(bk::finalize_partial_rows() * ((size_t)ix.n_files * 3 + 2)));
    BK_HIP(e->deferred.alloc(bk::v_plane_len(ix.n_full, ix.v_span, ix.n_prows) * (prm->pileup_selected_only ? 2 : 1)));   // (one list per mate file when it is kept between two passes)
    BK_HIP(e->n_deferred.alloc(2));   // one per mate file
    if (prm->pileup_selected_only && ix.ent_files.p) BK_HIP(e->deferred_mask.alloc(e->deferred.n));
    if (!e->sparse) {
        // dense planes: K2a zeroes the V counters as it reads them and the (small) E part is zeroed behind K2e, so a plane is
        // clean again when its sample is finalized -- no 37 MB memset per sample (config 2); the deferred k-mers' counts
        // travel with their indices
        BK_HIP(e->deferred_n.alloc(e->deferred.n));
        for (MatePlane& p : e->mate) BK_HIP(hipMemset(p.counters.p, 0, std::max<size_t>(p.counters.n, 1) * sizeof(unsigned long long)));
    }
    BK_HIP(e->pileup.alloc(ix.total_cells * 4 * 4));
    e->gather_mode = ix.gather_ok && e->sparse && ix.cell_file.p && ix.dirty_ans.p && ix.W > 1 && ix.file_cell_lo_d.p && !test_env("BK_NO_GATHER");
    if (e->gather_mode) {
        for (MatePlane& p : e->mate) BK_HIP(p.alias_hits.alloc((size_t)bk_engine::kAliasCap * 3));
        BK_HIP(e->n_alias_hits.alloc(2));
        BK_HIP(e->last_sel.upload(std::vector<int>(1, -1)));
        BK_HIP(hipMemset(e->pileup.p, 0, std::max<size_t>(e->pileup.n, 1) * sizeof(unsigned long long)));   // (selected-only: the rows of genomes never selected stay zero)
        // every genome's rows by the table of voters (bk_gather.hip): the table and the touched-row bits are this engine's for its
        // lifetime -- allocated here, never inside a sample (a hipMalloc synchronises the device: siblings in flight would stall)
        const bool two_pass = prm->pileup_selected_only != 0 && ix.n_files > 1;
        if (!two_pass && prm->cs < (1ull << 28) && ix.total_cells >= 2 * (uint64_t)ix.n_full && !test_env("BK_NO_VOTE_TABLE")) {
            BK_HIP(e->row_bits.alloc((size_t)((bk::v_real_rows(ix.n_full, ix.v_span) + 31) / 32) + 1));
            BK_HIP(e->vote_tab.alloc(bk::vote_table_words(ix.view())));
        }
    }
    BK_HIP(e->stats.alloc((size_t)2 * ix.n_files * 3));
    BK_HIP(e->present.alloc((size_t)2 * ix.n_files));
    if (prm->pileup_selected_only != 0 && ix.n_files > 1) BK_HIP(e->sel_out.alloc(1));   // (the genome selected between the two finalize passes)
    BK_HIP(e->l2_plan.alloc(4));
    BK_HIP(e->kstats.alloc(16));   // two sets, by sample parity (bk_engine::kstats_cur)
    // the scan: binned (items) when the planes are dense, the window's reference is staged in LDS and the bins are few enough;
    // else the whole-window difference array of scan_count_kernel with its slabs
    e->use_items = !e->sparse && ix.ref_in_lds && ix.W > 0 && ix.n_lds_bins > 0 && !test_env("BK_NO_ITEMS") && ix.seed_tab2.p && ix.rc_words.p &&
                   bk::item_geometry(std::min<uint32_t>(ix.n_lds_bins, (uint32_t)ix.total_cells), ix.n_full, ix.v_span, &e->ig) &&
                   bk::items_lds_bytes(e->ig, std::min<uint32_t>(ix.n_lds_bins, (uint32_t)ix.total_cells)) <= 128u * 1024u;
    if (e->use_items) {
        if (const char* cp = test_env("BK_ITEM_CAPS")) {   // measurement aid: "cap_e,cap_v" (multiples of 8, at most 64)
            unsigned ce = 0, cv = 0;
            if (sscanf(cp, "%u,%u", &ce, &cv) == 2 && ce >= 8 && cv >= 8 && ce <= 64 && cv <= 64 && ce % 8 == 0 && cv % 8 == 0) {
                bk::ItemGeom g2 = e->ig;
                g2.cap_e = ce; g2.cap_v = cv; g2.wg_items = g2.n_ebins * ce + g2.n_vbins * cv; g2.wg_stride = g2.wg_items;
                if (bk::items_lds_bytes(g2, std::min<uint32_t>(ix.n_lds_bins, (uint32_t)ix.total_cells)) <= 118u * 1024u) e->ig = g2;
            }
        }
        const size_t g = bk::items_max_grid(ix.n_cus);
        e->ig.grid_max = (uint32_t)g;
        BK_HIP(e->items.alloc(g * e->ig.wg_stride + 64));   // (+ 64: bin_count reads whole 16-byte units)
        BK_HIP(e->item_tab.alloc(g * ((size_t)e->ig.n_ebins + e->ig.n_vbins)));
        BK_HIP(e->item_gext.alloc(g * ((size_t)e->ig.n_ebins + e->ig.n_vbins) * bk::kItemGCap));   // (92 MB for one SARS-CoV-2 genome: 2 bytes x 256 slots x 701 bins x 256 workgroups)
        BK_HIP(e->ov.alloc((size_t)1 << 20));
        BK_HIP(e->ov_n.alloc(4));   // [2] overflow counts by launch parity, behind them (as 32-bit words) the scan's two chunk counters
        BK_HIP(hipMemset(e->ov_n.p, 0, 4 * sizeof(unsigned long long)));
    } else {
        BK_HIP(e->slabs.alloc((size_t)ix.n_cus * std::max<uint32_t>(ix.n_lds_bins, 1)));
    }
    if (ix.n_files > 1) { BK_HIP(e->win_votes.alloc((size_t)ix.n_files)); BK_HIP(e->win_sel.upload(std::vector<uint32_t>(2, 0u))); }
    // the scan's V items straight into the regional finalize (bk_finalize_lean.hip): where that kernel runs (one genome file, dense
    // planes, no statistics table, no pseudo k-mers, an answer table; FinalizeArgs are checked again at finalize), a V bin is the 64
    // row positions of one of its workgroups, and Level 2 is the only other writer of the V part (ScanArgs::n_direct: no nbatch_kernel)
    e->fuse_ok = e->use_items && ix.n_files == 1 && ix.max_seqs_per_file == 1 && (uint64_t)ix.n_lds_bins >= ix.total_cells && !e->ktab.keys.p && ix.n_prows == 0 &&
                 ix.n_u == ix.n_full && ix.n_full > 0 && ix.dirty_ans.p && ix.W > 1 && ix.v_span > 0 && ix.v_span <= 32 && e->fin_partials.p &&
                 prm->cs < (1ull << 32) && e->ig.vq_log2 == 6 && !test_env("BK_NO_LEAN_FINALIZE") && !test_env("BK_NO_FUSE") && !test_env("BK_NO_N_DIRECT");
    if (e->fuse_ok)
        for (MatePlane& p : e->mate) { BK_HIP(p.fuse_touch.alloc(((size_t)ix.n_full + (size_t)ix.v_span + 63) / 64 * 12 + 16)); BK_HIP(hipMemset(p.fuse_touch.p, 0, p.fuse_touch.n * sizeof(unsigned int))); }
    BK_HIP(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    e->stream = e->own_stream;
    return BK_OK;
}

extern "C" {

int bk_abi_version(void) { return BK_ABI_VERSION; }
int bk_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}
int bk_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
    if (!free_bytes || !total_bytes) return fail(BK_ERR_INVALID, "null argument");
    BK_HIP(hipSetDevice(device));
    size_t f = 0, t = 0;
    BK_HIP(hipMemGetInfo(&f, &t));
    *free_bytes = f; *total_bytes = t;
    return BK_OK;
}
const char* bk_last_error(void) { return g_err.c_str(); }

void bk_params_default(bk_params* p) {
    if (!p) return;
    p->n_fixed = 2;           // consts.rs:17
    p->use_full_kmer = 0;     // consts.rs:18
    p->ci = 3;                // consts.rs:5
    p->cs = 1000000;          // call.rs:1173
    p->cx = 1000000000ull;    // KMC default -cx
    p->device = 0;
    p->full_kmer_stats = 0;
    p->kmer_table_log2 = 26;
    p->pileup_selected_only = 0;
}


int bk_engine_create(const bk_index_desc* ix, const bk_params* prm, bk_engine** out) {
    if (!ix || !prm || !out) return fail(BK_ERR_INVALID, "null argument");
    *out = nullptr;
    const int k = ix->k;
    if (k < 3 || k > bk::kMaxK || (k & 1) == 0) return fail(BK_ERR_INVALID, "Invalid kmer size %d, must be odd and <= %d", k, bk::kMaxK);
    if (prm->n_fixed < 0) return fail(BK_ERR_INVALID, "n_fixed must be >= 0");
    if (ix->n_files <= 0 || ix->n_files > 65536) return fail(BK_ERR_INVALID, "n_files out of range");
    if (ix->n_buckets && (!ix->bucket_ids || !ix->bucket_off || !ix->entries)) return fail(BK_ERR_INVALID, "null index arrays");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(BK_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (prm->device < 0 || prm->device >= ndev) return fail(BK_ERR_NO_DEVICE, "device %d not present (%d visible)", prm->device, ndev);
    BK_HIP(hipSetDevice(prm->device));
    {
        hipDeviceProp_t prop;
        BK_HIP(hipGetDeviceProperties(&prop, prm->device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)   // the kernels are built for gfx950 only
            return fail(BK_ERR_NO_DEVICE, "device %d is %s, not gfx950 (MI355X); this library has no other code path", prm->device, prop.gcnArchName);
    }

    auto tab = std::make_shared<IndexTables>();
    PhaseClock pc;
    if (int rc = build_index_tables(ix, prm, *tab, pc)) return rc;
    std::unique_ptr<bk_engine> e(new bk_engine());
    e->params = *prm;
    e->device = prm->device;
    e->ix = tab;
    if (int rc = alloc_sample_state(e.get())) return rc;
    BK_HIP(tab->d_view.upload(std::vector<bk::IndexView>(1, tab->view())));
    pc.lap("uploads + buffers");
    *out = e.release();
    return BK_OK;
}

int bk_engine_fork(const bk_engine* parent, bk_engine** out) { return bk_engine_fork_params(parent, nullptr, out); }

int bk_engine_fork_params(const bk_engine* parent, const bk_params* prm, bk_engine** out) {
    if (!parent || !out) return fail(BK_ERR_INVALID, "null argument");
    if (prm && (prm->n_fixed != parent->params.n_fixed || (prm->use_full_kmer != 0) != (parent->params.use_full_kmer != 0) ||
                prm->device != parent->params.device || (prm->full_kmer_stats != 0) != (parent->params.full_kmer_stats != 0)))
        return fail(BK_ERR_INVALID, "bk_engine_fork_params: n_fixed, use_full_kmer, full_kmer_stats and device shape the shared tables and must equal the parent's");
    if (prm && prm->cs == 0) return fail(BK_ERR_INVALID, "cs must be >= 1");
    BK_HIP(hipSetDevice(parent->device));
    std::unique_ptr<bk_engine> e(new bk_engine());
    e->params = prm ? *prm : parent->params;
    e->device = parent->device;
    e->ix = parent->ix;   // the index tables are immutable after bk_engine_create: the fork reads the parent's
    e->ix->family.fetch_add(1);
    if (int rc = alloc_sample_state(e.get())) return rc;
    *out = e.release();
    return BK_OK;
}

void bk_engine_destroy(bk_engine* e) {
    if (!e) return;
    e->ix->family.fetch_sub(1);
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (auto& s : e->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto ev : e->free_events) (void)hipEventDestroy(ev);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;
}

int bk_engine_set_stream(bk_engine* e, void* hip_stream) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    BK_HIP(hipStreamSynchronize(e->stream));
    e->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : e->own_stream;
    return BK_OK;
}

void* bk_engine_get_stream(const bk_engine* e) { return e ? reinterpret_cast<void*>(e->stream) : nullptr; }

uint64_t bk_total_cells(const bk_engine* e) { return e ? e->ix->total_cells : 0; }
int32_t bk_n_files(const bk_engine* e) { return e ? e->ix->n_files : 0; }
uint64_t bk_n_slots(const bk_engine* e) { return e ? e->ix->n_slots : 0; }
uint64_t bk_counter_len(const bk_engine* e) { return e ? e->ix->plane_len : 0; }
int bk_can_shard(const bk_engine* e) { return e && !e->sparse ? 1 : 0; }

// a sample starts from an empty table (the capacity the last one grew to stays)
int GrowTable::clear(bk_engine* e) {
    if (!old.empty()) {   // tables the previous sample outgrew
        BK_HIP(hipStreamSynchronize(e->stream));
        for (auto& o : old) { (void)hipFree(o.first); (void)hipFree(o.second); }
        old.clear();
    }
    BK_HIP(hipMemsetAsync(keys.p, 0xff, keys.n * sizeof(unsigned long long), e->stream));
    BK_HIP(hipMemsetAsync(cnt.p, 0, cnt.n * sizeof(unsigned int), e->stream));
    fill_known = 0; fill_unknown_upper = 0; fill_pending = false;
    return BK_OK;
}

// may this engine's samples leave their zeroing to the Level 2 launch (bk_sample_begin)?  BK_NO_ZERO_RIDE (testing build): never
static bool zero_ride_ok(const bk_engine* e) {
    const bool sel_rows = e->gather_mode && e->params.pileup_selected_only != 0 && e->ix->n_files > 1;
    return !e->ktab.keys.p && !sel_rows && !test_env("BK_NO_ZERO_RIDE");
}
// what the zero ride zeroes: the sample's outputs and the kstats set of the next sample
static bk::ZeroRide zero_ride_args(const bk_engine* e) {
    bk::ZeroRide z{};
    z.big = e->pileup.p; z.n_big = e->gather_mode ? 0 : e->pileup.n;
    z.a = e->stats.p; z.n_a = (uint32_t)e->stats.n; z.b = e->kstats_other(); z.n_b = 8;
    z.c = e->present.p; z.n_c = (uint32_t)e->present.n; z.d = e->n_deferred.p; z.n_d = (uint32_t)e->n_deferred.n;
    return z;
}
// A sample whose zeros are still owed and that is about to need them (its finalize; it had no Level 2 launch to carry them): the
// launch bk_sample_begin left out, over the same buffers as the ride.
static void pay_owed_zeros(bk_engine* e) {
    if (!e->zero_owed) return;
    bk_engine::Span sp(e, 2);
    const bk::ZeroRide z = zero_ride_args(e);
    bk::launch_zero_small(z.a, z.n_a, z.b, z.n_b, nullptr, 0, z.c, z.n_c, z.d, z.n_d, z.big, z.n_big, e->stream);
    e->zero_owed = false; e->next_clean = true;
}

int bk_sample_begin(bk_engine* e) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    BK_HIP(hipSetDevice(e->device));
    bk_engine::Span sp(e, 2);
    e->win_chosen = false;
    // gathered votes (bk_gather.hip) store the rows they own: every genome's rows -- nothing to zero; the selected genome's -- the rows
    // the previous sample wrote are all that is not zero
    const bool sel_rows = e->gather_mode && e->params.pileup_selected_only != 0 && e->ix->n_files > 1;
    // The zero ride.  Nothing reads or writes the pileup, stats, present or n_deferred between here and the sample's finalize, so
    // they are zeroed by workgroups of the sample's first Level 2 launch (push_device; pay_owed_zeros for a sample that has none) and
    // not by a launch of their own.  The four words of kstats that the pushes add to must be clean NOW: that launch zeroed them a
    // sample ahead, in the set of the other parity.  Without the statistics table (ktab_out is its results) and the gathered votes'
    // row zeroing; the first sample of an engine, and one behind a sample that never paid, zero everything here as ever.
    if (zero_ride_ok(e) && e->next_clean) {
        e->kstats_par ^= 1; e->zero_owed = true; e->next_clean = false;
    } else {
        bk::launch_zero_small(e->stats.p, e->stats.n, e->kstats.p, e->kstats.n, e->ktab_out.p, e->ktab_out.n, e->present.p, e->present.n,
                              e->n_deferred.p, e->n_deferred.n, e->pileup.p, e->gather_mode ? 0 : e->pileup.n, e->stream);   // (both sets of kstats)
        e->zero_owed = false; e->next_clean = true;
    }
    if (sel_rows) bk::launch_zero_genome_rows(e->pileup.p, (size_t)e->ix->total_cells * 4, e->ix->file_cell_lo_d.p, e->ix->n_files, (uint32_t)e->ix->total_cells, e->last_sel.p, e->stream);
    if (e->ktab.keys.p) { if (int rc = e->ktab.clear(e)) return rc; }
    if (e->dump) { if (int rc = e->dump->begin_sample(e)) return rc; }
    for (EventPass* p : e->event_passes()) if (p) { if (int rc = p->begin_sample(e)) return rc; }
    if (e->linkage) { if (int rc = e->linkage->begin_sample(e)) return rc; }
    if (e->primers) { if (int rc = e->primers->begin_sample(e)) return rc; }
    if (e->adapters) { if (int rc = e->adapters->begin_sample(e)) return rc; }
    e->ktab_exchanged = false; e->in_sample = true; e->finalized_mates = 0; e->called = false; e->cons_made = false; e->minor_made = false; e->ci_made = false; e->regions_made = false;
    // items of a sample that was begun and never finalized are nobody's any more; neither are the rows Level 2 noted for them
    e->pending.on = false;
    for (MatePlane& p : e->mate) { if (int rc = p.begin_sample(e)) return rc; }
    return BK_OK;
}

int MatePlane::begin_sample(bk_engine* e) {
    stale = true; fuse_off = false; reduced_shards = 0; pushed_records = 0;
    if (touch_used) { BK_HIP(hipMemsetAsync(fuse_touch.p, 0, fuse_touch.n * sizeof(unsigned int), e->stream)); touch_used = false; }
    return BK_OK;
}

// the waiting V items of an earlier launch go to their plane after all: bin_count_kernel over the V bins, adding (Level 2 of that
// launch may have written to the plane since)
static int flush_pending_items(bk_engine* e) {
    if (!e->pending.on) return BK_OK;
    bk_engine::Span sp(e, 3);
    bk::BinArgs b = e->pending.b;
    b.part = 2; b.v_mode = e->ix->item_v_mode >= 0 && e->ix->item_v_mode != 2 ? e->ix->item_v_mode : 1;
    e->pending.on = false; e->mate[e->pending.mate].no_more_waiting();
    BK_HIP(bk::launch_bin_count(b, e->stream));
    return BK_OK;
}

int MatePlane::zero_if_stale(bk_engine* e) {
    if (!stale) return BK_OK;
    if (used) {   // (a sample that was abandoned, or a dense plane finalized in shards: whole samples leave their planes clean)
        bk_engine::Span sp(e, 2);
        BK_HIP(hipMemsetAsync(counters.p, 0, std::max<size_t>(counters.n, 1) * sizeof(unsigned long long), e->stream));
        if (e->sparse) for (DevBuf<unsigned int>* t : {&touch_v, &touch_p, &touch_b, &touch_e}) BK_HIP(hipMemsetAsync(t->p, 0, t->n * 4, e->stream));
        used = false;
    }
    stale = false;
    v_clean = true;   // all zero now: the sample's first bin_count launch stores where it would add
    return BK_OK;
}

// full_kmer_stats: the statistics table holds every distinct k-mer that touches no window bucket -- as many as the sample has
// sequencing errors, unknown in advance (the k-mer dump's table: every distinct k-mer).  Its load stays below one half: before a
// batch of at most `upper` k-mers is pushed, the keys it holds (read back from the device tallies at out[8 ..] after every push;
// the engine only waits for that reading when the bound says the batch might not fit) plus `upper` must fit, else the table is
// rehashed into one four times larger.
int GrowTable::ensure_room(bk_engine* e, unsigned long long* out, uint64_t upper) {
    if (!keys.p) return BK_OK;
    const uint64_t cap = 1ull << log2;
    if (fill_known + fill_unknown_upper + upper > cap / 2) {
        if (fill_pending) { BK_HIP(hipEventSynchronize(fill_ev)); read_fill(); }
        uint32_t nl = log2;
        while (nl < 31 && fill_known + fill_unknown_upper + upper > (1ull << nl) / 2) nl += 2;
        if (nl > 31) nl = 31;
        if (nl != log2) {
            unsigned long long* nk = nullptr; unsigned int* nc = nullptr;
            BK_HIP(hipMalloc(reinterpret_cast<void**>(&nk), ((size_t)1 << nl) * sizeof(unsigned long long)));
            BK_HIP(hipMalloc(reinterpret_cast<void**>(&nc), ((size_t)1 << nl) * sizeof(unsigned int)));
            BK_HIP(hipMemsetAsync(nk, 0xff, ((size_t)1 << nl) * sizeof(unsigned long long), e->stream));
            BK_HIP(hipMemsetAsync(nc, 0, ((size_t)1 << nl) * sizeof(unsigned int), e->stream));
            bk::launch_ktab_rehash(keys.p, cnt.p, log2, nk, nc, nl, out + 4, e->stream);
            old.emplace_back(keys.p, cnt.p);   // still read by the rehash in flight
            keys.p = nk; keys.n = (size_t)1 << nl;
            cnt.p = nc; cnt.n = (size_t)1 << nl;
            log2 = nl;
        }
    }
    fill_unknown_upper += upper;
    return BK_OK;
}
int GrowTable::note_fill(bk_engine* e, const unsigned long long* out) {   // after a push: a fresh copy of the tallies
    if (!keys.p) return BK_OK;
    BK_HIP(hipMemcpyAsync(h_fill.p, out + 8, bk::ktab_fill_words() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipEventRecord(fill_ev, e->stream));
    fill_pending = true;
    return BK_OK;
}

#ifdef BK_TESTING   // (the testing build's reports)
// BK_L2_COUNT (debugging aid): how much a scan launch leaves to Level 2
static int l2_count_report(bk_engine* e, const bk::ScanArgs& a) {
    if (!test_env("BK_L2_COUNT")) return BK_OK;
    const uint64_t take = a.n_records;
    std::vector<unsigned int> hb((size_t)take * a.l2_words), ha((size_t)(take + 31) / 32);
    BK_HIP(hipMemcpyAsync(hb.data(), e->n_bits.p, hb.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipMemcpyAsync(ha.data(), e->n_any.p, ha.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    uint64_t nk = 0, nr = 0, runs = 0;
    for (size_t i = 0; i < hb.size(); i++) { nk += (uint64_t)__builtin_popcount(hb[i]); runs += (uint64_t)__builtin_popcount(hb[i] & ~(hb[i] << 1)); }
    for (unsigned int w : ha) nr += (uint64_t)__builtin_popcount(w);
    fprintf(stderr, "[bk] left to level 2 by the scan: %llu of %llu records marked, %llu k-mers in %llu N runs (per 32-bit word)\n", (unsigned long long)nr,
            (unsigned long long)take, (unsigned long long)nk, (unsigned long long)runs);
    return BK_OK;
}
// BK_L2_STATS: the scan and Level 2 tally what they see in `dbg` (allocated by the first push that asks for it); every finalize prints
// the tallies, the clocks of the last scan launch's workgroups and what finalize deferred, and zeroes them
static int l2_stats_arm(bk_engine* e) {
    if (test_env("BK_L2_STATS") && !e->dbg.p) { BK_HIP(e->dbg.alloc(32 + 4 * 1024)); BK_HIP(hipMemsetAsync(e->dbg.p, 0, (32 + 4 * 1024) * sizeof(unsigned long long), e->stream)); }
    return BK_OK;
}
static int l2_stats_report(bk_engine* e) {
    if (!e->dbg.p) return BK_OK;
    const IndexTables& ix = *e->ix;
    unsigned long long h[32]; unsigned int nd[2] = {0, 0};
    BK_HIP(hipMemcpyAsync(nd, e->n_deferred.p, sizeof nd, hipMemcpyDeviceToHost, e->stream));
    std::vector<unsigned long long> clk(4 * 1024);
    BK_HIP(hipMemcpyAsync(h, e->dbg.p, sizeof h, hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipMemcpyAsync(clk.data(), e->dbg.p + 32, clk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipMemsetAsync(e->dbg.p, 0, (32 + 4 * 1024) * sizeof(unsigned long long), e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    // the scan's workgroups on the clock (the sample's last launch): when each started, had its reference, ran out of tiles, ended
    unsigned long long t0 = ~0ull;
    int n_wg = 0;
    for (int b = 0; b < 512; b++) if (clk[4 * b]) { t0 = std::min(t0, clk[4 * b]); n_wg = b + 1; }   // (the second half holds the prologue clocks)
    if (n_wg) {
        double mx[4] = {0, 0, 0, 0}, mean[4] = {0, 0, 0, 0}, mn[4] = {1e30, 1e30, 1e30, 1e30};
        for (int b = 0; b < n_wg; b++)
            for (int j = 0; j < 4; j++) {
                const double us = (double)(clk[4 * b + j] - t0) * 0.01;
                mx[j] = std::max(mx[j], us); mn[j] = std::min(mn[j], us); mean[j] += us / n_wg;
            }
        fprintf(stderr, "[bk] scan workgroups (%d), us after the first start, min / mean / max: start %.1f / %.1f / %.1f, reference staged %.1f / %.1f / %.1f, "
                "tiles done %.1f / %.1f / %.1f, end %.1f / %.1f / %.1f\n", n_wg, mn[0], mean[0], mx[0], mn[1], mean[1], mx[1], mn[2], mean[2], mx[2], mn[3], mean[3], mx[3]);
        double m2[4] = {0, 0, 0, 0};
        int n2 = 0;
        for (int b = 0; b < std::min(n_wg, 512); b++) if (clk[2048 + 4 * b]) { n2++; for (int j = 0; j < 4; j++) m2[j] += (double)(clk[2048 + 4 * b + j] - t0) * 0.01; }
        if (n2) fprintf(stderr, "[bk]   ... mean: first tile's copy sent %.1f, window's loads stored %.1f, wave 0 has its first tile %.1f, buckets written out %.1f\n",
                        m2[0] / n2, m2[1] / n2, m2[2] / n2, m2[3] / n2);
        if (test_env("BK_L2_STATS")[0] == '2')
            for (int b = 0; b < n_wg; b++) fprintf(stderr, "[bk]   wg %d: %.1f %.1f %.1f %.1f\n", b, (clk[4 * b] - t0) * 0.01, (clk[4 * b + 1] - t0) * 0.01, (clk[4 * b + 2] - t0) * 0.01, (clk[4 * b + 3] - t0) * 0.01);
    }
    fprintf(stderr, "[bk] finalize: %u + %u k-mers deferred (items the regional finalize settles in place, or the general kernel's list)\n", nd[0], nd[1]);
    if (e->gather_mode) {
        unsigned int ah[2] = {0u, 0u};
        BK_HIP(hipMemcpy(ah, e->n_alias_hits.p, sizeof ah, hipMemcpyDeviceToHost));
        fprintf(stderr, "[bk] votes gathered cell by cell (bk_gather.hip); alias hits among the deferred k-mers: %u + %u\n", ah[0], ah[1]);
    }
    if (e->sparse) {
        unsigned int nl[8];
        BK_HIP(hipMemcpy(nl, e->mate[0].n_list.p, sizeof nl, hipMemcpyDeviceToHost));
        fprintf(stderr, "[bk] sparse finalize (mate file 0): %u V rows of %llu, %u pseudo rows of %llu, %u reference k-mers of %u and %u pseudo k-mers of %u touched\n",
                nl[0], (unsigned long long)bk::v_real_rows(ix.n_full, ix.v_span), nl[4], (unsigned long long)ix.n_prows, nl[2], ix.n_full, nl[3], ix.n_u - ix.n_full);
    }
    fprintf(stderr, "[bk] scan: %llu mismatches counted, %llu items processed, %llu E gaps before a mismatch, %llu behind the last\n", h[23], h[24], h[25], h[26]);
    fprintf(stderr, "[bk] scan N batches: %llu with %llu pieces (%.1f per batch), %llu of them forced by a tile's end\n", h[20], h[21], h[20] ? (double)h[21] / (double)h[20] : 0.0, h[22]);
    fprintf(stderr, "[bk] level 2 discovery: %llu records newly marked by the scan, %llu records queued, g_work %llu\n", h[27], h[28], h[29]);
    fprintf(stderr, "[bk] scan marked: no-diagonal %llu, dirty-head %llu, clean-head %llu, pairs %llu | level 2: k-mers %llu in %llu chunks, simple %llu, dead %llu, "
            "dirty answers %llu (one difference but id unknown: %llu), neither half present %llu, slow %llu (diffs 0/1/2/3+ with a diagonal: %llu/%llu/%llu/%llu) -> member %llu, neighbour %llu, nothing %llu\n",
            h[0], h[1], h[2], h[3], h[4], h[11], h[5], h[6], h[16], h[17], h[18], h[7], h[12], h[13], h[14], h[15], h[8], h[9], h[10]);
    return BK_OK;
}
#else
static int l2_count_report(bk_engine*, const bk::ScanArgs&) { return BK_OK; }
static int l2_stats_arm(bk_engine*) { return BK_OK; }
static int l2_stats_report(bk_engine*) { return BK_OK; }
#endif

// The scan's arguments that every launch of a push shares.  Built for each push: a rehash of the statistics table
// (GrowTable::ensure_room) moves ktab.keys and raises ktab.log2 in the middle of a sample.
static bk::ScanArgs scan_args(const bk_engine* e, int mate, const Records& r) {
    const IndexTables& ix = *e->ix;
    const MatePlane& pl = e->mate[mate];
    bk::ScanArgs a{};
    a.n_records_dev = r.n_dev; a.ixp = ix.d_view.p;
    a.k = ix.k; a.wstart = ix.wstart; a.W = ix.W; a.v_omin = ix.v_omin; a.v_span = ix.v_span; a.v_off = ix.v_off; a.total_cells = (uint32_t)ix.total_cells; a.n_u = ix.n_u;
    a.ref_words = ix.ref_words.p; a.cell_codes = ix.cell_codes.p; a.cell_has = ix.cell_has.p; a.cell_clean = ix.cell_clean.p; a.cell_clean3 = ix.cell_clean3.p; a.cell_yf = ix.cell_yf.p; a.cell_yr = ix.cell_yr.p; a.id_at = ix.id_at.p; a.cell_fast = ix.cell_fast.p; a.cell_nat = ix.cell_nat.p; a.cell_natrow = ix.cell_natrow.p; a.cell_blk = ix.cell_blk.p; a.seed_tab = ix.seed_tab.p; a.seed_log2 = ix.seed_log2;
    a.seed_tab2 = ix.seed_tab2.p; a.seed2_log2 = ix.seed2_log2; a.rc_words = ix.rc_words.p;
    a.n_direct = e->use_items && ix.n_files == 1 && ix.max_seqs_per_file == 1 && (uint64_t)ix.n_lds_bins >= ix.total_cells && !test_env("BK_NO_N_DIRECT");
    a.words = r.words; a.lens = r.lens; a.n_records = r.n; a.stride_words = r.stride_words;
    a.counters = pl.counters.p; a.kmer_total = e->kstats_cur() + mate * 4 + 1;
    a.ablate = ix.ablate; a.slabs = e->slabs.p; a.n_lds_bins = ix.n_lds_bins; a.ref_in_lds = ix.ref_in_lds ? 1 : 0;
    a.ktab_keys = e->ktab.keys.p; a.ktab_cnt = e->ktab.cnt.p; a.ktab_log2 = e->ktab.log2;
    a.ktab_overflow = e->ktab_out.p + 4; a.mate = (uint32_t)mate;
    a.occ = ix.occ.p; a.n_files = ix.n_files;
    if (e->sparse) {
        a.touch_v = pl.touch_v.p; a.touch_b = pl.touch_b.p; a.touch_p = pl.touch_p.p; a.touch_e = pl.touch_e.p;
        a.rl_recip = ~0ull / (unsigned long long)(ix.v_span + 1) + 1ull;   // ceil(2^64 / row length): exact quotients for 32-bit counter indices
    }
    a.dbg = e->dbg.p; a.l2_words = bk::scan_l2_words(r.stride_words, ix.k); a.l2_min_grid = (uint32_t)std::max(1, ix.n_cus / 2);
    if (const char* mg = test_env("BK_L2_MIN_GRID")) a.l2_min_grid = (uint32_t)std::max(1, atoi(mg));   // testing aid: a plan so small that a wave of level2_kernel goes round several times
    if (e->use_items) { a.ig = e->ig; a.items = e->items.p; a.tab = e->item_tab.p; a.gext = e->item_gext.p; a.ov = e->ov.p; a.ov_n = e->ov_n.p; a.ov_cap = (uint32_t)e->ov.n; }
    return a;
}
// Multi-genome indexes: the first records of the sample vote for the genome they look like; the LDS window goes on that genome and
// stays there for the sample.  Vote and choice are made on the device (the scan reads the window from device memory): no host round
// trip between a sample's first push and its scan.  Any choice gives the same counts -- this is about speed.
static int choose_window(bk_engine* e, bk::ScanArgs& a, uint64_t n) {
    const IndexTables& ix = *e->ix;
    if (ix.occ.p && !e->win_chosen && n > 0) {
        BK_HIP(hipMemsetAsync(e->win_votes.p, 0, e->win_votes.n * sizeof(unsigned int), e->stream));
        const char* wf = test_env("BK_WINDOW_FILE");   // testing aid
        const int forced = wf ? std::max(0, atoi(wf)) : -1;
        bk::launch_pick_window(a, 16384, e->win_votes.p, ix.file_cell_lo_d.p, forced, e->win_sel.p, e->stream);
        e->win_chosen = true;
    }
    a.win_dev = ix.occ.p ? e->win_sel.p : nullptr;
    return BK_OK;
}
// How many of the `left` records the next launch scans (at most `l2_cap`), and on how many workgroups (`grid`)
static uint64_t next_launch(const bk_engine* e, uint64_t left, uint64_t l2_cap, uint32_t& grid) {
    const IndexTables& ix = *e->ix;
    grid = bk::scan_grid(left, ix.n_cus);
    // (the slab scan: no more than one workgroup's 16-bit LDS bins can receive; the binned scan has none to keep from wrapping)
    uint64_t take = e->use_items ? std::min<uint64_t>(left, l2_cap) : std::min<uint64_t>(std::min<uint64_t>(left, bk::scan_max_records(grid)), l2_cap);
    if (ix.max_launch_records) take = std::min<uint64_t>(take, ix.max_launch_records);
    if (e->use_items) {
        // A scan workgroup fills its CU (16 waves of 128 registers, 127 KB of LDS): on every CU it shuts out the other samples'
        // finalize / Level 2 kernels, which are chains of short launches that wait for latency, not for CUs.  With siblings in
        // flight three quarters of the CUs scan and the rest keep those chains moving (config 2, three samples in flight: 8.35
        // -> 9.06 G reads/s; one sample alone is 4% slower that way and keeps the whole chip).  DESIGN.md §4 has the sweeps of the
        // share: three quarters, whatever the number of siblings.
        int share = ix.n_cus - ix.n_cus / 4;
        if (const char* fr = test_env("BK_ITEM_SHARE")) share = std::max(1, std::min(ix.n_cus, ix.n_cus * atoi(fr) / 16));   // measurement aid: sixteenths of the CUs
        grid = bk::items_grid(take, ix.family.load() > 1 ? share : ix.n_cus);
        if (const char* gr = test_env("BK_ITEM_GRID")) grid = std::max<uint32_t>(1, std::min<uint32_t>(grid, (uint32_t)atoi(gr)));
    }
    return take;
}
// Level 2's buffers for a launch of a.n_records records: grown (the stream drained first) when the launch does not fit them
static int make_l2_room(bk_engine* e, bk::ScanArgs& a, uint64_t l2_cap) {
    if (e->l2_bits.n < a.n_records * a.l2_words || e->l2_diag.n < a.n_records) {
        BK_HIP(hipStreamSynchronize(e->stream));
        const uint64_t recs = std::min<uint64_t>(std::max<uint64_t>(a.n_records + a.n_records / 4, 1 << 16), l2_cap);
        BK_HIP(e->l2_bits.alloc((size_t)recs * a.l2_words)); BK_HIP(e->n_bits.alloc((size_t)recs * a.l2_words)); BK_HIP(e->l2_diag.alloc((size_t)recs));
        BK_HIP(e->l2_any.alloc((size_t)(recs + 31) / 32)); BK_HIP(e->n_any.alloc((size_t)(recs + 31) / 32));
        for (DevBuf<unsigned int>* b : {&e->l2_bits, &e->l2_any, &e->n_bits, &e->n_any}) BK_HIP(hipMemsetAsync(b->p, 0, b->n * sizeof(unsigned int), e->stream));
    }
    a.l2_bits = e->l2_bits.p; a.l2_diag = e->l2_diag.p; a.l2_any = e->l2_any.p; a.n_bits = e->n_bits.p; a.n_any = e->n_any.p;
    return BK_OK;
}
// The binned scan's items, bin by bin -> u64 plane (before Level 2 adds to it: a sample's first launch finds the V part all zero).
// `wait_v`: the mate file's first launch, whose V items wait for the regional finalize (or for the next launch, which sends them to
// the plane); Level 2 then notes the V rows it writes to.
// `ride`: Level 2 follows and counts the E bins inside its own launch (*ride: what launch_level2 is to be given) -- both only add
// to the E counters with atomics and read only what the scan wrote, and nothing reads an E counter before the finalize.  Then
// bin_count_kernel is launched over the V bins alone (its plain read-modify-write of the V part stays in front of Level 2), and
// with waiting V items not at all.  E bin 0 zeroes the next launch's overflow count wherever the E bins run: once per scan launch.
static int bin_items(bk_engine* e, bk::ScanArgs& a, int mate, uint32_t grid, bool wait_v, bk::BinArgs* ride) {
    const IndexTables& ix = *e->ix;
    MatePlane& pl = e->mate[mate];
    bk_engine::Span sp(e, 3);
    bk::BinArgs b{};
    b.ig = e->ig; b.items = e->items.p; b.tab = e->item_tab.p; b.gext = e->item_gext.p; b.n_wg = grid; b.ov = e->ov.p; b.ov_n = e->ov_n.p; b.ov_cap = (uint32_t)e->ov.n;
    b.ov_par = e->ov_par; e->ov_par ^= 1u;
    b.id_at = ix.id_at.p; b.cell_codes = ix.cell_codes.p + bk::scan_ref_pad_words(); b.win_lo = a.win_lo; b.win_dev = a.win_dev; b.total_cells = (uint32_t)ix.total_cells;
    b.counters = pl.counters.p; b.v_off = ix.v_off; b.v_real_len = bk::v_real_len(ix.n_full, ix.v_span); b.rl = (uint32_t)ix.v_span + 1u;
    const bool v_clean = pl.take_v_clean();   // (whatever the mode: the next launch adds)
    b.v_mode = ix.item_v_mode >= 0 ? ix.item_v_mode : (v_clean ? 2 : 1);
    if (const char* ba = test_env("BK_BIN_ABLATE")) b.ablate = atoi(ba);
    if (wait_v) {
        e->pending.on = true; e->pending.mate = mate; e->pending.b = b;   // (the V bins' side of b: the same whoever counts the E bins)
        b.part = 1;
        a.touch_v = pl.fuse_touch.p; a.rl_recip = ~0ull / (unsigned long long)(ix.v_span + 1) + 1ull;
        pl.items_wait();
    } else {
        pl.no_more_waiting();
        if (e->fuse_ok) a.touch_v = nullptr;   // (a push of several launches: set by the first)
    }
    if (ride) {
        *ride = b; ride->part = 1;
        if (wait_v) return BK_OK;
        b.part = 2;
    }
    BK_HIP(bk::launch_bin_count(b, e->stream));
    return BK_OK;
}
// will level2_and_fold launch level2_kernel for this scan launch?  (Only then can the E bins ride in it.)
static bool level2_runs(const bk_engine* e, const bk::ScanArgs& a) { return e->ix->ablate != 1 && e->ix->ablate != 4 && bk::level2_launches(a); }
// Level 2 over the k-mers the scan left marked (it clears the marks it takes); behind the slab scan, its per-cell bin slabs -> u64 plane
static int level2_and_fold(bk_engine* e, const bk::ScanArgs& a, int mate, uint32_t grid, const bk::BinArgs* ride, const bk::ZeroRide* zero) {
    const IndexTables& ix = *e->ix;
    bk_engine::Span sp(e, 3);
    if (int rc = l2_count_report(e, a)) return rc;
    if (ix.ablate == 1 || ix.ablate == 4) {   // measurement aids: without Level 2 (and without a ride: push_device asked level2_runs)
        BK_HIP(hipMemsetAsync(e->n_bits.p, 0, (size_t)a.n_records * a.l2_words * sizeof(unsigned int), e->stream));
        BK_HIP(hipMemsetAsync(e->n_any.p, 0, e->n_any.n * sizeof(unsigned int), e->stream));
    }
    else BK_HIP(bk::launch_level2(a, ix.n_cus, e->stream, ride, zero));
    if (!e->use_items) {
        bk::FoldArgs f{};
        f.slabs = e->slabs.p; f.n_slabs = grid; f.n_lds_bins = ix.n_lds_bins; f.id_at = ix.id_at.p; f.cell_codes = ix.cell_codes.p + bk::scan_ref_pad_words(); f.win_lo = a.win_lo; f.win_dev = a.win_dev; f.touch_e = a.touch_e;
        f.counters = e->mate[mate].counters.p;
        bk::launch_fold(f, e->stream);
    }
    return BK_OK;
}
}  // extern "C" (bk_engine.h declares the next function for bk_ingest.cpp)
int push_device(bk_engine* e, int mate, const Records& r) {
    MatePlane& pl = e->mate[mate];
    if (int rc = pl.zero_if_stale(e)) return rc;
    const uint64_t n = r.n, upper = r.kmers_upper ? r.kmers_upper : n * (uint64_t)r.stride_words * 16;
    if (int rc = e->ktab.ensure_room(e, e->ktab_out.p, upper)) return rc;
    if (e->dump) { if (int rc = e->dump->push(e, mate, r, upper)) return rc; }
    pl.written();
    if (int rc = l2_stats_arm(e)) return rc;
    bk::ScanArgs a = scan_args(e, mate, r);
    if (e->ix->W <= 0) {
        // empty window: nothing can touch the index (map_kmers finds no bucket, call.rs:1291-1307); KMC's total k-mer count is all
        bk::launch_count_kmers(a, e->stream);
    } else {
        if (int rc = choose_window(e, a, n)) return rc;
        // a launch keeps Level 2's bitmap below 1 GiB
        const uint64_t l2_cap = std::max<uint64_t>(64, ((1ull << 30) / sizeof(unsigned int)) / a.l2_words);
        for (uint64_t base = 0; base < n; base += a.n_records) {
            uint32_t grid = 0;
            a.rec_base = base; a.n_records = next_launch(e, n - base, l2_cap, grid);
            if (int rc = make_l2_room(e, a, l2_cap)) return rc;
            if (int rc = flush_pending_items(e)) return rc;   // (the scan below overwrites the item buffers)
            const bool wait_v = e->fuse_ok && a.n_direct && !pl.fuse_off && e->ix->item_v_mode < 0;
            // (one genome file, the binned scan, four or more samples in flight: Level 2 on as many workgroups as its marks are worth)
            a.l2_plan = e->use_items && e->ix->n_files == 1 && e->ix->family.load() >= 4 && !test_env("BK_NO_L2_PLAN") ? e->l2_plan.p : nullptr;
            {
                bk_engine::Span sp(e, 0);
                if (e->use_items) { a.ov_par = e->ov_par; BK_HIP(bk::launch_scan_items(a, grid, e->stream)); }
                else BK_HIP(bk::launch_scan_count(a, grid, e->stream));
            }
            // (the binned scan followed by a Level 2 launch: its E bins ride in that launch; BK_NO_E_RIDE, testing build: a launch of their own)
            bk::BinArgs ride_b{};
            const bool ride = e->use_items && level2_runs(e, a) && !test_env("BK_NO_E_RIDE");
            if (e->use_items) { if (int rc = bin_items(e, a, mate, grid, wait_v, ride ? &ride_b : nullptr)) return rc; }
            // (the sample's first Level 2 launch: the zeros bk_sample_begin left owing ride in it too; later launches carry none)
            const bool zride = e->zero_owed && level2_runs(e, a);
            const bk::ZeroRide zero_b = zride ? zero_ride_args(e) : bk::ZeroRide{};
            if (int rc = level2_and_fold(e, a, mate, grid, ride ? &ride_b : nullptr, zride ? &zero_b : nullptr)) return rc;
            if (zride) { e->zero_owed = false; e->next_clean = true; }
        }
    }
    for (EventPass* p : e->event_passes()) if (p) { if (int rc = p->push(e, r)) return rc; }
    if (e->linkage) { if (int rc = e->linkage->push(e, r)) return rc; }
    BK_HIP(hipGetLastError());
    if (!r.n_dev) pl.pushed_records += n;
    return e->ktab.note_fill(e, e->ktab_out.p);
}
extern "C" {

int bk_counters_device_ptr(bk_engine* e, int mate, void** d_ptr) {
    if (!e || !d_ptr || mate < 0 || mate > 1) return fail(BK_ERR_INVALID, "bad argument");
    if (e->sparse) return fail(BK_ERR_UNSUPPORTED, "an index this large keeps its counter planes sparse: shard whole samples over GPUs, not one sample's reads");
    if (e->pending.on) { BK_HIP(hipSetDevice(e->device)); if (int rc = flush_pending_items(e)) return rc; }
    if (e->in_sample) {   // a mate file nothing was pushed for yet: its plane is zeroed lazily -- now, before the caller reduces it
        BK_HIP(hipSetDevice(e->device));
        if (int rc = e->mate[mate].zero_if_stale(e)) return rc;
    }
    e->mate[mate].handed_out();   // (so the next bin_count launch adds to the V part instead of storing over it)
    *d_ptr = e->mate[mate].counters.p;
    return BK_OK;
}

int bk_pileup_device_ptr(bk_engine* e, void** d_ptr) {
    if (!e || !d_ptr) return fail(BK_ERR_INVALID, "bad argument");
    *d_ptr = e->pileup.p;
    return BK_OK;
}

// One finalize call: the part of the planes it maps; pileup_selected_only's two passes (the statistics of every genome, the genome's
// selection, its votes); gathered votes (the statistics pass, then gather_votes_kernel); whole dense planes, which it leaves zeroed
struct FinalizeCall { int n_mates; uint64_t elem_lo, elem_hi; bool two_pass = false, gather = false, clean_dense = false; };
// sparse planes: the touch bitmaps -> the lists finalize walks
static int compact_sparse_lists(bk_engine* e, int n_mates) {
    const IndexTables& ix = *e->ix;
    for (int m = 0; m < n_mates; m++) {
        MatePlane& pl = e->mate[m];
        bk_engine::Span sp(e, 1);
        BK_HIP(hipMemsetAsync(pl.n_list.p, 0, 8 * sizeof(unsigned int), e->stream));
#ifdef BK_TESTING
        if (ix.ablate == 15) BK_HIP(hipMemsetAsync(pl.touch_b.p, 0xff, pl.touch_b.n * 4, e->stream));   // (15: every block counts as touched)
#endif
        bk::launch_expand_touched_blocks(pl.touch_b.p, (uint32_t)((ix.total_cells + 63) / 64), ix.cell_blk.p, pl.touch_v.p, (uint32_t)ix.k,
                                         (uint64_t)ix.n_full + (uint64_t)ix.v_span, e->stream);
        bk::launch_compact_touched(pl.touch_v.p, bk::v_real_rows(ix.n_full, ix.v_span), pl.touch_p.p, ix.n_prows, pl.touch_e.p, ix.n_u,
                                   ix.n_full, pl.v_list.p, pl.p_list.p, pl.e_list.p, pl.n_list.p, e->stream);
    }
    return BK_OK;
}
static bk::FinalizeArgs finalize_args(const bk_engine* e, const FinalizeCall& c, int m, int pass) {
    const IndexTables& ix = *e->ix;
    const MatePlane& pl = e->mate[m];
    bk::FinalizeArgs a{};
    a.ix = ix.view();
    // (a part that came through bk_shard_received lives in its own buffer: element i of the plane is reduced[i - elem_lo])
    a.counters = pl.reduced_shards > 0 ? pl.reduced.p - c.elem_lo : pl.counters.p;
    a.elem_lo = c.elem_lo; a.elem_hi = c.elem_hi; a.ci = e->params.ci; a.cs = e->params.cs; a.cx = e->params.cx; a.pileup = e->pileup.p; a.plane = (size_t)ix.total_cells * 4;
    a.stats = e->stats.p + (size_t)m * ix.n_files * 3; a.present = e->present.p + (size_t)m * ix.n_files; a.kept_total = e->kstats_cur() + m * 4 + 3; a.distinct_total = e->kstats_cur() + m * 4 + 2;
    a.partials = e->fin_partials.p; a.n_deferred = e->n_deferred.p + m;
    a.deferred = e->deferred.p + (c.two_pass ? (size_t)m * (e->deferred.n / 2) : 0);   // (kept from the first pass to the second)
    a.file_cell_lo = ix.file_cell_lo_d.p; a.max_file_cells = (uint32_t)ix.max_file_cells_idx;
    a.deferred_mask = c.two_pass && e->deferred_mask.p ? e->deferred_mask.p + (size_t)m * (e->deferred_mask.n / 2) : nullptr;
    a.ktab_keys = e->ktab.keys.p; a.ktab_cnt = e->ktab.cnt.p; a.ktab_log2 = e->ktab.log2; a.ktab_overflow = e->ktab_out.p + 4; a.mate = (uint32_t)m;
    if (e->sparse) { a.v_list = pl.v_list.p; a.p_list = pl.p_list.p; a.e_list = pl.e_list.p; a.n_list = pl.n_list.p; }
    a.deferred_n = e->deferred_n.p ? e->deferred_n.p + (c.two_pass ? (size_t)m * (e->deferred_n.n / 2) : 0) : nullptr;
    a.clear_v = c.clean_dense && pass == (c.two_pass ? 1 : 0);
    a.mode = c.two_pass ? pass + 1 : c.gather ? (pass == 0 ? 1 : 3) : 0;
    if (c.gather) {
        if (const char* ga = test_env("BK_GATHER_ABLATE")) a.gather_ablate = atoi(ga);
        a.merged_slots = ix.merged_slots.p; a.n_merged_slots = ix.n_merged_slots;
        a.gather = pass == 1 ? 1 : 0; a.alias_hits = pl.alias_hits.p; a.n_alias_hits = e->n_alias_hits.p + m; a.alias_cap = bk_engine::kAliasCap;
    }
    a.sel = c.two_pass ? &e->sel_out.p->file_id : nullptr; a.sel_file = -1;
    // dense planes mapped whole: K2a zeroes the V counters it reads; the E part (two counters per reference k-mer) is zeroed by
    // the reduce kernel of the mate file's last statistics pass (it runs behind K2e, the E part's only reader in that pass;
    // a second, votes-only pass reads it again: then clean_planes' memset does it)
    const bool ride = c.clean_dense && !c.two_pass && e->fin_partials.p && pl.used;
    a.no_lean = test_env("BK_NO_LEAN_FINALIZE") != nullptr; a.lean_list_cap = bk::kLeanListCap;
    if (const char* lc = test_env("BK_LEAN_LIST_CAP")) a.lean_list_cap = (uint32_t)std::max(1, std::min((int)bk::kLeanListCap, atoi(lc)));   // testing aid: a list that a small reference fills
    a.zero_e = ride ? pl.counters.p : nullptr; a.zero_e_n = ride ? (size_t)std::min<uint64_t>(ix.v_off, ix.plane_len) : 0;
    return a;
}
// the end of a whole-sample finalize: what the maps read is zeroed again, so the planes are all zero for the next sample; the
// statistics table's distinct and kept k-mers are counted
static int clean_planes(bk_engine* e, const FinalizeCall& c) {
    const IndexTables& ix = *e->ix;
    for (int m = 0; m < c.n_mates && c.clean_dense; m++) {   // K2a zeroed the V counters; the E part (two counters per reference k-mer) goes here
        MatePlane& pl = e->mate[m];
        if (pl.used) {
            bk_engine::Span sp(e, 2);
            BK_HIP(hipMemsetAsync(pl.counters.p, 0, (size_t)std::min<uint64_t>(ix.v_off, ix.plane_len) * sizeof(unsigned long long), e->stream));
        }
        pl.finalized_clean();
    }
    for (int m = 0; m < c.n_mates && e->sparse; m++) {   // the maps are done: clear_touched zeroes what they read
        MatePlane& pl = e->mate[m];
        bk_engine::Span sp(e, 1);
        bk::launch_clear_touched(pl.counters.p, ix.v_off, bk::v_real_len(ix.n_full, ix.v_span), (uint32_t)ix.v_span + 1u, pl.v_list.p, pl.p_list.p,
                                 pl.e_list.p, pl.n_list.p, ix.n_u, e->stream);
        pl.finalized_clean();
    }
    if (e->ktab.keys.p) { bk_engine::Span sp(e, 1); bk::launch_ktab_stats(e->ktab.keys.p, e->ktab.cnt.p, e->ktab.log2, e->params.ci, e->params.cx, e->ktab_out.p, e->stream); }
    return BK_OK;
}
static int finalize_part(bk_engine* e, int n_mates, uint64_t elem_lo, uint64_t elem_hi) {
    const IndexTables& ix = *e->ix;
    if (!e->in_sample) return fail(BK_ERR_STATE, "bk_sample_finalize called before bk_sample_begin");
    if (n_mates < 1 || n_mates > 2) return fail(BK_ERR_INVALID, "n_mates must be 1 or 2");
    BK_HIP(hipSetDevice(e->device));
    pay_owed_zeros(e);   // (a sample without a Level 2 launch)
    const bool whole = elem_lo == 0 && elem_hi == ix.plane_len;
    const bool via_reduced = e->mate[0].reduced_shards > 0 || e->mate[1].reduced_shards > 0;   // (the planes themselves are not what is mapped: they are zeroed at the next push)
    // bk_params.pileup_selected_only (several genome files): first the statistics of every genome without a single vote, then the
    // genome is selected on the device (call.rs:422-502), then the votes -- only the BucketInfos of that genome.  Gathered votes
    // (bk_gather.hip): the statistics pass as ever, then gather_votes_kernel for the selected genome's cells or for all
    FinalizeCall c{n_mates, elem_lo, elem_hi};
    c.two_pass = e->params.pileup_selected_only != 0 && ix.n_files > 1;
    c.gather = e->gather_mode && whole && !via_reduced;
    c.clean_dense = !e->sparse && whole && !via_reduced;   // (this call maps whole planes: it leaves them zeroed)
    if (c.two_pass && !whole) return fail(BK_ERR_UNSUPPORTED, "pileup_selected_only cannot be combined with a sharded finalize");
    if (e->sparse && !whole) return fail(BK_ERR_UNSUPPORTED, "an index this large cannot be finalized in shards");
    if (e->sparse) { if (int rc = compact_sparse_lists(e, n_mates)) return rc; }
    if (c.gather) BK_HIP(hipMemsetAsync(e->n_alias_hits.p, 0, 2 * sizeof(unsigned int), e->stream));
    auto sync_debug = [e](const char* what) -> int {   // testing build, BK_SYNC_DEBUG: which launch of the gathered voting pass faults
        if (test_env("BK_SYNC_DEBUG")) { fprintf(stderr, "[bk] %s ...", what); BK_HIP(hipStreamSynchronize(e->stream)); fprintf(stderr, " ok\n"); }
        return BK_OK;
    };
    for (int pass = 0; pass < ((c.two_pass || c.gather) ? 2 : 1); pass++) {
        const bool votes = c.gather && pass == 1;
        if (votes) {   // difference arrays -> counts (the rows are zeroed behind the sample)
            bk_engine::Span sp(e, 1);
            if (int rc = sync_debug("statistics pass")) return rc;
            // (every genome's rows by the table of voters, allocated with the engine: which V rows the sample's mate files touched, as bits)
            if (e->row_bits.p) BK_HIP(hipMemsetAsync(e->row_bits.p, 0, e->row_bits.n * sizeof(unsigned int), e->stream));
            for (int m = 0; m < n_mates; m++) bk::launch_prefix_rows(e->mate[m].counters.p, ix.view(), e->mate[m].v_list.p, e->mate[m].n_list.p, e->row_bits.p, e->stream);
            if (int rc = sync_debug("prefix_rows")) return rc;
        }
        for (int m = 0; m < n_mates; m++) {   // R1 then R2 into the same arrays (call.rs:316-317)
            bk::FinalizeArgs a = finalize_args(e, c, m, pass);
            if (a.zero_e) e->mate[m].finalized_clean();   // (this pass's kernels leave the whole plane zeroed)
            if (pass == 0) { if (int rc = e->mate[m].zero_if_stale(e)) return rc; }
            if (e->pending.on && e->pending.mate == m) {
                // the mate file's reads were one launch: the regional finalize takes the V counts from the scan's items
                const bk::BinArgs& pb = e->pending.b;
                a.f_items = pb.items; a.f_tab = pb.tab; a.f_gext = pb.gext; a.f_ov = pb.ov; a.f_ov_n = pb.ov_n; a.f_ov_cap = pb.ov_cap; a.f_ov_par = pb.ov_par;
                a.f_n_wg = pb.n_wg; a.f_ig = pb.ig; a.f_touch = e->mate[m].fuse_touch.p;
                if (c.clean_dense && !c.two_pass && bk::finalize_runs_by_region(a)) { e->pending.on = false; e->mate[m].items_taken(); }
                else { a.f_items = nullptr; if (int rc = flush_pending_items(e)) return rc; }
            }
            bk_engine::Span sp(e, 1);
            if (votes && m == 0) {   // (both mate files' counts at once: it stores)
                const unsigned long long* c1 = n_mates == 2 ? e->mate[1].counters.p : nullptr;
                // many genomes that share their k-mers: the voters once per (k-mer, window position), not once per occurrence
                if (bk::vote_table_fits(a) && e->row_bits.p && e->vote_tab.n >= bk::vote_table_words(a.ix)) bk::launch_gather_votes_table(a, c1, e->vote_tab.p, e->row_bits.p, e->stream);
                else bk::launch_gather_votes(a, c1, e->stream);
                if (int rc = sync_debug("gather_votes")) return rc;
            }
            if (votes && ix.n_merged_slots) { bk::launch_merged_votes(a, e->stream); if (int rc = sync_debug("merged_votes")) return rc; }
            bk::launch_finalize(a, e->stream);
            if (votes) if (int rc = sync_debug("alias-only general kernels")) return rc;
        }
        if (c.two_pass && pass == 0) {
            bk::CallArgs s{};
            s.n_files = ix.n_files; s.n_mates = n_mates; s.stats = e->stats.p; s.present = e->present.p; s.genome_len = ix.genome_len.p; s.out = e->sel_out.p;
            bk_engine::Span sp(e, 1);
            bk::launch_select_genome(s, e->stream);
            if (c.gather) bk::launch_copy_int(e->last_sel.p, &e->sel_out.p->file_id, e->stream);   // (the rows the next sample zeroes)
        }
    }
    if (int rc = clean_planes(e, c)) return rc;
    BK_HIP(hipGetLastError());
    e->in_sample = false; e->finalized_mates = n_mates;
    return l2_stats_report(e);
}

int bk_sample_finalize(bk_engine* e, int n_mates) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (e->mate[0].reduced_shards > 1 || e->mate[1].reduced_shards > 1) return fail(BK_ERR_STATE, "this sample's planes went through bk_shard_transport: finalize it with bk_sample_finalize_shard");
    int rc = finalize_part(e, n_mates, 0, e->ix->plane_len);
    if (rc == BK_OK && e->dump) rc = e->dump->finalize(e, n_mates);
    return rc;
}

int bk_sample_finalize_shard(bk_engine* e, int n_mates, int shard, int n_shards) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (n_shards < 1 || (int)bk::kMaxShards % n_shards != 0 || shard < 0 || shard >= n_shards)
        return fail(BK_ERR_INVALID, "n_shards must divide %u and 0 <= shard < n_shards", bk::kMaxShards);
    if (e->ktab.keys.p && n_shards > 1 && !e->ktab_exchanged)
        return fail(BK_ERR_STATE, "full_kmer_stats with a sharded finalize: exchange the ranks' k-mer statistics tables first "
                                  "(bk_kmer_table_partition, all-to-all, bk_kmer_table_replace)");
    const uint64_t part = e->ix->plane_len / (uint64_t)n_shards;
    for (int m = 0; m < n_mates; m++)
        if (e->mate[m].reduced_shards > 0 && (e->mate[m].reduced_shards != n_shards || e->mate[m].reduced_shard != shard))
            return fail(BK_ERR_STATE, "bk_sample_finalize_shard(%d of %d): mate file %d received part %d of %d (bk_shard_received)", shard, n_shards, m,
                        e->mate[m].reduced_shard, e->mate[m].reduced_shards);
    int rc = finalize_part(e, n_mates, part * shard, part * (shard + 1));
    if (rc != BK_OK) return rc;
    if (e->ktab.keys.p) bk::launch_ktab_totals_to_kstats(e->ktab_out.p, e->kstats_cur(), n_mates, e->stream);   // (the ranks' totals add up)
    for (int m = 0; m < n_mates; m++) {   // the records this rank pushed join the device tally, so that the sum over ranks is the sample's
        if (e->mate[m].pushed_records) bk::launch_add_const_u64(e->kstats_cur() + m * 4 + 0, e->mate[m].pushed_records, e->stream);
        e->mate[m].pushed_records = 0;
    }
    bk::launch_pack_sums(e->shard_sums.p, e->stats.p, e->present.p, e->kstats_cur(), e->ix->n_files, e->xport_flag.p, e->stream);
    BK_HIP(hipGetLastError());
    return BK_OK;
}

int bk_kmer_table_partition(bk_engine* e, int n_parts, void** d_keys, void** d_counts, uint64_t* part_off) {
    if (!e || !d_keys || !d_counts || !part_off) return fail(BK_ERR_INVALID, "null argument");
    if (n_parts < 1 || n_parts > (int)bk::kMaxShards) return fail(BK_ERR_INVALID, "1 <= n_parts <= %u", bk::kMaxShards);
    if (!e->ktab.keys.p) return fail(BK_ERR_STATE, "the engine was created without full_kmer_stats");
    if (!e->in_sample) return fail(BK_ERR_STATE, "bk_kmer_table_partition comes between the pushes and the finalize of a sample");
    BK_HIP(hipSetDevice(e->device));
    if (!e->xchg_cursors.p) BK_HIP(e->xchg_cursors.alloc(bk::kMaxShards));
    BK_HIP(hipMemsetAsync(e->xchg_cursors.p, 0, bk::kMaxShards * sizeof(unsigned long long), e->stream));
    bk::launch_ktab_count_parts(e->ktab.keys.p, e->ktab.log2, (uint32_t)n_parts, e->xchg_cursors.p, e->stream);
    unsigned long long counts[bk::kMaxShards];
    if (int rc = download(e, counts, e->xchg_cursors.p, (size_t)n_parts)) return rc;
    unsigned long long first[bk::kMaxShards];
    part_off[0] = 0;
    for (int r = 0; r < n_parts; r++) { first[r] = part_off[r]; part_off[r + 1] = part_off[r] + counts[r]; }
    const uint64_t total = part_off[n_parts];
    if (e->xchg_keys.n < total || !e->xchg_keys.p) {
        BK_HIP(e->xchg_keys.alloc(std::max<uint64_t>(total + total / 4, 1024)));
        BK_HIP(e->xchg_cnt.alloc(e->xchg_keys.n));
    }
    BK_HIP(hipMemcpyAsync(e->xchg_cursors.p, first, (size_t)n_parts * sizeof(unsigned long long), hipMemcpyHostToDevice, e->stream));
    bk::launch_ktab_scatter_parts(e->ktab.keys.p, e->ktab.cnt.p, e->ktab.log2, (uint32_t)n_parts, e->xchg_cursors.p, e->xchg_keys.p, e->xchg_cnt.p, e->stream);
    BK_HIP(hipGetLastError());
    BK_HIP(hipStreamSynchronize(e->stream));   // (`first` is read by the copy above; the caller reads the arrays on its own stream)
    *d_keys = e->xchg_keys.p; *d_counts = e->xchg_cnt.p;
    return BK_OK;
}

int bk_kmer_table_replace(bk_engine* e, const void* d_keys, const void* d_counts, uint64_t n) {
    if (!e || (n && (!d_keys || !d_counts))) return fail(BK_ERR_INVALID, "null argument");
    if (!e->ktab.keys.p) return fail(BK_ERR_STATE, "the engine was created without full_kmer_stats");
    if (!e->in_sample) return fail(BK_ERR_STATE, "bk_kmer_table_replace comes between the pushes and the finalize of a sample");
    BK_HIP(hipSetDevice(e->device));
    // an empty table with room for the n entries (and, like after any push, for what finalize adds: the load stays below a half)
    BK_HIP(hipMemsetAsync(e->ktab.keys.p, 0xff, e->ktab.keys.n * sizeof(unsigned long long), e->stream));
    BK_HIP(hipMemsetAsync(e->ktab.cnt.p, 0, e->ktab.cnt.n * sizeof(unsigned int), e->stream));
    BK_HIP(hipMemsetAsync(e->ktab_out.p + 8, 0, bk::ktab_fill_words() * sizeof(unsigned long long), e->stream));
    if (e->ktab.fill_pending) { BK_HIP(hipEventSynchronize(e->ktab.fill_ev)); e->ktab.fill_pending = false; }
    e->ktab.fill_known = 0; e->ktab.fill_unknown_upper = 0;
    if (int rc = e->ktab.ensure_room(e, e->ktab_out.p, n)) return rc;
    bk::launch_ktab_import(static_cast<const unsigned long long*>(d_keys), static_cast<const unsigned int*>(d_counts), n, e->ktab.keys.p, e->ktab.cnt.p,
                           e->ktab.log2, e->ktab_out.p + 4, e->stream);
    BK_HIP(hipGetLastError());
    e->ktab_exchanged = true;
    return e->ktab.note_fill(e, e->ktab_out.p);
}

int bk_shard_sums_device_ptr(bk_engine* e, void** d_ptr, uint64_t* len) {
    if (!e || !d_ptr || !len) return fail(BK_ERR_INVALID, "null argument");
    *d_ptr = e->shard_sums.p;
    *len = (uint64_t)2 * e->ix->n_files * 5 + 9;
    return BK_OK;
}

int bk_sample_merge_shards(bk_engine* e) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    BK_HIP(hipSetDevice(e->device));
    pay_owed_zeros(e);
    bk::launch_unpack_sums(e->shard_sums.p, e->stats.p, e->present.p, e->kstats_cur(), e->ix->n_files, e->xport_flag.p, e->stream);
    BK_HIP(hipGetLastError());
    return BK_OK;
}

static int shard_args_ok(bk_engine* e, int mate, int n_shards, int width) {
    if (!e || mate < 0 || mate > 1) return fail(BK_ERR_INVALID, "bad argument");
    if (n_shards < 1 || (int)bk::kMaxShards % n_shards != 0) return fail(BK_ERR_INVALID, "n_shards must divide %u", bk::kMaxShards);
    if (width != 16 && width != 32 && width != 64) return fail(BK_ERR_INVALID, "width must be 16, 32 or 64");
    if (e->sparse) return fail(BK_ERR_UNSUPPORTED, "an index this large keeps its counter planes sparse: shard whole samples over GPUs, not one sample's reads");
    if (!e->in_sample) return fail(BK_ERR_STATE, "the transport of a plane comes between the pushes and the finalize of a sample");
    return BK_OK;
}

int bk_shard_measure(bk_engine* e, int mate, void** d_max) {
    if (!d_max) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = shard_args_ok(e, mate, 1, 64)) return rc;
    BK_HIP(hipSetDevice(e->device));
    if (int rc = flush_pending_items(e)) return rc;
    if (int rc = e->mate[mate].zero_if_stale(e)) return rc;
    BK_HIP(hipMemsetAsync(e->xport_flag.p + 2, 0, 2 * sizeof(unsigned long long), e->stream));
    bk::launch_xport_measure(e->mate[mate].counters.p, e->ix->plane_len, e->ix->v_off, e->xport_flag.p + 2, e->stream);
    BK_HIP(hipGetLastError());
    *d_max = e->xport_flag.p + 2;
    return BK_OK;
}

int bk_shard_transport(bk_engine* e, int mate, int n_shards, int width, void** d_send, uint64_t* part_bytes, void** d_recv) {
    if (!d_send || !part_bytes || !d_recv) return fail(BK_ERR_INVALID, "null argument");
    if (int rc = shard_args_ok(e, mate, n_shards, width)) return rc;
    const IndexTables& ix = *e->ix;
    BK_HIP(hipSetDevice(e->device));
    if (int rc = flush_pending_items(e)) return rc;
    if (int rc = e->mate[mate].zero_if_stale(e)) return rc;   // (a mate file nothing was pushed for: its plane is zeroed lazily -- now)
    e->mate[mate].written();
    e->xport_ever = true;
    if (e->mate[0].reduced_shards == 0 && e->mate[1].reduced_shards == 0)   // first transport of this sample
        BK_HIP(hipMemsetAsync(e->xport_flag.p, 0, sizeof(unsigned long long), e->stream));
    const uint64_t pb = bk::xport_part_bytes(ix.plane_len, ix.v_off, (uint32_t)n_shards, width);
    // Width 16 spends four lanes on an E count: with many shards (or a plane that is mostly E counts) its part is no smaller than
    // the 32-bit one -- it would send more, not less.  Refused, so that nobody packs a plane for nothing ("auto" falls back on 32).
    if (width == 16 && pb >= bk::xport_part_bytes(ix.plane_len, ix.v_off, (uint32_t)n_shards, 32))
        return fail(BK_ERR_INVALID, "width 16 does not shrink the plane at %d shards (every E count takes four 16-bit lanes): use width 32", n_shards);
    // The buffers are sized ONCE, for the worst case over every shard count and width (the whole plane for `reduced`; the
    // largest packed plane and part for the transport), and stay where they are for the engine's lifetime: a host may keep views.
    if (e->mate[mate].reduced.n < ix.plane_len) {
        BK_HIP(hipStreamSynchronize(e->stream));
        BK_HIP(e->mate[mate].reduced.alloc(ix.plane_len));
    }
    *part_bytes = pb;
    if (width == 64) {   // nothing to pack: the plane itself is the send buffer and the received part is the reduced part
        *d_send = e->mate[mate].counters.p;
        *d_recv = e->mate[mate].reduced.p;
        return BK_OK;
    }
    if (!e->xport_send.p) {
        uint64_t max_part = 0, max_all = 0;
        for (uint32_t n = 1; n <= bk::kMaxShards; n *= 2)
            for (int w : {16, 32}) {
                const uint64_t b = bk::xport_part_bytes(ix.plane_len, ix.v_off, n, w);
                max_part = std::max(max_part, b);
                max_all = std::max(max_all, b * n);
            }
        BK_HIP(hipStreamSynchronize(e->stream));
        BK_HIP(e->xport_send.alloc(max_all));
        BK_HIP(e->xport_recv.alloc(max_part));
    }
    bk_engine::Span sp(e, 2);
    bk::launch_xport_pack(e->mate[mate].counters.p, ix.plane_len, ix.v_off, (uint32_t)n_shards, width, e->xport_send.p, e->xport_flag.p, e->stream);
    BK_HIP(hipGetLastError());
    *d_send = e->xport_send.p;
    *d_recv = e->xport_recv.p;
    return BK_OK;
}

int bk_shard_received(bk_engine* e, int mate, int shard, int n_shards, int width) {
    if (int rc = shard_args_ok(e, mate, n_shards, width)) return rc;
    if (shard < 0 || shard >= n_shards) return fail(BK_ERR_INVALID, "0 <= shard < n_shards");
    const uint64_t part = e->ix->plane_len / (uint64_t)n_shards;
    if (e->mate[mate].reduced.n < part || (width != 64 && !e->xport_recv.p)) return fail(BK_ERR_STATE, "bk_shard_received without bk_shard_transport");
    BK_HIP(hipSetDevice(e->device));
    if (width != 64) {
        bk_engine::Span sp(e, 2);
        bk::launch_xport_unpack(e->xport_recv.p, e->ix->plane_len, e->ix->v_off, (uint32_t)n_shards, (uint32_t)shard, width, e->mate[mate].reduced.p, e->stream);
        BK_HIP(hipGetLastError());
    }
    e->mate[mate].reduced_shards = n_shards;
    e->mate[mate].reduced_shard = shard;
    return BK_OK;
}

int bk_transport_overflow(bk_engine* e, int* overflowed) {
    if (!e || !overflowed) return fail(BK_ERR_INVALID, "null argument");
    BK_HIP(hipSetDevice(e->device));
    unsigned long long f[2] = {0, 0};
    BK_HIP(hipMemcpyAsync(f, e->xport_flag.p, sizeof f, hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipMemsetAsync(e->xport_flag.p + 1, 0, sizeof(unsigned long long), e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    *overflowed = f[1] != 0;
    return BK_OK;
}

int bk_sample_download(bk_engine* e, int n_mates, uint64_t* fwd_depth, uint64_t* rev_depth, uint64_t* fwd_nk, uint64_t* rev_nk,
                       uint64_t* stats, uint8_t* present, uint64_t* kmer_stats) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    if (n_mates < 1 || n_mates > 2) return fail(BK_ERR_INVALID, "n_mates must be 1 or 2");
    BK_HIP(hipSetDevice(e->device));
    pay_owed_zeros(e);   // (a sample begun and not finalized reads zero, as ever)
    const size_t plane = (size_t)e->ix->total_cells * 4;
    uint64_t* dst[4] = {fwd_depth, rev_depth, fwd_nk, rev_nk};
    {
        bk_engine::Span sp(e, 2);
        for (int i = 0; i < 4; i++)
            if (dst[i] && plane) BK_HIP(hipMemcpyAsync(dst[i], e->pileup.p + (size_t)i * plane, plane * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
        if (stats) BK_HIP(hipMemcpyAsync(stats, e->stats.p, (size_t)n_mates * e->ix->n_files * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
        if (present) BK_HIP(hipMemcpyAsync(present, e->present.p, (size_t)n_mates * e->ix->n_files, hipMemcpyDeviceToHost, e->stream));
        if (kmer_stats) BK_HIP(hipMemcpyAsync(kmer_stats, e->kstats_cur(), (size_t)n_mates * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    }
    unsigned long long kt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (kmer_stats) BK_HIP(hipMemcpyAsync(kt, e->ktab_out.p, sizeof kt, hipMemcpyDeviceToHost, e->stream));
    unsigned long long xf = 0;
    if (e->xport_ever) {
        BK_HIP(hipMemcpyAsync(&xf, e->xport_flag.p + 1, sizeof xf, hipMemcpyDeviceToHost, e->stream));
        BK_HIP(hipMemsetAsync(e->xport_flag.p + 1, 0, sizeof xf, e->stream));
    }
    unsigned int ah[2] = {0u, 0u};
    if (e->gather_mode) BK_HIP(hipMemcpyAsync(ah, e->n_alias_hits.p, sizeof ah, hipMemcpyDeviceToHost, e->stream));
    BK_HIP(hipStreamSynchronize(e->stream));
    if (ah[0] > bk_engine::kAliasCap || ah[1] > bk_engine::kAliasCap)
        return fail(BK_ERR_RANGE, "more than %u k-mers of this sample reach a bucket through the 64-bit wrap of its id: the list of them overflowed, the pileup is incomplete", bk_engine::kAliasCap);
    if (xf) return fail(BK_ERR_RANGE, "a counter of this (or an earlier, unchecked) sample did not fit the width its plane was exchanged at: the results are "
                                      "invalid -- repeat the sample with a wider bk_shard_transport (bk_shard_measure tells which width is safe)");
    if (kmer_stats) {
        for (int m = 0; m < n_mates; m++) {
            kmer_stats[m * 4 + 0] += e->mate[m].pushed_records;   // + the device-side tally of bk_push_reads_ascii batches
            if (e->ktab.keys.p) {
                // index-touching k-mers are in the counter plane (kept tally in [3], distinct tally in [2] by finalize);
                // the rest are in the hash table
                if (kt[4] || kmer_stats[m * 4 + 2] >= (1ull << 56)) { kmer_stats[m * 4 + 2] = kmer_stats[m * 4 + 3] = ~0ull; }   // (2^56: a rank's table overflowed, sharded finalize)
                else { kmer_stats[m * 4 + 2] += kt[m * 2 + 0]; kmer_stats[m * 4 + 3] += kt[m * 2 + 1]; }
            } else {
                kmer_stats[m * 4 + 2] = 0;
            }
        }
    }
    return BK_OK;
}

int bk_sample_finish(bk_engine* e, int n_mates, uint64_t* fwd_depth, uint64_t* rev_depth, uint64_t* fwd_nk, uint64_t* rev_nk,
                     uint64_t* stats, uint8_t* present, uint64_t* kmer_stats) {
    int rc = bk_sample_finalize(e, n_mates);
    if (rc != BK_OK) return rc;
    return bk_sample_download(e, n_mates, fwd_depth, rev_depth, fwd_nk, rev_nk, stats, present, kmer_stats);
}

// ---- measurement ---------------------------------------------------------------------------------------------
int bk_timing_enable(bk_engine* e, int on) {
    if (!e) return fail(BK_ERR_INVALID, "null engine");
    e->timing = on != 0;
    e->timing_kinds = (on & 0xff) == 1 ? 0xfu : (unsigned)(on >> 1) & 0xfu;   // on = 1: all kinds; otherwise bit (1 + kind) selects a kind
    e->timing_every = std::max(1u, ((unsigned)on >> 8) & 0xffu);                // bits 8..15: every N-th launch of a kind only
    for (auto& c : e->timing_seen) c = 0;
    return BK_OK;
}

int bk_timing_read(bk_engine* e, double ms[4], uint64_t n[4], int reset) {
    if (!e || !ms || !n) return fail(BK_ERR_INVALID, "bad argument");
    BK_HIP(hipSetDevice(e->device));
    BK_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < 4; i++) { ms[i] = 0.0; n[i] = 0; }
    for (auto& s : e->spans) {
        float t = 0.f;
        BK_HIP(hipEventElapsedTime(&t, s.a, s.b));
        ms[s.kind] += t;
        n[s.kind] += 1;
    }
    if (reset) {
        for (auto& s : e->spans) { e->free_events.push_back(s.a); e->free_events.push_back(s.b); }
        e->spans.clear();
    }
    return BK_OK;
}

}  // extern "C"
