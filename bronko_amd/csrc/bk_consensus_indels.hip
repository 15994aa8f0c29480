// bk_consensus_indels.hip -- the sample's indels applied to its consensus (bk_sample_consensus_indels; `bronko call --consensus-indels`).
//
// The rule is stated in include/bronko_hip.h and DESIGN.md section CI; bronko_amd/host/consensus_indels.cpp and
// tests/consensus_indels_ref.py restate it.  Both inputs lie on the device: the consensus letters (consensus_kernel) and the indels'
// event table with its prefix-summed span array (bk_indels.hip).  Three passes over the table's slots, each with the event
// report's grid (bk_event_pass.h), none of which writes the table:
//   ci_best_kernel   a slot's event (bk_indel_slot.h) with s = fwd + rev, r = span[cell]; an accepted one raises best[b] to its s on
//                    every boundary b it occupies (atomicMax);
//   ci_ties_kernel   an accepted event adds one to ties[b] where its s is best[b];
//   ci_apply_kernel  an accepted event is applied iff on each of its boundaries best == s and ties == 1: it is the only one with the
//                    largest s there.  The accepted rows are appended with one returning add per wave (as event_report appends), the
//                    letters of an applied deletion become '-' (applied deletions share no boundary, so no cell: plain stores), the
//                    tallies are added once per wave.
// What a pass decides depends on the events alone, not on their slots or on the order of the atomics: a maximum and a count.
// Vector stores and atomics only.
#include "bk_event_pass.h"
#include "bk_indel_slot.h"

namespace bk {
namespace {

struct CiEvent {
    IndelSlot ev;
    uint32_t s, r, last;                 // supporting and reference-spanning records; the last boundary it occupies (the first: ev.cell)
};

// Slot i as an event and whether it is accepted.  false: no event there.
__device__ __forceinline__ bool ci_decode(const ConsensusIndelArgs& a, uint64_t i, CiEvent& c, bool& accepted) {
    accepted = false;
    if (!indel_slot_decode(a.key0[i], a.key1[i], c.ev)) return false;
    c.last = c.ev.cell + (c.ev.kind ? 0u : c.ev.len);
    if (c.last > a.total_cells || c.last < c.ev.cell) return false;   // (no event of the scan's reaches past the genome: best and ties end there)
    c.s = a.counts[2u * i] + a.counts[2u * i + 1u];
    c.r = a.span[c.ev.cell];
    const unsigned long long n = (unsigned long long)c.s + c.r;
    accepted = n >= a.prm.min_depth && (double)c.s >= a.prm.min_freq * (double)n;   // consensus_kernel's compare
    return true;
}

__global__ __launch_bounds__(kEventBlock) void ci_best_kernel(ConsensusIndelArgs a) {
    if (a.out->file_id < 0) return;
    const uint64_t n_slots = 1ull << a.log2n;
    for (uint64_t i = (uint64_t)blockIdx.x * kEventBlock + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * kEventBlock) {
        CiEvent c;
        bool accepted;
        if (!ci_decode(a, i, c, accepted) || !accepted) continue;
        for (uint32_t b = c.ev.cell; b <= c.last; ++b) atomicMax(a.best + b, c.s);
    }
}

__global__ __launch_bounds__(kEventBlock) void ci_ties_kernel(ConsensusIndelArgs a) {
    if (a.out->file_id < 0) return;
    const uint64_t n_slots = 1ull << a.log2n;
    for (uint64_t i = (uint64_t)blockIdx.x * kEventBlock + threadIdx.x; i < n_slots; i += (uint64_t)gridDim.x * kEventBlock) {
        CiEvent c;
        bool accepted;
        if (!ci_decode(a, i, c, accepted) || !accepted) continue;
        for (uint32_t b = c.ev.cell; b <= c.last; ++b)
            if (a.best[b] == c.s) atomicAdd(a.ties + b, 1u);
    }
}

__device__ __forceinline__ void ci_add(uint64_t* tally, unsigned long long v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(tally), v);
}

__global__ __launch_bounds__(kEventBlock) void ci_apply_kernel(ConsensusIndelArgs a) {
    const int file = a.out->file_id;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.summary->file_id = file;
    if (file < 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0 && *a.table_overflow) atomicExch(&a.summary->overflow, 1);   // events were lost before this step
    const uint64_t cell_lo = a.seq_cell[a.seq_first[file]];
    const uint64_t n_slots = 1ull << a.log2n;
    const uint32_t lane = threadIdx.x & 63u;
    ConsensusIndelSummaryDev* const t = a.summary;
    for (uint64_t base = (uint64_t)blockIdx.x * kEventBlock + (threadIdx.x & ~63u); base < n_slots; base += (uint64_t)gridDim.x * kEventBlock) {
        const uint64_t i = base + lane;
        CiEvent c{};
        bool accepted = false;
        const bool there = i < n_slots && ci_decode(a, i, c, accepted);
        const unsigned long long m_there = __ballot(there);
        if (m_there == 0ull) continue;
        bool applied = accepted;
        if (accepted)
            for (uint32_t b = c.ev.cell; b <= c.last; ++b) applied = applied && a.best[b] == c.s && a.ties[b] == 1u;
        const bool del = applied && c.ev.kind == 0u, ins = applied && c.ev.kind != 0u;
        const unsigned long long m_acc = __ballot(accepted), m_app = __ballot(applied), m_del = __ballot(del), m_shift = __ballot(applied && c.ev.len % 3u != 0u);
        const uint32_t del_bases = wave_total(del ? c.ev.len : 0u), ins_bases = wave_total(ins ? c.ev.len : 0u);
        unsigned long long at = 0ull;
        if (lane == 0) {
            ci_add(&t->candidates, (unsigned long long)__popcll(m_there));
            if (m_acc) at = atomicAdd(reinterpret_cast<unsigned long long*>(&t->accepted), (unsigned long long)__popcll(m_acc));
            ci_add(&t->applied, (unsigned long long)__popcll(m_app));
            ci_add(&t->contested, (unsigned long long)__popcll(m_acc & ~m_app));
            ci_add(&t->deletions, (unsigned long long)__popcll(m_del));
            ci_add(&t->insertions, (unsigned long long)__popcll(m_app & ~m_del));
            ci_add(&t->deleted_bases, del_bases);
            ci_add(&t->inserted_bases, ins_bases);
            ci_add(&t->frameshifts, (unsigned long long)__popcll(m_shift));
        }
        at = __shfl(at, 0);
        if (accepted) {
            const uint64_t o = at + lane_prefix(m_acc);
            if (o < (uint64_t)BK_CONSENSUS_INDEL_MAX) {
                ConsensusIndelRecordDev row;
                row.cell = c.ev.cell;
                row.len = c.ev.kind ? -(int32_t)c.ev.len : (int32_t)c.ev.len;
                row.support = c.s; row.ref_span = c.r;
                row.seq = c.ev.seq;
                row.applied = applied ? 1u : 0u; row.pad = 0u;
                a.rows[o] = row;
            } else {
                atomicExch(&t->overflow, 1);   // more accepted events than travel: the download is an error
            }
        }
        if (del && c.ev.cell >= cell_lo) {
            const uint64_t first = c.ev.cell - cell_lo;
            for (uint32_t j = 0; j < c.ev.len; ++j)
                if (first + j < a.n_letters) a.letters[first + j] = (uint8_t)'-';
        }
    }
}

}  // namespace

void launch_consensus_indels(const ConsensusIndelArgs& a, hipStream_t stream) {
    const dim3 grid(event_report_grid(a.log2n)), block(kEventBlock);
    hipLaunchKernelGGL(ci_best_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(ci_ties_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(ci_apply_kernel, grid, block, 0, stream, a);
}

}  // namespace bk
