// bk_indel_slot.h -- a slot of the indels' event table (bk_indels.hip) as an event: the one decoding of its two key words, for the
// report of bk_indels.hip and for the passes of bk_consensus_indels.hip.  The layout is indel_event_insert's: the first word holds
// cell | kind << 32 | (len - 1) << 33 | S's first base << 38, the second S's other bases; a word of all ones is free, and a slot is
// an event once both its words are written.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "bk_anchor.h"

namespace bk {

struct IndelSlot {
    uint32_t cell, kind, len;            // kind 0 a deletion, 1 an insertion; len 1..32
    unsigned long long seq;              // S, base t at bits [2t, 2t + 2) (0 for a deletion)
};

// false: the slot is free, or an event is being written to it
__device__ __forceinline__ bool indel_slot_decode(unsigned long long k0, unsigned long long k1, IndelSlot& s) {
    if (k0 == kEventFreeWord || k1 == kEventFreeWord) return false;
    s.cell = (uint32_t)k0;
    s.kind = (uint32_t)(k0 >> 32) & 1u;
    s.len = ((uint32_t)(k0 >> 33) & 31u) + 1u;
    s.seq = (k1 << 2) | ((k0 >> 38) & 3ull);
    return true;
}

}  // namespace bk
