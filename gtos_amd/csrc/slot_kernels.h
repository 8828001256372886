// The fixed-slot decode contract every device-resident decoder shares (csrc/beam.hip, csrc/sample.hip), written so that the SAME code
// compiles for the host; the device half (the register top-k pass, the next-input write) is csrc/slot_device.h.
//
// Slots: B graphs of k slots each, N = B*k; slot s belongs to graph s / k.  A decoder launches once per step t for all N slots,
// whether they are live or not; what a slot holds (a beam hypothesis, an independent sample) is the decoder's.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GTOS_SLOT_HD __host__ __device__ inline
#else
#define GTOS_SLOT_HD inline
#endif

namespace gtos_slot {

// string class of an output id, from the per-batch tables of Generator.search_tables (Beam.advance compares the STRING with
// <UNK> / <END>)
enum { TOK_PLAIN = 0, TOK_UNK = 1, TOK_END = 2 };

// Output ids < V index the shared tables (the predictable-token vocabulary); ids in [V, tot) are copy ids and index graph b's row
// of the local tables [B, tot-V]
GTOS_SLOT_HD int64_t local_index(int V, int tot, int b, int id) { return (int64_t)b * (tot - V) + (id - V); }

GTOS_SLOT_HD uint8_t token_flag(const uint8_t* flag_shared, const uint8_t* flag_local, int V, int tot, int b, int id) {
    return id < V ? flag_shared[id] : flag_local[local_index(V, tot, b, id)];
}

// (fp32 ll, column) a ranks before b: larger ll first, equal ll lower column first
GTOS_SLOT_HD bool before(float va, int ca, float vb, int cb) { return va > vb || (va == vb && ca < cb); }

// active int32 [3] rotates the "some slot goes on" flag between steps (initially {1, 0, 0}): step t runs only if the word it reads
// is set, ORs its own answer into the word step t + 1 reads, and clears the word step t + 2 will set.  A step that does not run
// (the host loop would have stopped) changes nothing else, and the flag stays 0 from then on.
GTOS_SLOT_HD int active_read(int t) { return t % 3; }
GTOS_SLOT_HD int active_set(int t) { return (t + 1) % 3; }
GTOS_SLOT_HD int active_clear(int t) { return (t + 2) % 3; }

}  // namespace gtos_slot
