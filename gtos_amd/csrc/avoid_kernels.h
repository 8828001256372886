// Negative constraints of the fixed-slot decoders (csrc/avoid.hip): words and phrases a graph's output must not hold, written so
// that the SAME code compiles for the host: tests/test_avoid_block.py builds it with g++ and compares banned_serial with a brute-force
// statement of the rule on random histories.  The kernel runs the same per-position helper, one pattern position per lane.
//
// The rule (the negative constraints of Post & Vilar 2018 / Hu et al. 2019): graph b has a list of avoid entries, each a non-empty
// sequence of output ids p[0, L).  A hypothesis that has generated y[0, t) may not take column w at step t if some entry has
// p[L-1] == w and y[t-L+1 .. t-1] == p[0 .. L-2]: appending w would complete the entry.  With L = 1 the condition is empty and the
// word is banned at every step, step 0 included.  Banned means the column's ll becomes -inf before any selection, exactly as in
// csrc/ngram_kernels.h; nothing else changes.
//
// The state: no history is scanned.  The entries of a graph are concatenated into pat[0, n_pos), n_pos <= MAX_POS = 64 (one wave),
// INIT has a bit at the first position of every entry and LAST at the last one, and a hypothesis carries one 64-bit word D of the
// multi-pattern shift-and matcher (Bitap): bit i is set iff the hypothesis ends in pat[start(i) .. i], start(i) the first position
// of the entry that holds i.  Taking token w gives D' = ((D << 1) | INIT) & MASK(w), MASK(w) having bit i set iff pat[i] == w (a
// bit shifted out of one entry into the next lands on a first position, where INIT is set anyway); the positions that could be
// matched next are (D' << 1) | INIT, and those of them that end an entry, & LAST, ban their pat[i].
#pragma once
#include "slot_kernels.h"

namespace gtos_avoid {

using namespace gtos_slot;              // the active[3] rotation

// Pattern positions per graph: one per lane of a wave, one per bit of the state word
constexpr int MAX_POS = 64;

// MASK(w) by one thread (the host check; the kernel takes it as one wave ballot of pat[lane] == w)
GTOS_SLOT_HD uint64_t mask_serial(const int* pat, int n_pos, int w) {
    uint64_t m = 0;
    for (int i = 0; i < n_pos && i < MAX_POS; ++i)
        if (pat[i] == w) m |= (uint64_t)1 << i;
    return m;
}

// The state after taking a token with mask MASK(w), from the parent's state
GTOS_SLOT_HD uint64_t next_state(uint64_t d_parent, uint64_t init, uint64_t mask) { return ((d_parent << 1) | init) & mask; }

// The positions whose id a hypothesis in state d may not take next
GTOS_SLOT_HD uint64_t ban_word(uint64_t d, uint64_t init, uint64_t last) { return ((d << 1) | init) & last; }

// Position i, holding id pat_i: the id it bans under the ban word, or -1
GTOS_SLOT_HD int ban_at(uint64_t ban, int i, int pat_i) { return i >= 0 && i < MAX_POS && ((ban >> i) & 1) ? pat_i : -1; }

// The whole row by one thread (the host check; the kernel gives every position a lane): the banned ids of state d in position
// order, repeats included, into out [n_pos].  Returns how many.
GTOS_SLOT_HD int banned_serial(const int* pat, int n_pos, uint64_t d, uint64_t init, uint64_t last, int* out) {
    const uint64_t ban = ban_word(d, init, last);
    int m = 0;
    for (int i = 0; i < n_pos && i < MAX_POS; ++i) {
        const int id = ban_at(ban, i, pat[i]);
        if (id >= 0) out[m++] = id;
    }
    return m;
}

}  // namespace gtos_avoid
