// Repeat-n-gram blocking of the fixed-slot decoders (csrc/ngram.hip), written so that the SAME code compiles for the host:
// tests/test_ngram_block.py builds it with g++ and compares banned_serial with a brute-force statement of the rule on random
// histories.  The kernel runs the same per-position helper, one history position per lane.
//
// The rule (fairseq's --no-repeat-ngram-size): a hypothesis has generated y[0, t) (output ids; <STR> is not counted, <END> never
// occurs in a live hypothesis) and n >= 1 is the blocked n-gram size.  If t >= n - 1, then for every i in [0, t - n] with
// y[i .. i+n-2] == y[t-n+1 .. t-1] the column y[i+n-1] of the hypothesis' ll row is banned: appending it would repeat the n-gram
// that starts at i.  With n = 1 the condition is empty and every token generated so far is banned.  Banned means the column's ll
// becomes -inf before any selection (the top-k of the beam search, rule 1 of csrc/sample_kernels.h); nothing else changes.
#pragma once
#include "slot_kernels.h"

#define GTOS_NGRAM_HD GTOS_SLOT_HD

namespace gtos_ngram {

using namespace gtos_slot;              // the active[3] rotation

// The longest history a launch takes: the kernel stages one int32 row of max_time_step entries in LDS, 16 KiB of the 64 KiB a
// workgroup may declare statically.
constexpr int MAX_T = 4096;

// Position i of the history y[0, t): the id it bans, or -1.  Positions past t - n ban nothing (no whole n-gram starts there).
GTOS_NGRAM_HD int ban_at(const int* y, int t, int n, int i) {
    if (i < 0 || i > t - n) return -1;
    const int* suffix = y + (t - n + 1);        // the n - 1 last tokens
    for (int j = 0; j < n - 1; ++j)
        if (y[i + j] != suffix[j]) return -1;
    return y[i + n - 1];
}

// The whole row by one thread (the host check; the kernel spreads the positions over a workgroup): the banned ids of y[0, t) in
// position order, repeats included, into out [t].  Returns how many.
GTOS_NGRAM_HD int banned_serial(const int* y, int t, int n, int* out) {
    int m = 0;
    for (int i = 0; i + n <= t; ++i) {
        const int id = ban_at(y, t, n, i);
        if (id >= 0) out[m++] = id;
    }
    return m;
}

}  // namespace gtos_ngram
