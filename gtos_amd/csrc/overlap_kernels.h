// Clipped n-gram overlap of two symbol sequences (csrc/overlap.hip), written so that the SAME code compiles for the host:
// tests/test_overlap_metrics.py builds it with g++ and compares overlap_serial with a Counter statement of the rule on random
// sequences, for equality.  The kernel runs the same per-position helper, hypothesis positions strided over a workgroup.
//
// The rule.  A hypothesis h[0, Lh) and a reference r[0, Lr) of int32 symbols (word ids for BLEU and the word half of chrF++, code
// points for its character half), orders n = 1 .. n_max <= MAX_ORDER.  Per order:
//   hypothesis n-grams  max(Lh - n + 1, 0), reference n-grams max(Lr - n + 1, 0),
//   matches             sum over the DISTINCT n-grams g of min(count_h(g), count_r(g))       (the clipped count of BLEU and chrF)
// stated without a hash table.  For the hypothesis position i that starts a whole n-gram g_i (i + n <= Lh):
//   earlier_i = the number of positions i' < i that hold the same n-gram,
//   inref_i   = the number of reference positions that hold it,
//   position i counts iff earlier_i < inref_i.
// Of the count_h(g) positions that hold g, in position order, the first min(count_h(g), count_r(g)) count: the sum over i is the
// clipped count.  Nothing is hashed, so nothing can collide: the result is exact integer arithmetic.
//
// One scan serves every order at once: with c = the length of the common prefix of h[i:] and x[j:] (x the reference, or the
// hypothesis itself for earlier_i), capped at the orders position i has, position j holds g_i for exactly the orders n <= c.
#pragma once
#include "slot_kernels.h"

#define GTOS_OVERLAP_HD GTOS_SLOT_HD

namespace gtos_overlap {

constexpr int MAX_ORDER = 8;            // n_max of a launch: the per-order counters of a position live in registers
// The longest sequence of a launch: the kernel stages both int32 rows of a pair in LDS, 2 x 16 KiB of the 64 KiB a workgroup may
// declare statically.  A row of length 0 is legal: all of its counts are 0.
constexpr int MAX_SYMBOLS = 4096;
constexpr int STATS = 3;                // (matches, hypothesis n-grams, reference n-grams) per order

GTOS_OVERLAP_HD int n_grams(int L, int n) { return L - n + 1 > 0 ? L - n + 1 : 0; }

// Length of the common prefix of a[0, cap) and b[0, cap)
GTOS_OVERLAP_HD int common_prefix(const int* a, const int* b, int cap) {
    int c = 0;
    while (c < cap && a[c] == b[c]) ++c;
    return c;
}

// Hypothesis position i in [0, Lh): counts[n - 1] = 1 if the n-gram that starts at i is a clipped match, else 0, for n = 1 .. n_max
// (orders with no whole n-gram at i, and the entries from n_max on: 0).
GTOS_OVERLAP_HD void position_counts(const int* h, int Lh, const int* r, int Lr, int n_max, int i, int (&counts)[MAX_ORDER]) {
    int inref[MAX_ORDER], earlier[MAX_ORDER];
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) inref[n] = earlier[n] = 0;
    const int orders = n_max < Lh - i ? n_max : Lh - i;         // >= 1: the orders with a whole n-gram at i
    const int first = h[i];
    for (int j = 0; j < Lr; ++j) {
        if (r[j] != first) continue;
        const int cap = orders < Lr - j ? orders : Lr - j;
        const int c = 1 + common_prefix(h + i + 1, r + j + 1, cap - 1);
#pragma unroll
        for (int n = 0; n < MAX_ORDER; ++n) inref[n] += n < c;
    }
    for (int j = 0; j < i; ++j) {                                // Lh - j > Lh - i: the cap is position i's own
        if (h[j] != first) continue;
        const int c = 1 + common_prefix(h + i + 1, h + j + 1, orders - 1);
#pragma unroll
        for (int n = 0; n < MAX_ORDER; ++n) earlier[n] += n < c;
    }
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) counts[n] = (n < orders && earlier[n] < inref[n]) ? 1 : 0;
}

// The whole pair by one thread (the host check; the kernel spreads the positions over a workgroup): out [n_max, 3].
GTOS_OVERLAP_HD void overlap_serial(const int* h, int Lh, const int* r, int Lr, int n_max, int* out) {
    int total[MAX_ORDER];
    for (int n = 0; n < MAX_ORDER; ++n) total[n] = 0;
    for (int i = 0; i < Lh; ++i) {
        int counts[MAX_ORDER];
        position_counts(h, Lh, r, Lr, n_max, i, counts);
        for (int n = 0; n < MAX_ORDER; ++n) total[n] += counts[n];
    }
    for (int n = 0; n < n_max; ++n) {
        out[n * STATS + 0] = total[n];
        out[n * STATS + 1] = n_grams(Lh, n + 1);
        out[n * STATS + 2] = n_grams(Lr, n + 1);
    }
}

// The arguments a launch takes, checked on the host copies of the row offsets and the pair list (what the C entry point and the
// host check share): 0, or the C ABI's shape error -10.
GTOS_OVERLAP_HD int check_launch(const int* off, int R, const int* pairs, int64_t P, int n_max) {
    if (n_max < 1 || n_max > MAX_ORDER || R < 0 || P < 0) return -10;
    if (off[0] < 0) return -10;
    for (int q = 0; q < R; ++q)
        if (off[q + 1] < off[q] || off[q + 1] - off[q] > MAX_SYMBOLS) return -10;
    for (int64_t p = 0; p < 2 * P; ++p)
        if (pairs[p] < 0 || pairs[p] >= R) return -10;
    return 0;
}

}  // namespace gtos_overlap
