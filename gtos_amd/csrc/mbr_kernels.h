// All-pairs clipped n-gram overlap inside groups of candidates (csrc/mbr.hip: the count under minimum-Bayes-risk selection,
// gtos_amd.metrics.pairwise / mbr_select), written so that the SAME code compiles for the host: tests/test_mbr.py builds it with
// g++ and compares group_serial with a Counter statement of the rule, for equality.
//
// Input.  R rows of int32 symbols in CSR form (sym, off [R+1]) as for gtos_ngram_overlap, and grp [G+1], non-decreasing row offsets:
// group g holds the rows grp[g] .. grp[g+1], n_g of them (0 is legal).  Output int32 [cells, n_max, 3] with cells = sum n_g^2: the
// cell of (hypothesis i, reference j) of group g -- i, j counted inside the group -- sits at cell_off[g] + i * n_g + j, cell_off the
// running sum of n_g^2 (cell_offsets below, int64).  Every cell holds what gtos_ngram_overlap stores for the pair (row i, row j):
// per order the clipped matches, the hypothesis n-grams, the reference n-grams (overlap_kernels.h).
//
// Two facts of that rule carry the kernel.
//   1. position_counts decides "position i counts iff earlier_i < inref_i".  earlier_i looks at the hypothesis alone, so it is computed
//      once per candidate and serves every reference the candidate meets.  earlier_counts and inref_counts below are the two scans of
//      position_counts, taken apart and otherwise unchanged; position_matches is its last line.  Together they RESTATE
//      position_counts (tests/test_mbr.py compares the two on random inputs).
//   2. The clipped count sum_g min(count_a(g), count_b(g)) is symmetric: cells (i, j) and (j, i) hold the same matches and differ in
//      which side's n-gram totals stand in columns 1 and 2.  The diagonal needs no scan: matches = n_grams(L, n).
// So candidate i scans only the half circle of its group (scan_count / scan_ref) and stores both mirrored cells of every scan plus
// its own diagonal cell: every ordered cell has exactly one owner, nothing is accumulated across workgroups, two launches store
// identical values.
#pragma once
#include "overlap_kernels.h"

namespace gtos_mbr {

using gtos_overlap::MAX_ORDER;
using gtos_overlap::STATS;
using gtos_overlap::common_prefix;
using gtos_overlap::n_grams;

constexpr int MAX_GROUP = 64;               // candidates per group: the group's row offsets sit in LDS
// Symbols per row (a sentence of 100 tokens is ~600 characters).  At 256 threads a thread owns at most 4 positions, and a count of
// earlier positions is below 1024: the 8 per-order counts of a position pack into three 32-bit registers, 10 bits each.
constexpr int GROUP_MAX_SYMBOLS = 1024;
constexpr int64_t MAX_OUT = 2147483647;     // the kernel indexes the output with int32: cells * n_max * 3 may not exceed it

// earlier[n - 1] = the number of positions j < i of h that hold the n-gram starting at i, n = 1 .. n_max (0 for the orders with no
// whole n-gram at i and from n_max on): the second scan of position_counts.
GTOS_OVERLAP_HD void earlier_counts(const int* h, int Lh, int n_max, int i, int (&earlier)[MAX_ORDER]) {
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) earlier[n] = 0;
    const int orders = n_max < Lh - i ? n_max : Lh - i;
    const int first = h[i];
    for (int j = 0; j < i; ++j) {                                // Lh - j > Lh - i: the cap is position i's own
        if (h[j] != first) continue;
        const int c = 1 + common_prefix(h + i + 1, h + j + 1, orders - 1);
#pragma unroll
        for (int n = 0; n < MAX_ORDER; ++n) earlier[n] += n < c;
    }
}

// inref[n - 1] = the number of positions of r that hold the n-gram starting at position i of h: the first scan of position_counts.
GTOS_OVERLAP_HD void inref_counts(const int* h, int Lh, const int* r, int Lr, int n_max, int i, int (&inref)[MAX_ORDER]) {
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) inref[n] = 0;
    const int orders = n_max < Lh - i ? n_max : Lh - i;
    const int first = h[i];
    for (int j = 0; j < Lr; ++j) {
        if (r[j] != first) continue;
        const int cap = orders < Lr - j ? orders : Lr - j;
        const int c = 1 + common_prefix(h + i + 1, r + j + 1, cap - 1);
#pragma unroll
        for (int n = 0; n < MAX_ORDER; ++n) inref[n] += n < c;
    }
}

// The last line of position_counts: counts[n - 1] = 1 iff position i holds a whole n-gram and earlier < inref.
GTOS_OVERLAP_HD void position_matches(int Lh, int n_max, int i, const int (&earlier)[MAX_ORDER], const int (&inref)[MAX_ORDER],
                                      int (&counts)[MAX_ORDER]) {
    const int orders = n_max < Lh - i ? n_max : Lh - i;
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) counts[n] = (n < orders && earlier[n] < inref[n]) ? 1 : 0;
}

// The schedule.  Candidate i of a group of n scans scan_count(i, n) references, the half circle j = i + 1 .. i + n / 2 (mod n); for
// even n the pair at distance n / 2 would be met from both ends and belongs to its lower index only.  Candidate i stores its own
// cell (i, i), and (i, j) and (j, i) for every j it scans.
GTOS_OVERLAP_HD int scan_count(int i, int n) { return (n - 1) / 2 + ((n % 2 == 0 && i < n / 2) ? 1 : 0); }
GTOS_OVERLAP_HD int scan_ref(int i, int n, int k) { return (i + 1 + k) % n; }

// The two mirrored cells of one scanned pair, and the diagonal cell (all [n_max, 3])
GTOS_OVERLAP_HD void store_pair(const int* matches, int Lh, int Lr, int n_max, int* cell_ij, int* cell_ji) {
    for (int n = 0; n < n_max; ++n) {
        cell_ij[n * STATS + 0] = cell_ji[n * STATS + 0] = matches[n];
        cell_ij[n * STATS + 1] = cell_ji[n * STATS + 2] = n_grams(Lh, n + 1);
        cell_ij[n * STATS + 2] = cell_ji[n * STATS + 1] = n_grams(Lr, n + 1);
    }
}

// One whole group by one thread through the helpers above (the host check; the kernel gives every candidate a workgroup and keeps
// earlier[] across the references): rows row0 .. row0 + n of (sym, off) -> cells int32 [n * n, n_max, 3].
GTOS_OVERLAP_HD void group_serial(const int* sym, const int* off, int row0, int n, int n_max, int* cells) {
    const int64_t W = (int64_t)n_max * STATS;
    for (int i = 0; i < n; ++i) {
        const int* h = sym + off[row0 + i];
        const int Lh = off[row0 + i + 1] - off[row0 + i];
        int* diag = cells + ((int64_t)i * n + i) * W;
        for (int m = 0; m < n_max; ++m) diag[m * STATS + 0] = diag[m * STATS + 1] = diag[m * STATS + 2] = n_grams(Lh, m + 1);
        for (int k = 0; k < scan_count(i, n); ++k) {
            const int j = scan_ref(i, n, k);
            const int* r = sym + off[row0 + j];
            const int Lr = off[row0 + j + 1] - off[row0 + j];
            int total[MAX_ORDER];
            for (int m = 0; m < MAX_ORDER; ++m) total[m] = 0;
            for (int p = 0; p < Lh; ++p) {
                int earlier[MAX_ORDER], inref[MAX_ORDER], counts[MAX_ORDER];
                earlier_counts(h, Lh, n_max, p, earlier);
                inref_counts(h, Lh, r, Lr, n_max, p, inref);
                position_matches(Lh, n_max, p, earlier, inref, counts);
                for (int m = 0; m < MAX_ORDER; ++m) total[m] += counts[m];
            }
            store_pair(total, Lh, Lr, n_max, cells + ((int64_t)i * n + j) * W, cells + ((int64_t)j * n + i) * W);
        }
    }
}

// cell_off [G + 1]: the running sum of n_g^2, in int64 (cell_off[G] = cells).  grp as check_groups accepts it.
inline void cell_offsets(const int* grp, int G, int64_t* cell_off) {
    cell_off[0] = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t n = (int64_t)grp[g + 1] - grp[g];
        cell_off[g + 1] = cell_off[g] + n * n;
    }
}

// The arguments a launch takes, checked on the host copies of the row offsets and the group offsets (what the C entry point and the
// host check share): 0, or the C ABI's shape error -10.
inline int check_groups(const int* off, int R, const int* grp, int G, int n_max) {
    if (n_max < 1 || n_max > MAX_ORDER || R < 0 || G < 0) return -10;
    if (grp[0] != 0 || grp[G] != R) return -10;
    int64_t cells = 0;
    for (int g = 0; g < G; ++g) {
        if (grp[g + 1] < grp[g] || grp[g + 1] - grp[g] > MAX_GROUP) return -10;
        const int64_t n = grp[g + 1] - grp[g];
        cells += n * n;
        if (cells * n_max * STATS > MAX_OUT) return -10;
    }
    if (off[0] < 0) return -10;
    for (int q = 0; q < R; ++q)
        if (off[q + 1] < off[q] || off[q + 1] - off[q] > GROUP_MAX_SYMBOLS) return -10;
    return 0;
}

}  // namespace gtos_mbr
