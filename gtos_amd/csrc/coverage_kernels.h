// Selection rule of the coverage-penalised beam search (csrc/coverage.hip; the GNMT coverage penalty, Wu et al. 2016, eq. 14), written
// so that the SAME code compiles for the host: tests/test_coverage_beam.py builds it with g++ and compares a serial advance
// (advance_serial) with gtos_amd.search.CoverageBeam.advance on random pools.  It is the rule of csrc/beam_kernels.h with another
// ranking key; cand_score, before, rank_of, pool_entry, cut_size, place_cut and the state words are that header's.
//
// Slots as in csrc/slot_kernels.h.  n: the node rows of the graph memory; pad [n, N] (uint8, 1: node i of slot s's graph is padding);
// a_t [N, n] fp32: the alignment weights of step t (TokenGenerator.alignment_layer, the row the copy mechanism reads), known before
// the token of step t is chosen and the same for every candidate of one parent.
//
// Coverage.  cov_t[s, i] = cov_{t-1}[parent_{t-1}(s), i] + a_t[s, i], one fp32 add; before step 0 the coverage is zero and a slot is
// its own parent.  A slot with a negative parent is dead: its row is zero and its penalty 0.
// Penalty.   cp_t[s] = sum over the nodes i that are not padding of (double) logf(fminf(cov_t[s, i], 1.0f) + 1e-12f): the term in
// fp32 (a saturated node gives exactly 0, an untouched one logf(1e-12f)), the sum in fp64 in an order that depends on n alone --
// CP_LANES strided partial sums (lane l: the nodes l, l + CP_LANES, ... in this order), then for o = CP_LANES / 2, CP_LANES / 4, ..., 1
// partial l < o takes partial l + o added to it -- so a row's penalty has the same bits at any slot of any batch.
// Selection. gtos_beam's advance with the pool sorted by
//     key_p = score_p + beta * cp_t[parent slot of p]            (fp64; stable, descending: before())
// Every score written to the tables is the MODEL score, never the key; -inf stays -inf; with beta = 0 the key is the score.
// A survivor records the penalty of its parent at this step: slot_cp for a hypothesis that lives on, comp_cp for a completion.
#pragma once
#include "beam_kernels.h"

#include <math.h>

namespace gtos_coverage {

using namespace gtos_beam;

constexpr int CP_LANES = 256;               // partial sums of a penalty (the workgroup of the device kernel)

// the penalty weight an entry point accepts: finite and >= 0 (false for NaN)
GTOS_BEAM_HD bool beta_ok(double beta) { return beta >= 0.0 && beta < __builtin_inf(); }

// one node's term of the penalty
GTOS_BEAM_HD float cp_term(float cov) { return logf(fminf(cov, 1.0f) + 1e-12f); }

// Python's `score + beta * cp`
GTOS_BEAM_HD double key_of(double score, double beta, double cp) { return score + beta * cp; }

// place_cut's hook of this rule: every survivor records this step's penalty of its parent
struct PenaltyHook {
    const double* cp;
    double* slot_cp;
    double* comp_cp;
    GTOS_BEAM_HD void live(int, int parent, int dst) const { slot_cp[dst] = cp[parent]; }
    GTOS_BEAM_HD void done(int, int parent, int dst) const { comp_cp[dst] = cp[parent]; }
};

// gtos_beam::place that also records the parent's penalty of every survivor: slot_cp [N] next to slot_score, comp_cp [B, k] next to
// comp_score.  cp [N]: this step's penalty of every slot (read at the parents only).
GTOS_BEAM_HD bool place(int b, int k, int min_time_step, int max_time_step, const int* order, int m, const double* pool_score,
                        const int* pool_tok, const uint8_t* pool_flag, int t, int* state, int* bp_parent_t, int* bp_token_t,
                        double* slot_score, int* comp_step, int* comp_parent, double* comp_score, const double* cp, double* slot_cp,
                        double* comp_cp) {
    return place_cut(b * k, k, k, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, t,
                     state + (int64_t)b * BS_WORDS, bp_parent_t, bp_token_t, slot_score, comp_step, comp_parent, comp_score,
                     PenaltyHook{cp, slot_cp, comp_cp});
}

// The whole advance of one beam by one thread (the host check; the kernel parallelises the pool and the ranks).  pool_* are scratch
// arrays of k*k entries, order of k.  Does nothing to a done beam.  Returns place()'s flag (false for a done beam).
GTOS_BEAM_HD bool advance_serial(int b, int k, double beta, int t, int V, int tot, int min_time_step, int max_time_step,
                                 const float* topv, const int* topi, const uint8_t* flag_shared, const uint8_t* flag_local,
                                 double* slot_score, int* state, int* bp_parent_t, int* bp_token_t, int* comp_step, int* comp_parent,
                                 double* comp_score, const double* cp, double* slot_cp, double* comp_cp, double* pool_score,
                                 double* pool_key, int* pool_tok, uint8_t* pool_flag, int* order) {
    const int* st = state + (int64_t)b * BS_WORDS;
    if (st[BS_DONE]) return false;
    const int P = st[BS_NLIVE] * k;
    for (int p = 0; p < P; ++p) {
        pool_entry(b, k, p, topv, topi, slot_score, flag_shared, flag_local, V, tot, pool_score + p, pool_tok + p, pool_flag + p);
        pool_key[p] = key_of(pool_score[p], beta, cp[b * k + p / k]);
    }
    const int m = cut_size(P, k, st[BS_NCOMP]);
    for (int p = 0; p < P; ++p) {
        const int r = rank_of(pool_key, P, p);
        if (r < m) order[r] = p;
    }
    return place(b, k, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, t, state, bp_parent_t, bp_token_t,
                 slot_score, comp_step, comp_parent, comp_score, cp, slot_cp, comp_cp);
}

}  // namespace gtos_coverage
