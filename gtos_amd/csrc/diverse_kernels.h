// Selection rule of the diverse (group) beam search (csrc/diverse.hip; Vijayakumar et al., "Diverse Beam Search", with the Hamming
// penalty), written so that the SAME code compiles for the host: tests/test_diverse_beam.py builds it with g++ and compares a serial
// advance (advance_serial) with gtos_amd.search.GroupBeam.advance on random pools.  It is the rule of csrc/beam_kernels.h applied per
// group; cand_score, before, rank_of, cut_size, place_cut and the state words are that header's.
//
// Slots as in csrc/slot_kernels.h: k per graph, cut into G groups of width g = k / G.  Group j of graph b is "group q = b*G + j": it
// owns slots q*g .. q*g + g - 1 (= b*k + j*g ..), its own state words state[q] = (steps, #completed, #live, done) and rows q*g .. of the
// completion tables (the [B, k] tables of the plain search read as [B, G, g]).  It is a width-g beam of its own: done when
// #completed >= g or steps + 1 >= max_time_step, its live slots after an advance its first #live.  At step 0 only the first slot of
// every group is live.
//
// One step of one graph takes its groups in order j = 0 .. G-1 with a list C of chosen output ids, empty at first.  A done group is
// left alone; a group that is not done but has no live slot has an empty pool: its step is counted, as the plain search counts it
// (G = 1 leaves the tables of beam_kernels.h's advance_serial), and it adds nothing to C.  The pool of group j is the top-k candidates (the whole k, not g) of its live slots in (slot, rank) order, position
// p = i*k + r.  Entry p has the model score m_p = cand_score(slot score, ll, class) and the selection key
//     key_p = m_p - lambda * count(C, id_p)            (fp64; count with multiplicity)
// The pool is sorted by KEY (stable, descending: before()), cut to g - #completed and placed as gtos_beam::place_cut places it; every
// score written to the tables is the MODEL score, never the key, so a hypothesis's score stays its log-likelihood.  The output ids of
// the entries that survive are appended to C in placement order; completions are not.
//
// Why the top-k of a slot is enough: C holds at most k - g ids when a group reads it, and a penalty only lowers keys.  Of a slot's
// whole row at most k - g columns are penalised, so at least g of its k best unpenalised columns keep their key, and every column
// outside the top-k has a key no larger than its model score, which is no larger than those g.  The g best penalised candidates of a
// slot therefore lie within its unpenalised top-k (up to the order of exact ties), the cut takes at most g entries, and the rule
// equals group beam search over the full vocabulary.  gtos_beam_topk(ll, k) stays the only pass over ll.
//
// The device compares output ids; the host search (gtos_amd.search.GroupBeam) compares token strings.  They agree because id and
// string map one to one within a graph, which repeat-n-gram blocking (csrc/ngram_kernels.h) relies on as well.
#pragma once
#include "beam_kernels.h"

namespace gtos_diverse {

using namespace gtos_beam;

constexpr int MAX_POOL = MAX_K * MAX_K;     // G = 1: g*k = k*k entries

// the diversity penalty weight an entry point accepts: finite and >= 0 (false for NaN)
GTOS_BEAM_HD bool lambda_ok(double lambda) { return lambda >= 0.0 && lambda < __builtin_inf(); }

// entries of chosen[0, n) equal to id
GTOS_BEAM_HD int count_of(const int* chosen, int n, int id) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += chosen[i] == id;
    return c;
}

// Python's `m - diversity * chosen.count(token)`
GTOS_BEAM_HD double key_of(double m, double lambda, int count) { return m - lambda * (double)count; }

// pool entry p of group q = b*G + j (width g) of graph b: model score, selection key, token id and string class
GTOS_BEAM_HD void pool_entry(int b, int q, int g, int k, int p, const float* topv, const int* topi, const double* slot_score,
                             const uint8_t* flag_shared, const uint8_t* flag_local, int V, int tot, double lambda, const int* chosen,
                             int n_chosen, double* model, double* key, int* tok, uint8_t* flag) {
    const int slot = q * g + p / k;
    const int64_t c = (int64_t)slot * k + p % k;
    const int id = topi[c];
    const uint8_t f = token_flag(flag_shared, flag_local, V, tot, b, id);
    const double m = cand_score(slot_score[slot], topv[c], f);
    *model = m;
    *key = key_of(m, lambda, count_of(chosen, n_chosen, id));
    *tok = id;
    *flag = f;
}

// place_cut's hook of this rule: the output id of every survivor is appended to chosen (n: its length); completions are not
struct ChosenHook {
    const int* pool_tok;
    int* chosen;
    int* n;
    GTOS_BEAM_HD void live(int p, int, int) const { chosen[(*n)++] = pool_tok[p]; }
    GTOS_BEAM_HD void done(int, int, int) const {}
};

// gtos_beam::place_cut for group q of width g (done at g completions) whose pool holds k candidates per slot: order[r] = pool position
// of the r-th best KEY, m entries.  Writes the group's slots of the back-pointer rows, the survivors' MODEL scores, completions at rows
// q*g + #completed, the group's state words, and appends the survivors' ids to chosen.  Returns true when the group stays not-done with
// live slots.
GTOS_BEAM_HD bool place(int q, int g, int k, int min_time_step, int max_time_step, const int* order, int m, const double* pool_model,
                        const int* pool_tok, const uint8_t* pool_flag, int t, int* state, int* bp_parent_t, int* bp_token_t,
                        double* slot_score, int* comp_step, int* comp_parent, double* comp_score, int* chosen, int* n_chosen) {
    return place_cut(q * g, g, k, min_time_step, max_time_step, order, m, pool_model, pool_tok, pool_flag, t,
                     state + (int64_t)q * BS_WORDS, bp_parent_t, bp_token_t, slot_score, comp_step, comp_parent, comp_score,
                     ChosenHook{pool_tok, chosen, n_chosen});
}

// The whole advance of one graph by one thread (the host check; the kernel parallelises each group's pool and ranks).  pool_* are
// scratch arrays of MAX_POOL entries, order and chosen of MAX_K.  Returns true when some group stays not-done with live slots.
GTOS_BEAM_HD bool advance_serial(int b, int k, int G, double lambda, int t, int V, int tot, int min_time_step, int max_time_step,
                                 const float* topv, const int* topi, const uint8_t* flag_shared, const uint8_t* flag_local,
                                 double* slot_score, int* state, int* bp_parent_t, int* bp_token_t, int* comp_step, int* comp_parent,
                                 double* comp_score, double* pool_model, double* pool_key, int* pool_tok, uint8_t* pool_flag,
                                 int* order, int* chosen) {
    const int g = k / G;
    int n_chosen = 0;
    bool go = false;
    for (int j = 0; j < G; ++j) {
        const int q = b * G + j;
        const int* st = state + (int64_t)q * BS_WORDS;
        if (st[BS_DONE]) continue;
        const int P = st[BS_NLIVE] * k;
        for (int p = 0; p < P; ++p)
            pool_entry(b, q, g, k, p, topv, topi, slot_score, flag_shared, flag_local, V, tot, lambda, chosen, n_chosen, pool_model + p,
                       pool_key + p, pool_tok + p, pool_flag + p);
        const int m = cut_size(P, g, st[BS_NCOMP]);
        for (int p = 0; p < P; ++p) {
            const int r = rank_of(pool_key, P, p);
            if (r < m) order[r] = p;
        }
        go |= place(q, g, k, min_time_step, max_time_step, order, m, pool_model, pool_tok, pool_flag, t, state, bp_parent_t, bp_token_t,
                    slot_score, comp_step, comp_parent, comp_score, chosen, &n_chosen);
    }
    return go;
}

}  // namespace gtos_diverse
