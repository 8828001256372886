// Selection rule of the device-resident beam search (csrc/beam.hip), written so that the SAME code compiles for the host:
// tests/test_device_beam_search.py builds it with g++ and compares a serial advance (beam_advance_serial) with
// gtos_amd.search.Beam.advance / Beam.completed on random pools, step counters included.  The kernel runs the same helpers:
// the pool is filled and ranked by many threads (pool_entry, rank_of), the cut is placed by one (place, which is place_cut -- the
// placement that the rules of the diverse, constrained and coverage searches run as well, each through a hook for its own stores).
//
// Slots as in csrc/slot_kernels.h, one beam per graph.  After an advance the live hypotheses of beam b are its
// slots b*k .. b*k + n_live - 1, in the order Beam.advance returns them.  The pool of an advance is the candidates of the live
// slots in (slot, candidate rank) order: position p = j*k + r for live slot j and rank r, k candidates per slot.
#pragma once
#include "slot_kernels.h"

#define GTOS_BEAM_HD GTOS_SLOT_HD

namespace gtos_beam {

using namespace gtos_slot;              // token classes, token_flag, the active[3] rotation
// per-beam state words, int32 [B, BS_WORDS]
enum { BS_STEPS = 0, BS_NCOMP = 1, BS_NLIVE = 2, BS_DONE = 3, BS_WORDS = 4 };
constexpr int MAX_K = 32;

// Python's `float('-inf') if token == UNK else base + ll`: base is the parent's fp64 score, ll an fp32 log-likelihood
GTOS_BEAM_HD double cand_score(double base, float ll, uint8_t flag) {
    return flag == TOK_UNK ? -__builtin_inf() : base + (double)ll;
}

// candidate a goes before candidate b: stable descending sort on the score (list.sort(key=score, reverse=True) keeps equal
// scores, -inf included, in pool order)
GTOS_BEAM_HD bool before(double sa, int pa, double sb, int pb) { return sa > sb || (sa == sb && pa < pb); }

// position of pool entry i in the sorted pool
GTOS_BEAM_HD int rank_of(const double* score, int P, int i) {
    const double s = score[i];
    int r = 0;
    for (int j = 0; j < P; ++j) r += before(score[j], j, s, i);
    return r;
}

// pool entry p of beam b: score, token id and string class.  topv / topi: [N, k] candidates of every slot
GTOS_BEAM_HD void pool_entry(int b, int k, int p, const float* topv, const int* topi, const double* slot_score,
                             const uint8_t* flag_shared, const uint8_t* flag_local, int V, int tot,
                             double* score, int* tok, uint8_t* flag) {
    const int slot = b * k + p / k;
    const int64_t c = (int64_t)slot * k + p % k;
    const int id = topi[c];
    const uint8_t f = token_flag(flag_shared, flag_local, V, tot, b, id);
    *score = cand_score(slot_score[slot], topv[c], f);
    *tok = id;
    *flag = f;
}

// The placement of a sorted cut, the one statement of it that all four selection rules run (this header's place and those of
// csrc/diverse_kernels.h, constrain_kernels.h and coverage_kernels.h): Beam.place in gtos_amd/search.py.  A beam or group owns the
// `width` slots and completion rows from `base` on and the state words st[BS_WORDS]; its pool holds per_slot entries per live slot, so
// entry p has the parent slot base + p / per_slot.  order[r] = pool position of the r-th entry of the cut, m entries.  Clears the
// beam's slots of the back-pointer rows bp_parent_t / bp_token_t ([N]: parent slot or -1, token id), then takes the cut in order: an
// <END> entry becomes the completion at row base + #completed of comp_* if the hypothesis is long enough (else it is dropped), any other
// entry the next live slot, with its score in slot_score.  What a rule stores beyond that goes through its hook: hook.live(p, parent,
// dst) after entry p became live slot dst, hook.done(p, parent, dst) after it became completion row dst.  Writes the state words;
// returns true when the beam stays not-done with live slots (the next iteration runs only if some beam does).
template <class Hook>
GTOS_BEAM_HD bool place_cut(int base, int width, int per_slot, int min_time_step, int max_time_step, const int* order, int m,
                            const double* pool_score, const int* pool_tok, const uint8_t* pool_flag, int t, int* st, int* bp_parent_t,
                            int* bp_token_t, double* slot_score, int* comp_step, int* comp_parent, double* comp_score, Hook hook) {
    const int steps = st[BS_STEPS];
    int ncomp = st[BS_NCOMP], nlive = 0;
    for (int j = 0; j < width; ++j) {
        bp_parent_t[base + j] = -1;
        bp_token_t[base + j] = -1;
    }
    for (int r = 0; r < m; ++r) {
        const int p = order[r];
        const int parent = base + p / per_slot;
        if (pool_flag[p] == TOK_END) {
            if (steps >= min_time_step) {                 // len(hyp) - 2 >= min_time_step, len(hyp) = steps + 2
                comp_step[base + ncomp] = t;
                comp_parent[base + ncomp] = parent;
                comp_score[base + ncomp] = pool_score[p];
                hook.done(p, parent, base + ncomp);
                ++ncomp;
            }
        } else {
            bp_parent_t[base + nlive] = parent;
            bp_token_t[base + nlive] = pool_tok[p];
            slot_score[base + nlive] = pool_score[p];
            hook.live(p, parent, base + nlive);
            ++nlive;
        }
    }
    st[BS_STEPS] = steps + 1;
    st[BS_NCOMP] = ncomp;
    st[BS_NLIVE] = nlive;
    st[BS_DONE] = ncomp >= width || steps + 1 >= max_time_step;
    return !st[BS_DONE] && nlive > 0;
}

// the hook of a rule that stores nothing of its own
struct NoHook {
    GTOS_BEAM_HD void live(int, int, int) const {}
    GTOS_BEAM_HD void done(int, int, int) const {}
};

// One beam's advance at step t (Beam.advance + Beam.completed), given the sorted cut of m = min(P, k - #completed) entries: place_cut
// for beam b of width k, k pool entries per slot, the survivors' scores into slot_score, completions into comp_* [B, k] in append order.
GTOS_BEAM_HD bool place(int b, int k, int min_time_step, int max_time_step, const int* order, int m, const double* pool_score,
                        const int* pool_tok, const uint8_t* pool_flag, int t, int* state, int* bp_parent_t, int* bp_token_t,
                        double* slot_score, int* comp_step, int* comp_parent, double* comp_score) {
    return place_cut(b * k, k, k, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, t,
                     state + (int64_t)b * BS_WORDS, bp_parent_t, bp_token_t, slot_score, comp_step, comp_parent, comp_score, NoHook());
}

// Number of pool entries the cut keeps: Python's pool[:beam_size - len(completed)]
GTOS_BEAM_HD int cut_size(int P, int k, int ncomp) {
    const int c = k - ncomp;
    return P < c ? P : c;
}

// The whole advance of one beam by one thread (the host check; the kernel parallelises the pool and the ranks).  pool_* are
// scratch arrays of k*k entries, order of k.  Does nothing to a done beam.  Returns place()'s flag (false for a done beam).
GTOS_BEAM_HD bool advance_serial(int b, int k, int t, int V, int tot, int min_time_step, int max_time_step, const float* topv,
                                 const int* topi, const uint8_t* flag_shared, const uint8_t* flag_local, double* slot_score,
                                 int* state, int* bp_parent_t, int* bp_token_t, int* comp_step, int* comp_parent,
                                 double* comp_score, double* pool_score, int* pool_tok, uint8_t* pool_flag, int* order) {
    const int* st = state + (int64_t)b * BS_WORDS;
    if (st[BS_DONE]) return false;
    const int P = st[BS_NLIVE] * k;
    for (int p = 0; p < P; ++p)
        pool_entry(b, k, p, topv, topi, slot_score, flag_shared, flag_local, V, tot, pool_score + p, pool_tok + p, pool_flag + p);
    const int m = cut_size(P, k, st[BS_NCOMP]);
    for (int p = 0; p < P; ++p) {
        const int r = rank_of(pool_score, P, p);
        if (r < m) order[r] = p;
    }
    return place(b, k, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, t, state, bp_parent_t, bp_token_t,
                 slot_score, comp_step, comp_parent, comp_score);
}

}  // namespace gtos_beam
