// Selection rule of the lexically constrained beam search (csrc/constrain.hip; Post & Vilar, "Fast Lexically Constrained Decoding with
// Dynamic Beam Allocation", single-token constraints), written so that the SAME code compiles for the host:
// tests/test_constrained_beam.py builds it with g++ and compares a serial advance (advance_serial) with
// gtos_amd.search.ConstrainedBeam.advance on random pools.  It is the rule of csrc/beam_kernels.h with three additions; cand_score,
// before, cut_size, place_cut and the state words are that header's, and a graph without constraints gets exactly that header's tables.
//
// Constraints: cons int32 [B, Cw], row b the output ids graph b must produce, c_b of them (at most MAX_CONS), then -1.  An id outside
// [0, tot) ends the row like -1 does.  The ids of a row are distinct and of the plain string class (the caller's contract;
// gtos_amd.generator.check_constraints).  full_b = (1 << c_b) - 1.
//
// 1. State.  Every slot carries the bit mask `met` of its graph's constraints it has produced: met int32 [2, N], all zero at the start;
//    step t reads row t % 2 and writes row (t + 1) % 2.
// 2. Pool.  Beam b with n_live live slots has W = k + Cw entries per slot, position p = j*W + r for live slot j.
//    r < k: top-k candidate r of the slot, as in beam_kernels.h -- but ABSENT if its class is <END> and met[slot] != full_b: a hypothesis
//      ends only when it holds every constraint.
//    r >= k: the forced candidate of constraint i = r - k, PRESENT only if i < c_b, bit i of met[slot] is clear, cons[b][i] is not among
//      the slot's k top-k ids (it is in the pool already) and ll[slot, cons[b][i]] > -inf (ll as the selection sees it: after
//      repeat-n-gram blocking, so a banned constraint is not forced).  Its score is cand_score(slot score, ll[slot, id], class).
//    A present entry has mask' = met[slot] | (bit i for the i with id == cons[b][i]) and bank = popcount(mask').
// 3. Order.  Absent entries are never placed.  Within a bank, q is the entry's rank under before(score, p) (stable, descending).  The
//    final order is ascending q, then descending bank: the best of every bank from the fullest bank down, then the second best of
//    every bank, and so on.  The cut is m = min(#present, k - #completed); placement is gtos_beam::place_cut's with parent slot
//    b*k + p / W, and mask' of every survivor goes to the new met row at the survivor's new slot (0 at the beam's other slots).
//    Scores written are model scores.
//
// Why top-k plus forced candidates is the pool (it is Post & Vilar's candidate set, per slot instead of per beam): an entry outside a
// slot's top-k that advances no constraint has at least k - j better entries of the same slot in its own bank, j being the slot's
// top-k entries that advance a constraint and so sit in a fuller bank ahead of it.  With j = 0 it is never among the first k of the
// order, so the rule equals the same ordering over the full vocabulary; with j > 0 it could in rare cases reach the cut, and the pool
// as stated here is the definition.  The entries outside the top-k that matter are those that raise the bank: the forced ones.
// gtos_beam_topk(ll, k) stays the only pass over ll; a forced candidate reads one element of it.
//
// The device compares output ids; the host search (gtos_amd.search.ConstrainedBeam) compares token strings.  They agree because id and
// string map one to one within a graph, which repeat-n-gram blocking (csrc/ngram_kernels.h) relies on as well.
#pragma once
#include "beam_kernels.h"

namespace gtos_constrain {

using namespace gtos_beam;

constexpr int MAX_CONS = 16;
constexpr int MAX_POOL = MAX_K * (MAX_K + MAX_CONS);

// c_b: the leading ids of graph b's row that lie in [0, tot)
GTOS_BEAM_HD int n_cons(const int* cons_b, int Cw, int tot) {
    int c = 0;
    while (c < Cw && cons_b[c] >= 0 && cons_b[c] < tot) ++c;
    return c;
}

GTOS_BEAM_HD int bank_of(int mask) { return __builtin_popcount((unsigned)mask); }

// met | (bit i for every i < c with cons_b[i] == id)
GTOS_BEAM_HD int mask_with(int met, const int* cons_b, int c, int id) {
    for (int i = 0; i < c; ++i)
        if (cons_b[i] == id) met |= 1 << i;
    return met;
}

// Pool entry p of beam b (W = k + Cw entries per slot): returns whether it is present; if so its score, token id, string class and
// mask'.  topv / topi: [N, k] candidates of every slot; ll [N, tot] with row stride ld; met_t: the met row step t reads.  cons may be
// null when Cw == 0.
GTOS_BEAM_HD bool pool_entry(int b, int k, int Cw, int p, const float* topv, const int* topi, const float* ll, int64_t ld,
                             const int* cons, const double* slot_score, const int* met_t, const uint8_t* flag_shared,
                             const uint8_t* flag_local, int V, int tot, double* score, int* tok, uint8_t* flag, int* mask) {
    const int W = k + Cw, slot = b * k + p / W, r = p % W;
    const int* cons_b = Cw ? cons + (int64_t)b * Cw : nullptr;
    const int c = n_cons(cons_b, Cw, tot), met = met_t[slot];
    const int* ids = topi + (int64_t)slot * k;
    int id;
    float x;
    if (r < k) {
        id = ids[r];
        x = topv[(int64_t)slot * k + r];
    } else {
        const int i = r - k;
        if (i >= c || (met >> i & 1)) return false;
        id = cons_b[i];
        for (int j = 0; j < k; ++j)
            if (ids[j] == id) return false;
        x = ll[(int64_t)slot * ld + id];
        if (!(x > -__builtin_inff())) return false;
    }
    const uint8_t f = token_flag(flag_shared, flag_local, V, tot, b, id);
    if (r < k && f == TOK_END && met != (1 << c) - 1) return false;
    *score = cand_score(slot_score[slot], x, f);
    *tok = id;
    *flag = f;
    *mask = mask_with(met, cons_b, c, id);
    return true;
}

// q of present entry e: its rank among the present entries of its bank (bank[] < 0: absent)
GTOS_BEAM_HD int rank_in_bank(const double* score, const signed char* bank, int P, int e) {
    const double s = score[e];
    const int bk = bank[e];
    int q = 0;
    for (int j = 0; j < P; ++j) q += bank[j] == bk && before(score[j], j, s, e);
    return q;
}

// position of present entry e in the final order: ascending q, then descending bank ((q, bank) is unique among present entries)
GTOS_BEAM_HD int final_position(const int* q, const signed char* bank, int P, int e) {
    const int qe = q[e], bk = bank[e];
    int r = 0;
    for (int j = 0; j < P; ++j) r += bank[j] >= 0 && (q[j] < qe || (q[j] == qe && bank[j] > bk));
    return r;
}

// place_cut's hook of this rule: mask' of every survivor goes to the new met row at its new slot
struct MetHook {
    const int* pool_mask;
    int* met_next;
    GTOS_BEAM_HD void live(int p, int, int dst) const { met_next[dst] = pool_mask[p]; }
    GTOS_BEAM_HD void done(int, int, int) const {}
};

// gtos_beam::place_cut for a pool of W entries per slot that also writes the beam's slots of the new met row (0 where no survivor
// lands): order[r] = pool position of the r-th entry of the final order, m entries.  Returns true when the beam stays not-done with
// live slots.
GTOS_BEAM_HD bool place(int b, int k, int W, int min_time_step, int max_time_step, const int* order, int m, const double* pool_score,
                        const int* pool_tok, const uint8_t* pool_flag, const int* pool_mask, int t, int* state, int* bp_parent_t,
                        int* bp_token_t, double* slot_score, int* comp_step, int* comp_parent, double* comp_score, int* met_next) {
    for (int j = 0; j < k; ++j) met_next[b * k + j] = 0;
    return place_cut(b * k, k, W, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, t,
                     state + (int64_t)b * BS_WORDS, bp_parent_t, bp_token_t, slot_score, comp_step, comp_parent, comp_score,
                     MetHook{pool_mask, met_next});
}

// The whole advance of one beam by one thread (the host check; the kernel parallelises the pool and the two rankings).  pool_* are
// scratch arrays of MAX_POOL entries, order of MAX_K.  Does nothing to a done beam.  Returns place()'s flag (false for a done beam).
GTOS_BEAM_HD bool advance_serial(int b, int k, int Cw, int t, int V, int tot, int min_time_step, int max_time_step, const float* topv,
                                 const int* topi, const float* ll, int64_t ld, const int* cons, const uint8_t* flag_shared,
                                 const uint8_t* flag_local, double* slot_score, int* state, int* bp_parent_t, int* bp_token_t,
                                 int* comp_step, int* comp_parent, double* comp_score, const int* met_t, int* met_next,
                                 double* pool_score, int* pool_tok, uint8_t* pool_flag, int* pool_mask, signed char* pool_bank,
                                 int* pool_q, int* order) {
    const int* st = state + (int64_t)b * BS_WORDS;
    if (st[BS_DONE]) return false;
    const int W = k + Cw, P = st[BS_NLIVE] * W;
    int present = 0;
    for (int p = 0; p < P; ++p) {
        const bool here = pool_entry(b, k, Cw, p, topv, topi, ll, ld, cons, slot_score, met_t, flag_shared, flag_local, V, tot,
                                     pool_score + p, pool_tok + p, pool_flag + p, pool_mask + p);
        pool_bank[p] = here ? (signed char)bank_of(pool_mask[p]) : (signed char)-1;
        present += here;
    }
    const int m = cut_size(present, k, st[BS_NCOMP]);
    for (int p = 0; p < P; ++p)
        if (pool_bank[p] >= 0) pool_q[p] = rank_in_bank(pool_score, pool_bank, P, p);
    for (int p = 0; p < P; ++p) {
        if (pool_bank[p] < 0) continue;
        const int r = final_position(pool_q, pool_bank, P, p);
        if (r < m) order[r] = p;
    }
    return place(b, k, W, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, pool_mask, t, state, bp_parent_t,
                 bp_token_t, slot_score, comp_step, comp_parent, comp_score, met_next);
}

}  // namespace gtos_constrain
