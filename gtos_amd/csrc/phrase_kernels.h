// Selection rule of the phrase-constrained beam search (csrc/phrase.hip): the rule of csrc/constrain_kernels.h with multi-token
// constraints, written so that the SAME code compiles for the host: tests/test_phrase_beam.py builds it with g++ and compares a serial
// advance (advance_serial) with gtos_amd.search.PhraseBeam.advance on random pools.  cand_score, before, cut_size, place_cut and the
// state words are csrc/beam_kernels.h's; the two rankings, the hook and place() are csrc/constrain_kernels.h's.  With single-token
// phrases of distinct ids every table equals that header's; a graph without phrases gets exactly the tables of beam_kernels.h.
//
// Phrases: phr int32 [B, Cw, Lw], row (b, i) the output ids of phrase i of graph b, len_i of them (at most Lw <= MAX_LEN), then -1.  An
// id outside [0, tot) ends a phrase like -1 does; an empty phrase ends the graph's list, and so does a phrase with which the graph would
// hold more than MAX_TOKENS tokens: c_b phrases (at most MAX_PHR), full_b = (1 << c_b) - 1.  The ids are of the plain string class (the
// caller's contract; gtos_amd.generator.check_phrases).  A phrase may be listed twice and must then occur twice.
//
// 1. State.  Every slot carries `met` (the bit mask of its graph's phrases it has finished), `open` (the phrase in progress, or -1) and
//    `pos` (the tokens of the open phrase matched so far, 1 .. len - 1; 0 when nothing is open), packed into one int32 -- bits 0-15 met,
//    bits 16-20 open + 1, bits 21-25 pos -- of pst int32 [2, N], all zero at the start; step t reads row t % 2 and writes row
//    (t + 1) % 2.  With single-token phrases the word is the mask.
// 2. Transition on token x (next_state).  If a phrase is open and its token at pos is x, pos advances; when that completes the phrase
//    its bit is set and nothing is open.  Otherwise the open phrase's progress is dropped, and the lowest-index phrase whose bit is clear
//    and whose first token is x starts: met at once if its length is 1, else open with pos = 1; if none starts on x, nothing is open.
//    There are no failure links: "a a b" inside "a a a b" restarts at pos = 1 on the third a and the phrase is not found.  That is the
//    definition, on the device and in gtos_amd.search.phrase_state alike.
// 3. Bank.  The number of constraint tokens a state holds: the summed lengths of its met phrases plus pos.  A mismatch lowers it.
// 4. Pool.  Beam b with n_live live slots has W = k + Cw entries per slot, position p = j*W + r for live slot j.
//    r < k: top-k candidate r of the slot, as in beam_kernels.h -- but ABSENT if its class is <END> and met[slot] != full_b.
//    r >= k: the forced candidate of phrase i = r - k, PRESENT only if i < c_b, bit i of met is clear and
//      - a phrase is open: i == open, the id being that phrase's token at pos;
//      - nothing is open: the id is the phrase's first token and no lower-index phrase with its bit clear starts with the same id
//        (one pool entry per (slot, id));
//      and the id is not among the slot's k top-k ids and ll[slot, id] > -inf (ll as the selection sees it: after repeat-n-gram
//      blocking, so a banned token is not forced).  Its score is cand_score(slot score, ll[slot, id], class).
//    Every present entry's next state is the transition on its id, its bank that state's.
// 5. Order and placement: constrain_kernels.h's, unchanged -- within a bank the rank q under before(score, p), the final order
//    ascending q then descending bank, the cut m = min(#present, k - #completed), gtos_constrain::place with the packed next state as
//    the word a survivor carries to the new pst row (0 at the beam's other slots).  Scores written are model scores.
//
// What the rule guarantees: the best entry of the fullest bank always survives, and a slot of bank n < T_b (T_b: the tokens of the
// graph's phrases) offers, forced or in its top-k, a candidate of bank n + 1 whenever that id's ll is finite.  So the fullest bank rises
// by one per step and, with min_time_step <= T_b <= max_time_step, some hypothesis holds every phrase after T_b steps.
#pragma once
#include "constrain_kernels.h"

namespace gtos_phrase {

using namespace gtos_constrain;         // MAX_POOL (k + MAX_PHR entries per slot), rank_in_bank, final_position, place

constexpr int MAX_PHR = 16;
constexpr int MAX_LEN = 16;
constexpr int MAX_TOKENS = 64;
static_assert(MAX_PHR == MAX_CONS, "the pool bound and the mask bits are constrain_kernels.h's");

// One graph's phrases as the rule reads them: the row of phr, c and the lengths
struct PhraseSet {
    const int* tok;                     // [Cw, Lw]
    int Lw, c, total;                   // total: the tokens of the c phrases, T_b
    unsigned char len[MAX_PHR];
    GTOS_BEAM_HD int at(int i, int j) const { return tok[i * Lw + j]; }
};

// phr_b may be null when Cw == 0
GTOS_BEAM_HD void load_phrases(PhraseSet* s, const int* phr_b, int Cw, int Lw, int tot) {
    s->tok = phr_b;
    s->Lw = Lw;
    s->c = 0;
    s->total = 0;
    for (int i = 0; i < Cw && i < MAX_PHR; ++i) {
        int n = 0;
        while (n < Lw && phr_b[i * Lw + n] >= 0 && phr_b[i * Lw + n] < tot) ++n;
        if (n == 0 || s->total + n > MAX_TOKENS) break;
        s->len[i] = (unsigned char)n;
        s->total += n;
        s->c = i + 1;
    }
}

GTOS_BEAM_HD int pack_state(int met, int open, int pos) { return met | (open + 1) << 16 | pos << 21; }
GTOS_BEAM_HD int state_met(int w) { return w & 0xFFFF; }
GTOS_BEAM_HD int state_open(int w) { return (w >> 16 & 31) - 1; }
GTOS_BEAM_HD int state_pos(int w) { return w >> 21 & 31; }

// the transition (2.) of packed state w on token id x
GTOS_BEAM_HD int next_state(const PhraseSet& s, int w, int x) {
    int met = state_met(w);
    const int open = state_open(w), pos = state_pos(w);
    if (open >= 0 && open < s.c && pos < s.len[open] && s.at(open, pos) == x)
        return pos + 1 == s.len[open] ? pack_state(met | 1 << open, -1, 0) : pack_state(met, open, pos + 1);
    for (int i = 0; i < s.c; ++i)
        if (!(met >> i & 1) && s.at(i, 0) == x) return s.len[i] == 1 ? pack_state(met | 1 << i, -1, 0) : pack_state(met, i, 1);
    return pack_state(met, -1, 0);
}

// the bank (3.) of packed state w
GTOS_BEAM_HD int bank_of_state(const PhraseSet& s, int w) {
    const int met = state_met(w);
    int n = state_pos(w);
    for (int i = 0; i < s.c; ++i)
        if (met >> i & 1) n += s.len[i];
    return n;
}

// the id phrase i offers a slot in state w as its forced candidate (4.), or -1 when it offers none
GTOS_BEAM_HD int forced_id(const PhraseSet& s, int w, int i) {
    const int met = state_met(w), open = state_open(w);
    if (i >= s.c || (met >> i & 1)) return -1;
    if (open >= 0) return i == open && state_pos(w) < s.len[i] ? s.at(i, state_pos(w)) : -1;
    const int id = s.at(i, 0);
    for (int j = 0; j < i; ++j)
        if (!(met >> j & 1) && s.at(j, 0) == id) return -1;
    return id;
}

// Pool entry p of beam b (W = k + Cw entries per slot): returns whether it is present; if so its score, token id, string class and
// packed next state.  topv / topi: [N, k] candidates of every slot; ll [N, tot] with row stride ld; pst_t: the state row step t reads;
// s: the phrases of graph b.
GTOS_BEAM_HD bool pool_entry(int b, int k, int Cw, int p, const float* topv, const int* topi, const float* ll, int64_t ld,
                             const PhraseSet& s, const double* slot_score, const int* pst_t, const uint8_t* flag_shared,
                             const uint8_t* flag_local, int V, int tot, double* score, int* tok, uint8_t* flag, int* next) {
    const int W = k + Cw, slot = b * k + p / W, r = p % W;
    const int w = pst_t[slot];
    const int* ids = topi + (int64_t)slot * k;
    int id;
    float x;
    if (r < k) {
        id = ids[r];
        x = topv[(int64_t)slot * k + r];
    } else {
        id = forced_id(s, w, r - k);
        if (id < 0) return false;
        for (int j = 0; j < k; ++j)
            if (ids[j] == id) return false;
        x = ll[(int64_t)slot * ld + id];
        if (!(x > -__builtin_inff())) return false;
    }
    const uint8_t f = token_flag(flag_shared, flag_local, V, tot, b, id);
    if (r < k && f == TOK_END && state_met(w) != (1 << s.c) - 1) return false;
    *score = cand_score(slot_score[slot], x, f);
    *tok = id;
    *flag = f;
    *next = next_state(s, w, id);
    return true;
}

// The whole advance of one beam by one thread (the host check; the kernel parallelises the pool and the two rankings).  pool_* are
// scratch arrays of MAX_POOL entries, order of MAX_K.  Does nothing to a done beam.  Returns place()'s flag (false for a done beam).
GTOS_BEAM_HD bool advance_serial(int b, int k, int Cw, int Lw, int t, int V, int tot, int min_time_step, int max_time_step,
                                 const float* topv, const int* topi, const float* ll, int64_t ld, const int* phr,
                                 const uint8_t* flag_shared, const uint8_t* flag_local, double* slot_score, int* state, int* bp_parent_t,
                                 int* bp_token_t, int* comp_step, int* comp_parent, double* comp_score, const int* pst_t, int* pst_next,
                                 double* pool_score, int* pool_tok, uint8_t* pool_flag, int* pool_next, signed char* pool_bank,
                                 int* pool_q, int* order) {
    const int* st = state + (int64_t)b * BS_WORDS;
    if (st[BS_DONE]) return false;
    PhraseSet s;
    load_phrases(&s, Cw ? phr + (int64_t)b * Cw * Lw : nullptr, Cw, Lw, tot);
    const int W = k + Cw, P = st[BS_NLIVE] * W;
    int present = 0;
    for (int p = 0; p < P; ++p) {
        const bool here = pool_entry(b, k, Cw, p, topv, topi, ll, ld, s, slot_score, pst_t, flag_shared, flag_local, V, tot,
                                     pool_score + p, pool_tok + p, pool_flag + p, pool_next + p);
        pool_bank[p] = here ? (signed char)bank_of_state(s, pool_next[p]) : (signed char)-1;
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
    return place(b, k, W, min_time_step, max_time_step, order, m, pool_score, pool_tok, pool_flag, pool_next, t, state, bp_parent_t,
                 bp_token_t, slot_score, comp_step, comp_parent, comp_score, pst_next);
}

}  // namespace gtos_phrase
