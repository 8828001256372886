// Selection rule of stochastic beam search (csrc/sbs.hip; Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them"),
// written so that the SAME code compiles for the host: tests/test_stochastic_beam.py builds it with g++ and compares a serial step and
// advance with a numpy statement of the rule, and draws from it to check the law.  The kernels run the same helpers.
//
// Slots as in csrc/slot_kernels.h, one beam per graph, state words as in csrc/beam_kernels.h.  The search draws k DISTINCT sequences
// per graph without replacement from the tempered, locally normalised model distribution q: the Gumbel-top-k trick run top-down over
// the prefix tree.  A live slot s = (graph b, position j) carries score[s] (fp64 sum of the model's ll of its tokens), logq[s] (fp64
// log q of its prefix) and G[s] (fp64, its perturbed value); at step 0 slot 0 of a graph is live with score = logq = 0 and
// G = root_gumbel(seed, b), which the caller writes: a Gumbel(0) draw of its own.  (A root fixed at 0 conditions the largest value of
// the tree on 0.  The order of the hypotheses does not depend on that value, so the draw would follow the same law, but the values
// would not be independent Gumbel(logq) variates any more and the importance weights of an estimator, which read the k-th value as
// a threshold, would be biased: measured on the toy tree of the tests, 16 % low.)
// Step t, for every live slot, all in fp64 (T enters as the fp32 value the C ABI passes):
//  1. allowed columns: rule 1 of csrc/sample_kernels.h (allowed()).  A row with none has no candidates: its hypothesis ends there.
//  2. local normalisation: m = max allowed ll, lse = log sum_allowed exp((ll_c - m) / T), logq_c = logq_s + (ll_c - m) / T - lse.
//     Without it the candidates' masses would not add up to their parent's and the conditioning of 5 would draw from a wrong law.
//  3. keys: key_c = logq_c + gumbel(row_key(seed, b, j, t), c), the counter hash of the sampling decode.
//  4. row cut: the k allowed columns with the largest key (larger key, then lower column; fewer if fewer are allowed); Z = the largest.
//  5. conditioning on the parent's value: G'_c = -log(exp(-G_s) - exp(-Z) + exp(-key_c)), computed as condition() does.  Every
//     child's value is <= its parent's, the child with key_c == Z gets exactly G_s, and the order within a row is the key order.
//  6. pool of graph b: its retained completions with their stored G, then the candidates of its live slots in (slot, rank) order;
//     ranked by larger G, then earlier position; the first k stay.  A kept <END> candidate becomes a completion, every other kept
//     candidate the next live slot in rank order; a completion that falls out of the first k is dropped.  The completion rows are
//     rewritten in descending G every step, so #completed + #live <= k always: finished hypotheses compete until the search ends.
//  7. state words (steps, #completed, #live, done) in the format of gtos_beam_advance, so gtos_beam_reorder serves unchanged:
//     done = no live slot left, or steps == max_time_step.  The active[3] rotation of csrc/slot_kernels.h: some not-done graph has a
//     live slot.
// Why no other rule's placement serves: there a completion is final and takes its row in append order, and the ranking value is a
// sum along the path; here completions are ranked again every step and the ranking value is conditioned on the parent's.
#pragma once
#include "beam_kernels.h"
#include "sample_kernels.h"

#define GTOS_SBS_HD GTOS_SLOT_HD

namespace gtos_sbs {

using namespace gtos_sample;            // allowed, weight, row_key, gumbel, wins; through it gtos_slot
using gtos_beam::BS_DONE;
using gtos_beam::BS_NCOMP;
using gtos_beam::BS_NLIVE;
using gtos_beam::BS_STEPS;
using gtos_beam::BS_WORDS;
constexpr int MAX_K = 32;
constexpr int MAX_POOL = MAX_K + MAX_K * MAX_K;        // a graph's completion rows, then k candidates of each of k slots

// the perturbed value of graph b's empty prefix: column 0 of the row of slot index MAX_K, which no slot has
GTOS_SBS_HD double root_gumbel(uint64_t seed, int b) { return gumbel(row_key(seed, b, MAX_K, 0), 0); }

// rule 2 for one column: m and lse are the row's
GTOS_SBS_HD double child_logq(double logq_s, float ll, float m, double T, double lse) {
    return logq_s + ((double)ll - (double)m) / T - lse;
}

// rule 5: v = G_s - key + log(1 - exp(key - Z)), G' = G_s - max(0, v) - log(1 + exp(-|v|)); key <= Z
GTOS_SBS_HD double condition(double G_s, double key, double Z) {
    if (key == Z) return G_s;
    const double v = G_s - key + log1p(-exp(key - Z));
    return G_s - (v > 0.0 ? v : 0.0) - log1p(exp(-fabs(v)));
}

// candidate r of a row, column c with key `key`: what gtos_sbs_step stores for it
GTOS_SBS_HD void emit(const float* x, int c, double key, double Z, double logq_s, double G_s, float m, double T, double lse, int* tok,
                      float* cll, double* clogq, double* cG) {
    *tok = c;
    *cll = x[c];
    *clogq = child_logq(logq_s, x[c], m, T, lse);
    *cG = condition(G_s, key, Z);
}

// Rules 1-5 of one row by one thread (the host check; the kernel spreads the passes over a workgroup).  kk: scratch of k keys.
// Writes the row's n <= k candidates in key order and -1 into the rest of tok; returns n.
GTOS_SBS_HD int row_serial(const float* x, int tot, int V, int b, int j, int t, int min_time_step, const uint8_t* flag_shared,
                           const uint8_t* flag_local, const uint8_t* owned_local, double T, uint64_t seed, int k, double logq_s,
                           double G_s, int* tok, float* cll, double* clogq, double* cG, double* kk) {
    for (int r = 0; r < k; ++r) tok[r] = -1;
    float m = -INFINITY;
    for (int c = 0; c < tot; ++c)
        if (allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, x[c])) m = x[c] > m ? x[c] : m;
    if (!(m > -INFINITY)) return 0;
    double z = 0.0;
    for (int c = 0; c < tot; ++c)
        if (allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, x[c])) z += weight(x[c], m, T);
    const double lse = log(z);
    const uint64_t rk = row_key(seed, b, j, t);
    int n = 0;
    for (int c = 0; c < tot; ++c) {
        if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, x[c])) continue;
        const double key = child_logq(logq_s, x[c], m, T, lse) + gumbel(rk, c);
        if (n == k && !wins(key, c, kk[n - 1], tok[n - 1])) continue;
        int i = n < k ? n++ : n - 1;
        for (; i > 0 && wins(key, c, kk[i - 1], tok[i - 1]); --i) { kk[i] = kk[i - 1]; tok[i] = tok[i - 1]; }
        kk[i] = key;
        tok[i] = c;
    }
    for (int r = 0; r < n; ++r) emit(x, tok[r], kk[r], kk[0], logq_s, G_s, m, T, lse, tok + r, cll + r, clogq + r, cG + r);
    return n;
}

// is slot j of a graph with state words st live at this step?
GTOS_SBS_HD bool slot_is_live(const int* st, int j) { return !st[BS_DONE] && j < st[BS_NLIVE]; }

// The tables of gtos_sbs_advance, in the order the entry point takes them
struct Tables {
    int B, k, t, V, tot, min_t, max_t;
    const int* cand_tok;                // [N, k], -1 = absent; the four as gtos_sbs_step wrote them
    const float* cand_ll;
    const double* cand_logq;
    const double* cand_gumbel;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    double* slot_score;                 // [N]
    double* slot_logq;
    double* slot_gumbel;
    int* state;                         // [B, BS_WORDS]
    int* bp_parent;                     // [max_t, N]
    int* bp_token;
    int* comp_step;                     // [B, k], descending G
    int* comp_parent;
    double* comp_score;
    double* comp_logq;
    double* comp_gumbel;
    int* active;
};

// What place() overwrites while it still reads it, copied first: the graph's completion rows (their G is the pool's) and slot scores
struct Stage {
    int* c_step;                        // [k] each
    int* c_parent;
    double* c_score;
    double* c_logq;
    double* s_score;
};

// Pool position p of graph b: p < k completion row p (present below #completed), else candidate (p - k) % k of slot (p - k) / k.
// present / G of the entry
GTOS_SBS_HD void pool_entry(const Tables& a, int b, int p, int ncomp, double* G, uint8_t* present) {
    if (p < a.k) {
        *present = p < ncomp;
        *G = p < ncomp ? a.comp_gumbel[(int64_t)b * a.k + p] : -INFINITY;
    } else {
        const int64_t ci = ((int64_t)b * a.k + (p - a.k) / a.k) * a.k + (p - a.k) % a.k;
        *present = a.cand_tok[ci] >= 0;
        *G = *present ? a.cand_gumbel[ci] : -INFINITY;
    }
}

GTOS_SBS_HD void stage_row(const Tables& a, int b, int i, const Stage& s) {
    const int64_t at = (int64_t)b * a.k + i;
    s.c_step[i] = a.comp_step[at];
    s.c_parent[i] = a.comp_parent[at];
    s.c_score[i] = a.comp_score[at];
    s.c_logq[i] = a.comp_logq[at];
    s.s_score[i] = a.slot_score[at];
}

// rank of present entry i among the present entries: larger G first, equal G earlier position first
GTOS_SBS_HD int rank_of(const double* G, const uint8_t* present, int P, int i) {
    const double g = G[i];
    int r = 0;
    for (int q = 0; q < P; ++q) r += present[q] && (G[q] > g || (G[q] == g && q < i));
    return r;
}

// Rules 6 and 7 for graph b given the cut: order[r] = pool position of rank r, -1 from the number of present entries on (k entries).
// Returns true when the graph goes on.
GTOS_SBS_HD bool place(const Tables& a, int b, const int* order, const double* G, const Stage& s) {
    const int k = a.k, base = b * k;
    const int64_t N = (int64_t)a.B * k;
    int* st = a.state + (int64_t)b * BS_WORDS;
    int* bp_parent_t = a.bp_parent + a.t * N;
    int* bp_token_t = a.bp_token + a.t * N;
    const int steps = st[BS_STEPS];
    int ncomp = 0, nlive = 0;
    for (int j = 0; j < k; ++j) {
        bp_parent_t[base + j] = -1;
        bp_token_t[base + j] = -1;
    }
    for (int r = 0; r < k && order[r] >= 0; ++r) {
        const int p = order[r];
        if (p < k) {                                      // a completion that stays (row p >= ncomp: rows only move up)
            a.comp_step[base + ncomp] = s.c_step[p];
            a.comp_parent[base + ncomp] = s.c_parent[p];
            a.comp_score[base + ncomp] = s.c_score[p];
            a.comp_logq[base + ncomp] = s.c_logq[p];
            a.comp_gumbel[base + ncomp] = G[p];
            ++ncomp;
            continue;
        }
        const int j = (p - k) / k;
        const int64_t ci = (int64_t)(base + j) * k + (p - k) % k;
        const int id = a.cand_tok[ci];
        const double score = s.s_score[j] + (double)a.cand_ll[ci];
        if (token_flag(a.flag_shared, a.flag_local, a.V, a.tot, b, id) == TOK_END) {
            a.comp_step[base + ncomp] = a.t;
            a.comp_parent[base + ncomp] = base + j;
            a.comp_score[base + ncomp] = score;
            a.comp_logq[base + ncomp] = a.cand_logq[ci];
            a.comp_gumbel[base + ncomp] = G[p];
            ++ncomp;
        } else {
            bp_parent_t[base + nlive] = base + j;
            bp_token_t[base + nlive] = id;
            a.slot_score[base + nlive] = score;
            a.slot_logq[base + nlive] = a.cand_logq[ci];
            a.slot_gumbel[base + nlive] = G[p];
            ++nlive;
        }
    }
    st[BS_STEPS] = steps + 1;
    st[BS_NCOMP] = ncomp;
    st[BS_NLIVE] = nlive;
    st[BS_DONE] = nlive == 0 || steps + 1 >= a.max_t;
    return !st[BS_DONE];
}

// The whole advance of one graph by one thread (the host check; the kernel parallelises the pool and the ranks).  G / present:
// scratch of MAX_POOL entries, order of k, s of k per array.  Does nothing to a done graph.  Returns place()'s flag.
GTOS_SBS_HD bool advance_serial(const Tables& a, int b, double* G, uint8_t* present, int* order, const Stage& s) {
    const int* st = a.state + (int64_t)b * BS_WORDS;
    if (st[BS_DONE]) return false;
    const int ncomp = st[BS_NCOMP], P = a.k + st[BS_NLIVE] * a.k;
    for (int p = 0; p < P; ++p) pool_entry(a, b, p, ncomp, G + p, present + p);
    for (int i = 0; i < a.k; ++i) {
        stage_row(a, b, i, s);
        order[i] = -1;
    }
    for (int p = 0; p < P; ++p) {
        if (!present[p]) continue;
        const int r = rank_of(G, present, P, p);
        if (r < a.k) order[r] = p;
    }
    return place(a, b, order, G, s);
}

}  // namespace gtos_sbs
