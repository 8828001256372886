// The rule of teacher-forced scoring (csrc/copy_eval.hip), written so that the SAME code compiles for the host: tests/test_score_eval.py
// builds it with g++ and compares row_serial with a float64 numpy statement.
//
// Row r = (t, b) with target y, logits x [V], diverter (d0, d1), alignment a [S] and copy ids k_s = cp_seq[s, b]:
//   s = softmax(x), g = 1 / (1 + exp(d1 - d0)), c = 1 - g            (the gates exactly as gtos_copy_nll_fwd forms them)
//   p_k = g s_k [k < V] + c sum_{s: k_s == k} a_s,                    k >= 0 (a column no copy id names and that is >= V has p = 0)
//   nll  = 0 at y == pad, else -log(p_y + 1e-12)                     (p_y = 0 for a y that is neither < V nor a copy id of graph b)
//   pred = argmax_k p_k, equal values to the LOWER column (the tie rule of gtos_beam_topk); p_pred = p_pred's value.
// A padded row (y == pad) writes nll = 0 and still its pred / p_pred.
//
// Which columns compete.  Copy mass is non-negative and g s_k is monotone in x_k, so the argmax is the better of
//   (i)  the largest logit of the row, lowest column among equal logits, through g sig_top, sig_top = exp(top - lse), and
//   (ii) the best copy group: for every source position s that LEADS its id (k_s >= 0 and no j < s with k_j == k_s),
//        p = (k_s < V ? g column_sig(x_{k_s}) : 0) + c (a_s + the a_j of the later positions with the same id, in ascending j).
// (i) and (ii) are compared by better(): larger p, then lower column.  A group on the vocabulary winner's own column has p >= (i) and
// the same column, so the two never disagree about a column.  Negative copy ids are ignored (as gtos_copy_ll_fwd ignores them).
//
// Groups are found per row, in LDS: the kernel stages column b of cp_seq and the row's alignment (12 bytes per source position) and
// every thread scans for the leaders among its positions -- O(S^2 / 256) LDS reads per thread, S being a graph's node count (<= ~300;
// MAX_S bounds the LDS).  The group workspace of label smoothing (gtos_copy_nll_ls_prep) is NOT used: scoring stays one launch.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GTOS_EV_HD __host__ __device__ inline
#else
#define GTOS_EV_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GTOS_EV_EXP __expf
#define GTOS_EV_LOG __logf
#else
#define GTOS_EV_EXP expf
#define GTOS_EV_LOG logf
#endif

namespace gtos_eval {

constexpr float TINY = 1e-12f;
constexpr int MAX_S = 4096;           // source positions per graph: 12 bytes of LDS each
constexpr int NO_COL = 0x7fffffff;

GTOS_EV_HD void gates(float d0, float d1, float& g, float& c) {
    g = 1.f / (1.f + GTOS_EV_EXP(d1 - d0));
    c = 1.f - g;
}
// exp(x - lse) of a column.  A column whose logit EQUALS the row's largest takes the very value the vocabulary candidate was formed
// from (sig_top = exp(top - lse), evaluated once per row), so an exact tie of two logits is an exact tie of their p whatever form the
// compiler gives each expression (fast-math may fuse and reassociate them differently at different sites).
GTOS_EV_HD float column_sig(float x, float top, float sig_top, float lse) { return x == top ? sig_top : GTOS_EV_EXP(x - lse); }
GTOS_EV_HD float row_nll(float p, bool is_pad) { return is_pad ? 0.f : -GTOS_EV_LOG(p + TINY); }
// (p, col) beats (q, col2): the larger probability, equal ones to the lower column
GTOS_EV_HD bool better(float p, int col, float q, int col2) { return p > q || (p == q && col < col2); }

// ids: the copy ids of one graph, position s at ids[s * stride] (cp_seq column b: stride B; the LDS copy: stride 1)
GTOS_EV_HD bool leads(const int64_t* ids, int64_t stride, int s) {
    const int64_t id = ids[s * stride];
    if (id < 0) return false;
    for (int j = 0; j < s; ++j)
        if (ids[j * stride] == id) return false;
    return true;
}
// alignment mass of the group that position s leads (members in ascending position)
GTOS_EV_HD float group_mass(const int64_t* ids, int64_t stride, int S, int s, const float* a) {
    const int64_t id = ids[s * stride];
    float m = a[s];
    for (int j = s + 1; j < S; ++j)
        if (ids[j * stride] == id) m += a[j];
    return m;
}
// candidate (ii) of a leading position: its column's whole probability.  sig = exp(x_id - lse) for id < V, else 0
GTOS_EV_HD float group_p(float g, float c, float sig, float mass) { return g * sig + c * mass; }

// ---- host statement, one row (what the kernel computes, serially).  x: fp32 logits; cp: cp_seq [S, B]
inline void row_serial(const float* x, int V, float d0, float d1, const float* a, int S, const int64_t* cp, int B, int b, int64_t y,
                       int64_t pad, float* nll, int* pred, float* p_pred) {
    float mx = -INFINITY, se = 0.f;
    int amax = 0;
    for (int k = 0; k < V; ++k)
        if (x[k] > mx) { mx = x[k]; amax = k; }
    for (int k = 0; k < V; ++k) se += expf(x[k] - mx);
    const float lse = mx + logf(se);
    float g, c;
    gates(d0, d1, g, c);
    float mass = 0.f;
    for (int s = 0; s < S; ++s)
        if (cp[(int64_t)s * B + b] == y) mass += a[s];
    const float sig = (y >= 0 && y < V) ? expf(x[y] - lse) : 0.f;
    *nll = row_nll(g * sig + c * mass, y == pad);
    const float sig_top = expf(mx - lse);
    float best = g * sig_top;
    int col = amax;
    for (int s = 0; s < S; ++s) {
        if (!leads(cp + b, B, s)) continue;
        const int64_t id = cp[(int64_t)s * B + b];
        const float p = group_p(g, c, id < V ? column_sig(x[id], mx, sig_top, lse) : 0.f, group_mass(cp + b, B, S, s, a));
        if (better(p, (int)id, best, col)) { best = p; col = (int)id; }
    }
    *pred = col;
    *p_pred = best;
}

}  // namespace gtos_eval
