// The rule of token-level attribution (csrc/copy_explain.hip), written so that the SAME code compiles for the host: tests/test_explain.py
// builds it with g++ and compares row_serial with a float64 numpy statement.
//
// Row r = (t, b) with target y, logits x [V], diverter (d0, d1), alignment a [S] and copy ids k_s = cp_seq[s, b]; as in
// copy_eval_kernels.h:  s = softmax(x), (g, c) = gates,  q_k = g s_k [k < V],  p_k = q_k + c sum_{s: k_s == k} a_s.
// The UNIVERSE of a row is the vocabulary columns [0, V) plus the distinct non-negative copy ids of graph b; y is REACHABLE when it is
// in the universe.  Per row:
//   nll           gtos_copy_eval_fwd's value, bit for bit (0 at y == pad)
//   entropy       H = -sum_k p_k ln p_k over the universe, nats, 0 ln 0 = 0: of the mixture, not of the softmax
//   gate          c
//   copy_share    c mass_y / (q_y + c mass_y), 0 where the denominator is 0; exactly 1 for a reachable y >= V with positive mass
//   source        among the positions with k_s == y the one with the largest a_s, the lowest s among equals; -1 when none holds y
//   source_weight a_source (0 at source == -1)
//   focus         argmax_s a_s over all S positions, the lowest s among equals; focus_weight its weight (-1 and 0 at S == 0)
//   rank          #{k in the universe, k != y : p_k > p_y}, strict; -1 for an unreachable target
// A padded row (y == pad) writes nll = 0, copy_share = 0, source = -1, source_weight = 0, rank = -1 and still its entropy, gate, focus
// and focus_weight.  A negative y is never reachable (negative copy ids are ignored, as everywhere).
//
// No dense row.  With m = max x, e_k = exp(x_k - m), Z = sum e_k, E = sum e_k (x_k - m) and h(p) = -p ln p:
//   H = H_vocab + sum_{leading positions} [h(p_id) - h(q_id)],   H_vocab = -sum_{k<V} q_k ln q_k = h(g) + g (ln Z - E / Z)
// (ln s_k = (x_k - m) - ln Z; a leading position is one that leads() its id, its column's p is group_p of the id's whole mass; an id
// >= V has q = 0).  Both terms of H_vocab are sums of non-negative numbers.
//   rank = #{k < V, k != y : q_k > p_y} + sum_{leading positions, id != y} ([p_id > p_y] - [id < V and q_id > p_y])
// i.e. a count over the logits row, corrected at the columns that carry copy mass.  E, Z and the count come from ONE further pass over
// the logits after the two of the lse.
//
// One value per column.  Every site forms q of a column as gs * col_e(x, m) with gs = g exp(m - lse) evaluated once per row, and p_y
// and every p_id as group_p of that q, so two columns with equal logits and no copy mass have equal p in every comparison (rank is
// strict: an exact tie counts for neither), whatever form fast-math gives the surrounding code; on the device col_e's argument is
// made opaque for that.
// h() treats p below the smallest normal fp32 as 0: the device logarithm flushes denormals, and the term is < 1e-35.
#pragma once
#include "copy_eval_kernels.h"

namespace gtos_explain {

using gtos_eval::better;
using gtos_eval::gates;
using gtos_eval::group_mass;
using gtos_eval::group_p;
using gtos_eval::leads;

constexpr int NONE = 0x7fffffff;      // "no position" inside a reduction; written out as -1

GTOS_EV_HD float h(float p) { return p >= 1.17549435e-38f ? -p * GTOS_EV_LOG(p) : 0.f; }
// exp(x - m) of a column, the same bits at every site
GTOS_EV_HD float col_e(float x, float m) {
    float d = x - m;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(d));
#endif
    return GTOS_EV_EXP(d);
}
// (a, s) beats (a2, s2) as an alignment argmax: the larger weight, equal ones to the lower position
GTOS_EV_HD bool heavier(float a, int s, float a2, int s2) { return better(a, s, a2, s2); }
GTOS_EV_HD float vocab_entropy(float g, float Z, float E) { return h(g) + g * (GTOS_EV_LOG(Z) - E / Z); }
// q_y == 0 is tested first: cm / (0 + cm) must be exactly 1, and fast-math divides through an approximate reciprocal
GTOS_EV_HD float share(float q, float cm) { return q == 0.f ? (cm > 0.f ? 1.f : 0.f) : cm / (q + cm); }

// ---- host statement, one row (what the kernel computes, serially).  x: fp32 logits; cp: cp_seq [S, B]
inline void row_serial(const float* x, int V, float d0, float d1, const float* a, int S, const int64_t* cp, int B, int b, int64_t y,
                       int64_t pad, float* nll, float* entropy, float* gate, float* copy_share, int* source, float* source_weight,
                       int* focus, float* focus_weight, int* rank) {
    int pred_unused;
    float pp_unused;
    gtos_eval::row_serial(x, V, d0, d1, a, S, cp, B, b, y, pad, nll, &pred_unused, &pp_unused);      // nll: that code path, those bits
    float m = -INFINITY, Z = 0.f, E = 0.f;
    for (int k = 0; k < V; ++k)
        if (x[k] > m) m = x[k];
    for (int k = 0; k < V; ++k) Z += expf(x[k] - m);
    const float lse = m + logf(Z);
    float g, c;
    gates(d0, d1, g, c);
    const float gs = g * expf(m - lse);
    const bool live = y != pad && y >= 0;
    // the alignment: focus over all positions, source and the target's mass over those that hold y
    float fw = -INFINITY, sw = -INFINITY, mass_y = 0.f;
    int f = NONE, src = NONE;
    for (int s = 0; s < S; ++s) {
        if (heavier(a[s], s, fw, f)) { fw = a[s]; f = s; }
        if (live && cp[(int64_t)s * B + b] == y) {
            if (heavier(a[s], s, sw, src)) { sw = a[s]; src = s; }
            if (leads(cp + b, B, s)) mass_y = group_mass(cp + b, B, S, s, a);
        }
    }
    const bool reachable = live && (y < V || src != NONE);
    const float q_y = (reachable && y < V) ? gs * col_e(x[y], m) : 0.f;
    const float p_y = group_p(1.f, c, q_y, mass_y);
    // the logits row: E, and the vocabulary columns above the target
    int above = 0;
    for (int k = 0; k < V; ++k) {
        const float e = col_e(x[k], m);
        E += e * (x[k] - m);
        above += (k != y) && (gs * e > p_y);
    }
    float H = 0.f;
    for (int s = 0; s < S; ++s) {
        if (!leads(cp + b, B, s)) continue;
        const int64_t id = cp[(int64_t)s * B + b];
        const float q = id < V ? gs * col_e(x[id], m) : 0.f;
        const float p = group_p(1.f, c, q, group_mass(cp + b, B, S, s, a));
        H += h(p) - h(q);
        if (id != y) above += (int)(p > p_y) - (int)(id < V && q > p_y);
    }
    *entropy = vocab_entropy(g, Z, E) + H;
    *gate = c;
    *copy_share = reachable ? share(q_y, c * mass_y) : 0.f;
    *source = src == NONE ? -1 : src;
    *source_weight = src == NONE ? 0.f : sw;
    *focus = f == NONE ? -1 : f;
    *focus_weight = f == NONE ? 0.f : fw;
    *rank = reachable ? above : -1;
}

}  // namespace gtos_explain
