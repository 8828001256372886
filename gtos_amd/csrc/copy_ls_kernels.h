// Per-row arithmetic of the label-smoothed generate/copy loss (csrc/copy_ls.hip), written so that the SAME code compiles for the
// host: tests/test_label_smoothing.py builds it with g++ and compares row_serial with a float64 numpy statement of the loss.
//
// Row r = (t, b) with target y, logits x [V], diverter (d0, d1), alignment a [S] and copy ids k_s = cp_seq[s, b]:
//   s = softmax(x), (g, c) = softmax(d0, d1), C = max(V, 1 + max(cp_seq)) for the whole batch,
//   p_k = g s_k [k < V] + c sum_{s: k_s == k} a_s,  ll_k = log(p_k + 1e-12),  k in [0, C)
//   loss = 0 at y == pad, else (1 - eps) (-ll_y) + (eps / C) (-sum_k ll_k)   (the reference's label_smoothed_nll_loss on its ll row)
// Gradient: w_k = dloss/dp_k = -((1 - eps) [k == y] + eps / C) / (p_k + 1e-12), Sw = sum_{k<V} w_k s_k, Sc = sum_s a_s w_{k_s};
//   dx_j = g s_j (w_j - Sw), dg = Sw, dc = Sc, da_s = c w_{k_s}, then the diverter softmax as gtos_copy_nll_bwd.
// w is linear in the upstream gradient, so the forward saves Sw and Sc per row and the backward is one pass over the row.
//
// Copy ids belong to a graph: the batch's groups of equal ids (valid ids are >= 0) are built once (gtos_copy_nll_ls_prep) as tables in
// one int32 workspace, laid out by Layout.  Group i of graph b is the i-th distinct id in first-occurrence order; its members are listed
// in ascending position, so every row sums a group's alignment mass in the same order.  A per-graph bitmap marks the vocabulary columns
// (< V) that are copy ids: the vocabulary pass skips them and the group pass adds their exact terms (no subtract-and-add cancellation).
// Columns >= V that no copy id of the graph names have p = 0: each adds log(1e-12) to the sum and nothing to the gradient, so the row
// sums offsets from log(1e-12) (col_off), which are 0 there, and adds C log(1e-12) once.  nbig[b] counts the distinct ids >= V.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GTOS_LS_HD __host__ __device__ inline
#else
#define GTOS_LS_HD inline
#endif

namespace gtos_ls {

constexpr float TINY = 1e-12f;
constexpr int MAX_S = 4096;           // source positions per graph (the backward keeps two words per group in LDS)

// int32 workspace: [0] = C; ngrp [B]; nbig [B]; gid [B,S]; gstart [B,S+1]; gpos [B,S]; grp [B,S] (-1: invalid id); bm [B,W]
struct Layout {
    int64_t ngrp, nbig, gid, gstart, gpos, grp, bm, W, total;
    GTOS_LS_HD Layout(int B, int S, int V) {
        W = ((int64_t)V + 31) / 32;
        ngrp = 4; nbig = ngrp + B; gid = nbig + B; gstart = gid + (int64_t)B * S; gpos = gstart + (int64_t)B * (S + 1);
        grp = gpos + (int64_t)B * S; bm = grp + (int64_t)B * S; total = bm + (int64_t)B * W;
    }
};

// ---- grouping helpers (one source position s of graph b; cp_seq is [S, B])
GTOS_LS_HD int64_t cp_id(const int64_t* cp, int B, int b, int s) { return cp[(int64_t)s * B + b]; }
// first position with the same id (s itself for a group's leader); -1 for an invalid (negative) id
GTOS_LS_HD int leader_of(const int64_t* cp, int B, int b, int s) {
    const int64_t id = cp_id(cp, B, b, s);
    if (id < 0) return -1;
    for (int j = 0; j < s; ++j)
        if (cp_id(cp, B, b, j) == id) return j;
    return s;
}
// positions before s with the same id (s's place in its group's member list)
GTOS_LS_HD int rank_in_group(const int64_t* cp, int B, int b, int s) {
    const int64_t id = cp_id(cp, B, b, s);
    int r = 0;
    for (int j = 0; j < s; ++j) r += cp_id(cp, B, b, j) == id;
    return r;
}
GTOS_LS_HD int group_size(const int64_t* cp, int B, int S, int b, int s) {
    const int64_t id = cp_id(cp, B, b, s);
    int n = 0;
    for (int j = s; j < S; ++j) n += cp_id(cp, B, b, j) == id;
    return n;
}

// ---- per-element arithmetic
// the smaller gate directly, the larger as 1 - it: c = 1 - g alone loses c's relative precision when c is small (a copy target's
// p then carries it into the loss)
GTOS_LS_HD void gates(float d0, float d1, float& g, float& c) {
    if (d1 > d0) {
        g = 1.f / (1.f + expf(d1 - d0));
        c = 1.f - g;
    } else {
        c = 1.f / (1.f + expf(d0 - d1));
        g = 1.f - c;
    }
}
GTOS_LS_HD float col_ll(float p) { return logf(p + TINY); }
// ll_k - log(1e-12) = log1p(p_k / 1e-12) >= 0: the row sums these offsets (0 for an empty column), not ll_k itself.  A peaked row has
// ~V columns at ll ~ log(1e-12) ~ -27.6, whose plain fp32 sum loses ~1e-4 of the row's loss; their offsets are ~0.
GTOS_LS_HD float col_off(float p) { return log1pf(p / TINY); }
// dloss/dp of a column (per unit upstream gradient)
GTOS_LS_HD float col_w(float p, bool is_tgt, float eps, float eps_c) { return -((is_tgt ? 1.f - eps : 0.f) + eps_c) / (p + TINY); }
// sum_k ll_k = C log(1e-12) + sum_off, and eps_c * C = eps
GTOS_LS_HD float row_loss(float p_tgt, float sum_off, float eps, float eps_c) {
    return (1.f - eps) * -col_ll(p_tgt) - eps * col_ll(0.f) - eps_c * sum_off;
}
GTOS_LS_HD float d_logit(float u, float g, float s, float w, float sw) { return u * g * s * (w - sw); }
// d d0 = g (dg - m), d d1 = c (dc - m), m = g dg + c dc; with g + c = 1 that is g c (dg - dc) and its negative (no cancellation)
GTOS_LS_HD void d_gates(float u, float g, float c, float sw, float sc, float& dd0, float& dd1) {
    dd0 = g * c * (u * sw - u * sc);
    dd1 = -dd0;
}
GTOS_LS_HD bool bit(const int* bm, int k) { return (((uint32_t)bm[k >> 5]) >> (k & 31)) & 1u; }

// ---- host statement, one graph / one row (what the kernels compute, serially).  ws: the workspace of Layout(B, S, V)
inline void build_graph_serial(const int64_t* cp, int B, int S, int V, int b, int* ws) {
    const Layout L(B, S, V);
    int* gid = ws + L.gid + (int64_t)b * S;
    int* gstart = ws + L.gstart + (int64_t)b * (S + 1);
    int* gpos = ws + L.gpos + (int64_t)b * S;
    int* grp = ws + L.grp + (int64_t)b * S;
    int* bm = ws + L.bm + (int64_t)b * L.W;
    for (int64_t w = 0; w < L.W; ++w) bm[w] = 0;
    int ng = 0, nbig = 0, at = 0;
    for (int s = 0; s < S; ++s) {
        if (leader_of(cp, B, b, s) != s) continue;
        const int64_t id = cp_id(cp, B, b, s);
        gid[ng] = (int)id;
        gstart[ng] = at;
        at += group_size(cp, B, S, b, s);
        nbig += id >= V;
        if (id < V) bm[id >> 5] |= (int)(1u << (id & 31));
        ++ng;
    }
    gstart[ng] = at;
    for (int s = 0; s < S; ++s) {
        const int l = leader_of(cp, B, b, s);
        if (l < 0) { grp[s] = -1; continue; }
        int gi = 0;
        for (int j = 0; j < l; ++j) gi += leader_of(cp, B, b, j) == j;
        grp[s] = gi;
        gpos[gstart[gi] + rank_in_group(cp, B, b, s)] = s;
    }
    ws[L.ngrp + b] = ng;
    ws[L.nbig + b] = nbig;
}

// the whole workspace (what gtos_copy_nll_ls_prep writes), serially
inline void build_serial(const int64_t* cp, int B, int S, int V, int* ws) {
    int64_t m = -1;
    for (int64_t i = 0; i < (int64_t)S * B; ++i) m = cp[i] > m ? cp[i] : m;
    ws[0] = (int)(m + 1 > V ? m + 1 : V);
    for (int b = 0; b < B; ++b) build_graph_serial(cp, B, S, V, b, ws);
}

// alignment mass of group gi on one row (members in ascending position)
GTOS_LS_HD float group_mass(const int* gstart, const int* gpos, int gi, const float* a) {
    float m = 0.f;
    for (int i = gstart[gi]; i < gstart[gi + 1]; ++i) m += a[gpos[i]];
    return m;
}

// One row: loss, the saved sums (Sw, Sc) and, for upstream gradient u, dx [V], (dd0, dd1), da [S].  x: fp32 logits.
inline void row_serial(const float* x, int V, float d0, float d1, const float* a, int S, int B, int b, int64_t y, int64_t pad,
                       float eps, const int* ws, float u, float* loss, float* sums, float* dx, float* dd, float* da) {
    const Layout L(B, S, V);
    const int C = ws[0];
    const float eps_c = eps / (float)C;
    const int* gid = ws + L.gid + (int64_t)b * S;
    const int* gstart = ws + L.gstart + (int64_t)b * (S + 1);
    const int* gpos = ws + L.gpos + (int64_t)b * S;
    const int* grp = ws + L.grp + (int64_t)b * S;
    const int* bm = ws + L.bm + (int64_t)b * L.W;
    const int ng = ws[L.ngrp + b];
    float mx = -INFINITY, se = 0.f;
    for (int k = 0; k < V; ++k) mx = fmaxf(mx, x[k]);
    for (int k = 0; k < V; ++k) se += expf(x[k] - mx);
    const float lse = mx + logf(se);
    float g, c;
    gates(d0, d1, g, c);
    float sll = 0.f, sw = 0.f, sc = 0.f, py = 0.f;
    for (int k = 0; k < V; ++k) {
        if (bit(bm, k)) continue;
        const float s = expf(x[k] - lse), p = g * s;
        sll += col_off(p);
        sw += col_w(p, k == y, eps, eps_c) * s;
        if (k == y) py = p;
    }
    float* wg = new float[ng > 0 ? ng : 1];
    for (int gi = 0; gi < ng; ++gi) {
        const int id = gid[gi];
        const float m = group_mass(gstart, gpos, gi, a);
        const float s = id < V ? expf(x[id] - lse) : 0.f;
        const float p = g * s + c * m, w = col_w(p, id == y, eps, eps_c);
        sll += col_off(p);
        sw += w * s;
        sc += m * w;
        if (id == y) py = p;
        wg[gi] = w;
    }
    const bool is_pad = y == pad;
    *loss = is_pad ? 0.f : row_loss(py, sll, eps, eps_c);
    sums[0] = sw;
    sums[1] = sc;
    if (is_pad) u = 0.f;
    for (int j = 0; j < V; ++j) {
        const float s = expf(x[j] - lse);
        float w;
        if (bit(bm, j)) {
            int gi = 0;
            while (gid[gi] != j) ++gi;
            w = wg[gi];
        } else {
            w = col_w(g * s, j == y, eps, eps_c);
        }
        dx[j] = d_logit(u, g, s, w, sw);
    }
    d_gates(u, g, c, sw, sc, dd[0], dd[1]);
    for (int s = 0; s < S; ++s) da[s] = grp[s] >= 0 ? u * c * wg[grp[s]] : 0.f;
    delete[] wg;
}

}  // namespace gtos_ls
