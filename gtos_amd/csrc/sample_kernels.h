// Selection rule of the device-resident sampling decode (csrc/sample.hip), written so that the SAME code compiles for the host:
// tests/test_sample_decode.py builds it with g++ and compares select_serial with a numpy statement of the rule on random rows.  The
// kernel runs the same helpers: the allowed set, the top-p cut of a sorted candidate list, the weights, the counter hash and the
// Gumbel keys, and the slot update.
//
// Slots as in csrc/slot_kernels.h; slot s is sample s % k of graph s / k.  One row = one live slot at step t:
//  1. allowed: columns c in [0, tot) with a finite ll, except <UNK> strings, copy ids c >= V the slot's graph does not own, and <END>
//     while t < min_time_step;
//  2. top-k (top_k > 0): the allowed columns ranked < top_k in (ll descending, column ascending) order;
//  3. top-p (top_p < 1): with w_c = exp((ll_c - max) / T) summed in fp64, keep {c : ll_c >= v*}, v* the largest kept ll value whose
//     set holds a mass >= top_p * sum(w); ties at the cutoff are all kept;
//  4. draw: the kept column with the largest ll_c / T + g_c (fp64, ties to the lower column), g_c = -log(-log(u_c)), u_c from the top
//     53 bits of a splitmix64 hash of (seed, graph, sample, t, c).  T and top_p enter as fp32 values (the C ABI passes them so).
// A row with no allowed column stops its slot unfinished (no token).  Gumbel-max needs no sort and no fixed reduction order.
#pragma once
#include <math.h>

#include "slot_kernels.h"

#define GTOS_SAMPLE_HD GTOS_SLOT_HD

namespace gtos_sample {

using namespace gtos_slot;              // token classes, token_flag, before() (rule 2's order), the active[3] rotation
// per-slot state words, int32 [N, SS_WORDS]: steps taken part in, completion step (<END>) or -1, dead (ended or stopped)
enum { SS_STEPS = 0, SS_END = 1, SS_DEAD = 2, SS_WORDS = 3 };
constexpr int MAX_TOPK = 32;

constexpr uint64_t GOLD = 0x9E3779B97F4A7C15ull, MIX1 = 0xBF58476D1CE4E5B9ull, MIX2 = 0x94D049BB133111EBull;

GTOS_SAMPLE_HD uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * MIX1;
    z = (z ^ (z >> 27)) * MIX2;
    return z ^ (z >> 31);
}
// draw i of the splitmix64 stream seeded with s (gtos_amd.synth.SplitMix64(s).u64(i + 1)[i])
GTOS_SAMPLE_HD uint64_t draw(uint64_t s, uint64_t i) { return mix64(s + (i + 1) * GOLD); }
// the stream of one (graph, sample, step) row: column c draws draw(row_key, c)
GTOS_SAMPLE_HD uint64_t row_key(uint64_t seed, int g, int j, int t) {
    return draw(draw(draw(seed, (uint64_t)g), (uint64_t)j), (uint64_t)t);
}
// u = (m + 0.5) * 2^-53 from the top 53 bits m; m = 2^53 - 1 rounds to 1, clamped to the largest double below 1
GTOS_SAMPLE_HD double uniform(uint64_t key, int c) {
    const double u = ((double)(draw(key, (uint64_t)c) >> 11) + 0.5) * 0x1p-53;
    return u < 1.0 ? u : 1.0 - 0x1p-53;
}
GTOS_SAMPLE_HD double gumbel(uint64_t key, int c) { return -log(-log(uniform(key, c))); }
GTOS_SAMPLE_HD double draw_key(float ll, double T, uint64_t key, int c) { return (double)ll / T + gumbel(key, c); }
// the top-p weight of a column, m the largest kept ll
GTOS_SAMPLE_HD double weight(float ll, float m, double T) { return exp(((double)ll - (double)m) / T); }

// draw key a beats b: larger key, equal keys lower column
GTOS_SAMPLE_HD bool wins(double ka, int ca, double kb, int cb) { return ka > kb || (ka == kb && ca < cb); }

// rule 1 for column c of graph b at step t.  owned_local uint8 [B, tot-V]: 1 where local_idx2token of graph b holds the copy id
GTOS_SAMPLE_HD bool allowed(const uint8_t* flag_shared, const uint8_t* flag_local, const uint8_t* owned_local, int V, int tot, int b,
                            int c, int t, int min_time_step, float ll) {
    if (!(ll > -INFINITY && ll < INFINITY)) return false;              // -inf, +inf and NaN are never drawn
    if (c >= V && !owned_local[local_index(V, tot, b, c)]) return false;
    const uint8_t f = token_flag(flag_shared, flag_local, V, tot, b, c);
    return f == TOK_PLAIN || (f == TOK_END && t >= min_time_step);
}

// fp32 <-> an unsigned key of the same order (for the top-p threshold bisection; finite values only)
GTOS_SAMPLE_HD uint32_t order_key(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
GTOS_SAMPLE_HD float order_value(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// Rule 3 on n candidates sorted by before(): how many the top-p cut keeps (all with top_p >= 1).  Sums in rank order.
GTOS_SAMPLE_HD int topp_keep_sorted(const float* v, int n, double T, double top_p) {
    if (top_p >= 1.0 || n <= 1) return n;
    double Z = 0.0;
    for (int i = 0; i < n; ++i) Z += weight(v[i], v[0], T);
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        acc += weight(v[i], v[0], T);
        if ((i + 1 == n || v[i + 1] < v[i]) && acc >= top_p * Z) return i + 1;
    }
    return n;
}

// One bisection step of rule 3 over the whole row: the largest key K in [lo, hi) whose set {ll >= order_value(K)} holds a mass
// >= top_p * Z.  Invariant: lo qualifies, hi does not.  The answer is a kept ll value (the mass only changes at one).
GTOS_SAMPLE_HD uint32_t bisect_mid(uint32_t lo, uint32_t hi) { return lo + (hi - lo) / 2; }

// The whole selection of one row by one thread (the host check; the kernel spreads the passes over a workgroup).  kv / kc: scratch
// of MAX_TOPK entries.  Returns the winning column, or -1 when no column is allowed.
GTOS_SAMPLE_HD int select_serial(const float* ll, int tot, int V, int b, int j, int t, int min_time_step, const uint8_t* flag_shared,
                                 const uint8_t* flag_local, const uint8_t* owned_local, double T, int top_k, double top_p,
                                 uint64_t seed, float* kv, int* kc) {
    const uint64_t key = row_key(seed, b, j, t);
    int best = -1;
    double best_key = -INFINITY;
    if (top_k > 0) {
        int n = 0;
        for (int c = 0; c < tot; ++c) {
            if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
            if (n == top_k && !before(ll[c], c, kv[n - 1], kc[n - 1])) continue;
            int i = n < top_k ? n++ : n - 1;
            for (; i > 0 && before(ll[c], c, kv[i - 1], kc[i - 1]); --i) { kv[i] = kv[i - 1]; kc[i] = kc[i - 1]; }
            kv[i] = ll[c];
            kc[i] = c;
        }
        n = topp_keep_sorted(kv, n, T, top_p);
        for (int i = 0; i < n; ++i) {
            const double dk = draw_key(kv[i], T, key, kc[i]);
            if (best < 0 || wins(dk, kc[i], best_key, best)) { best_key = dk; best = kc[i]; }
        }
        return best;
    }
    float m = -INFINITY, lo = INFINITY;
    for (int c = 0; c < tot; ++c)
        if (allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) {
            m = ll[c] > m ? ll[c] : m;
            lo = ll[c] < lo ? ll[c] : lo;
        }
    if (!(m > -INFINITY)) return -1;
    float vstar = lo;
    if (top_p < 1.0) {
        double Z = 0.0;
        for (int c = 0; c < tot; ++c)
            if (allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) Z += weight(ll[c], m, T);
        uint32_t klo = order_key(lo), khi = order_key(m) + 1;
        while (khi - klo > 1) {
            const uint32_t mid = bisect_mid(klo, khi);
            const float v = order_value(mid);
            double mass = 0.0;
            for (int c = 0; c < tot; ++c)
                if (ll[c] >= v && allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c]))
                    mass += weight(ll[c], m, T);
            if (mass >= top_p * Z) klo = mid;
            else khi = mid;
        }
        vstar = order_value(klo);
    }
    for (int c = 0; c < tot; ++c)
        if (ll[c] >= vstar && allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) {
            const double dk = draw_key(ll[c], T, key, c);
            if (best < 0 || wins(dk, c, best_key, best)) { best_key = dk; best = c; }
        }
    return best;
}

// Rule 5 for slot s after its row picked w (or -1) at step t: the state words, the fp64 score, row t of the token table ([N]).
// Returns true when the slot samples again at step t + 1.
GTOS_SAMPLE_HD bool update(int s, int t, int max_time_step, int w, float ll_w, uint8_t flag_w, double* score, int* slot_state,
                           int* tokens_t) {
    int* st = slot_state + (int64_t)s * SS_WORDS;
    st[SS_STEPS] = t + 1;
    if (w < 0) {                                  // nothing allowed: the slot stops unfinished
        st[SS_DEAD] = 1;
        return false;
    }
    score[s] += (double)ll_w;
    tokens_t[s] = w;
    if (flag_w == TOK_END) {
        st[SS_END] = t;
        st[SS_DEAD] = 1;
        return false;
    }
    return t + 1 < max_time_step;
}

}  // namespace gtos_sample
