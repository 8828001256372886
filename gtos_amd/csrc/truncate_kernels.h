// Distribution-shaped truncation of the device-resident sampling decode (csrc/truncate.hip): min-p, locally typical and epsilon / eta
// cuts, written so that the SAME code compiles for the host: tests/test_truncate_sample.py builds it with g++ and compares
// truncate_serial with a numpy statement of the rule on random rows.  The kernel runs the same helpers.
//
// One row = one live slot at step t, ll as it arrives (after the n-gram / avoid bans).  A = the allowed set of rule 1 of
// csrc/sample_kernels.h.  All arithmetic is fp64; x_c = (double)ll_c / T; T and the four parameters enter as fp32 values (the C ABI
// passes them so).  The stages run in this order, each on the survivors of the one before, renormalised; a stage that is off is skipped:
//  1. min_p in (0, 1] (0 = off): with m = max x, keep x_c >= m + log(min_p).  min_p = 1 keeps exactly the columns at the maximum.
//  2. typical_p in (0, 1) (1 = off): Z = sum exp(x_c - m), E = sum exp(x_c - m)(x_c - m), H = log Z - E / Z (the entropy),
//     dev_c = |-(x_c - m - log Z) - H| rounded to fp32; keep {dev_c <= d*}, d* the smallest deviation value whose set holds a mass
//     >= typical_p * Z; ties at d* are all kept.  (m is still the maximum: stage 1 never removes it.)
//  3. epsilon_cutoff e in [0, 1) and eta_cutoff h in [0, 1) (0 = off): with m', Z', H' over the survivors and p'_c = exp(x_c - m') / Z',
//     thr = the larger of e (if on) and min(h, sqrt(h) exp(-H')) (if on); keep p'_c >= thr, and always the best survivor by
//     gtos_slot::before.
// Every column of A that did not survive gets ll = -inf; a column outside A and every survivor keep their bits; a row with empty A is
// left alone.  The set is never empty when A is not: the maximum survives stage 1, the columns at d* stage 2, the best one stage 3.
// top_k / top_p then act in gtos_sample_step on what is left.
#pragma once
#include <math.h>

#include "sample_kernels.h"

#define GTOS_TRUNC_HD GTOS_SLOT_HD

namespace gtos_truncate {

using namespace gtos_sample;            // allowed(), order_key / order_value, bisect_mid, before(), SS_DEAD, the active[3] rotation

GTOS_TRUNC_HD double scaled(float ll, double T) { return (double)ll / T; }
// stage 1: the smallest x that stays (log 1 = 0 exactly)
GTOS_TRUNC_HD double min_p_threshold(double m, double min_p) { return m + log(min_p); }
// stage 2 / 3: the entropy of the renormalised survivors from their sums
GTOS_TRUNC_HD double entropy(double Z, double E) { return log(Z) - E / Z; }
// stage 2: how far the information content of a column lies from the entropy, as the fp32 value the cut orders by
GTOS_TRUNC_HD float deviation(double x, double m, double logZ, double H) { return (float)fabs(-(x - m - logZ) - H); }
// stage 3: the probability below which a survivor goes (one of the two is on)
GTOS_TRUNC_HD double tail_threshold(double eps, double eta, double H) {
    double thr = eps > 0.0 ? eps : 0.0;
    if (eta > 0.0) {
        const double a = sqrt(eta) * exp(-H);
        const double e = eta < a ? eta : a;
        thr = e > thr ? e : thr;
    }
    return thr;
}

// Stage 2's search for d* is a bisection over order_key(dev) in (klo, khi]: klo never holds the mass, khi always does and is a
// deviation of the row.  After a pass that probed mid (enough: {dev <= order_value(mid)} holds the mass), with below the largest
// deviation <= order_value(mid) and above the smallest in (order_value(mid), order_value(khi)], the ends can move onto those values:
// {dev <= mid} = {dev <= below} and {dev <= mid} = {dev < above}.  The bounds checks keep every pass at least halving the interval.
GTOS_TRUNC_HD void narrow(uint32_t& klo, uint32_t& khi, uint32_t mid, bool enough, float below, float above) {
    const uint32_t kb = order_key(below), ka = order_key(above) - 1;
    if (enough) khi = (kb > klo && kb <= mid) ? kb : mid;
    else klo = (ka >= mid && ka < khi) ? ka : mid;
}

// What decides whether an allowed column survives stages 1 and 2; set membership is recomputed from it in every pass
struct Cut {
    bool min_p, typical;
    double thr1;                        // stage 1
    double m, logZ, H;                  // stage 2
    float dstar;
};
GTOS_TRUNC_HD bool survives(const Cut& q, double x) {
    if (q.min_p && !(x >= q.thr1)) return false;
    return !q.typical || deviation(x, q.m, q.logZ, q.H) <= q.dstar;
}
// ... and stage 3: m2 / Z2 of the survivors, best their first column by before() (thr < 0: the stage is off)
struct Tail {
    double thr, m2, Z2;
    int best;
};
GTOS_TRUNC_HD bool survives_tail(const Tail& q, double x, int c) { return q.thr < 0.0 || c == q.best || exp(x - q.m2) / q.Z2 >= q.thr; }

// The whole rule on one row by one thread, in place (the host check; the kernel spreads the passes over a workgroup).  Returns the
// number of survivors, or -1 when no column is allowed (the row is left alone).
GTOS_TRUNC_HD int truncate_serial(float* ll, int tot, int V, int b, int t, int min_time_step, const uint8_t* flag_shared,
                                  const uint8_t* flag_local, const uint8_t* owned_local, double T, double min_p, double typical_p,
                                  double eps, double eta) {
    float mx = -INFINITY;
    for (int c = 0; c < tot; ++c)
        if (allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) mx = ll[c] > mx ? ll[c] : mx;
    if (!(mx > -INFINITY)) return -1;
    Cut q{};
    q.m = scaled(mx, T);
    q.min_p = min_p > 0.0;
    if (q.min_p) q.thr1 = min_p_threshold(q.m, min_p);
    if (typical_p < 1.0) {
        double Z = 0.0, E = 0.0;
        for (int c = 0; c < tot; ++c) {
            if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
            const double x = scaled(ll[c], T);
            if (!survives(q, x)) continue;
            const double w = exp(x - q.m);
            Z += w;
            E += w * (x - q.m);
        }
        q.logZ = log(Z);
        q.H = entropy(Z, E);
        float dmin = INFINITY, dmax = 0.0f;
        for (int c = 0; c < tot; ++c) {
            if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
            const double x = scaled(ll[c], T);
            if (!survives(q, x)) continue;
            const float d = deviation(x, q.m, q.logZ, q.H);
            dmin = d < dmin ? d : dmin;
            dmax = d > dmax ? d : dmax;
        }
        // the smallest key in (klo, khi] whose set {dev <= order_value(key)} holds the mass; klo never qualifies, khi always does
        // (the kernel probes the same sets and, between passes, pulls both ends onto deviations of the row)
        uint32_t klo = order_key(dmin) - 1, khi = order_key(dmax);
        while (khi - klo > 1) {
            const uint32_t mid = bisect_mid(klo, khi);
            const float v = order_value(mid);
            double mass = 0.0;
            for (int c = 0; c < tot; ++c) {
                if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
                const double x = scaled(ll[c], T);
                if (survives(q, x) && deviation(x, q.m, q.logZ, q.H) <= v) mass += exp(x - q.m);
            }
            if (mass >= typical_p * Z) khi = mid;
            else klo = mid;
        }
        q.dstar = order_value(khi);
        q.typical = true;
    }
    Tail r{};
    r.thr = -1.0;
    if (eps > 0.0 || eta > 0.0) {
        float bv = -INFINITY;
        int bc = -1;
        for (int c = 0; c < tot; ++c) {
            if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
            if (survives(q, scaled(ll[c], T)) && (bc < 0 || before(ll[c], c, bv, bc))) { bv = ll[c]; bc = c; }
        }
        r.best = bc;
        r.m2 = scaled(bv, T);
        double Z = 0.0, E = 0.0;
        for (int c = 0; c < tot; ++c) {
            if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
            const double x = scaled(ll[c], T);
            if (!survives(q, x)) continue;
            const double w = exp(x - r.m2);
            Z += w;
            E += w * (x - r.m2);
        }
        r.Z2 = Z;
        r.thr = tail_threshold(eps, eta, entropy(Z, E));
    }
    int kept = 0;
    for (int c = 0; c < tot; ++c) {
        if (!allowed(flag_shared, flag_local, owned_local, V, tot, b, c, t, min_time_step, ll[c])) continue;
        const double x = scaled(ll[c], T);
        if (survives(q, x) && survives_tail(r, x, c)) ++kept;
        else ll[c] = -INFINITY;
    }
    return kept;
}

}  // namespace gtos_truncate
