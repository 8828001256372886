// Distribution-shaped truncation for the device-resident sampling decode (gtos_amd.search.sample_device), rule in
// csrc/truncate_kernels.h (shared with the host check): min-p, locally typical and epsilon / eta cuts.  One launch per step, after
// the decoder's ll (and gtos_ngram_block / gtos_avoid_block) and before gtos_sample_step: the columns of a live slot's row that the
// cuts remove are set to -inf, so the sampler's allowed set is what survived.  sample_step_kernel's shape, one workgroup per slot
// row: a max pass, an fp64 pass for the normaliser and the entropy, a threshold bisection over the deviations with fp64 block sums
// over the row, a best-column pass and a second normaliser for the tail cut, then the stores.  Rows are read from global memory as
// often as the passes need (they stay in L2 / MALL); LDS holds the partial results only, and whether a column is still in the set
// is recomputed in every pass from a handful of scalars.  Nothing here synchronises with the host.
#include "truncate_kernels.h"
#include "slot_device.h"

using namespace gtos_truncate;

namespace {

struct TruncArgs {
    int N, k, t, V, tot, min_t;
    double T, min_p, typical_p, eps, eta;
    float* ll;
    int64_t ld;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    const uint8_t* owned_local;
    const int* state;
    const int* active_t;                // the flag step t's kernels read
};

__device__ __forceinline__ bool col_allowed(const TruncArgs& a, int b, int c, float y) {
    return allowed(a.flag_shared, a.flag_local, a.owned_local, a.V, a.tot, b, c, a.t, a.min_t, y);
}

// the first (value, column) by before(), INT_MAX when no thread has one; every thread gets the result
__device__ void block_best(float& bv, int& bc, float* rv, int* rc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oc = __shfl_xor(bc, o);
        if (before(ov, oc, bv, bc)) { bv = ov; bc = oc; }
    }
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = bv; rc[threadIdx.x >> 6] = bc; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if (before(rv[w], rc[w], bv, bc)) { bv = rv[w]; bc = rc[w]; }
    __syncthreads();
}

// Z = sum exp(x - m) and E = sum exp(x - m)(x - m) over the survivors of q
__device__ void block_moments(const TruncArgs& a, const float* x, int b, const Cut& q, double m, double* red, double& Z, double& E) {
    double z = 0.0, e = 0.0;
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (!col_allowed(a, b, c, y)) continue;
        const double xs = scaled(y, a.T);
        if (!survives(q, xs)) continue;
        const double w = exp(xs - m);
        z += w;
        e += w * (xs - m);
    }
    Z = block_sum(z, red);
    E = block_sum(e, red);
}

// One workgroup per slot; a step that does not run and a dead slot leave the row alone
__global__ __launch_bounds__(NT) void truncate_block_kernel(TruncArgs a) {
    __shared__ double rd[NW];
    __shared__ float rmx[NW], rmn[NW];
    __shared__ int rc[NW];
    const int s = blockIdx.x, b = s / a.k;
    if (!*a.active_t || a.state[(int64_t)s * SS_WORDS + SS_DEAD]) return;
    float* x = a.ll + (int64_t)s * a.ld;
    float mx = -INFINITY, mn = INFINITY;
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (col_allowed(a, b, c, y)) { mx = fmaxf(mx, y); mn = fminf(mn, y); }
    }
    block_minmax(mx, mn, rmx, rmn);
    if (!(mx > -INFINITY)) return;
    Cut q{};
    q.m = scaled(mx, a.T);
    q.min_p = a.min_p > 0.0;
    if (q.min_p) q.thr1 = min_p_threshold(q.m, a.min_p);
    if (a.typical_p < 1.0) {
        double Z, E;
        block_moments(a, x, b, q, q.m, rd, Z, E);
        q.logZ = log(Z);
        q.H = entropy(Z, E);
        float dmax = 0.0f, dmin = INFINITY;
        for (int c = threadIdx.x; c < a.tot; c += NT) {
            const float y = x[c];
            if (!col_allowed(a, b, c, y)) continue;
            const double xs = scaled(y, a.T);
            if (!survives(q, xs)) continue;
            const float d = deviation(xs, q.m, q.logZ, q.H);
            dmax = fmaxf(dmax, d);
            dmin = fminf(dmin, d);
        }
        block_minmax(dmax, dmin, rmx, rmn);
        // truncate_serial's bisection (klo never qualifies, khi always does and is a deviation of the row), with both ends pulled
        // onto the row's own values after every pass: the sets {dev <= mid} and {dev <= the largest deviation <= mid} are the
        // same, and so are {dev <= mid} and {dev < the smallest deviation above mid}.  Same d*, about log2(columns) passes
        // instead of 31, never more than the plain bisection's.
        uint32_t klo = order_key(dmin) - 1, khi = order_key(dmax);
        while (khi - klo > 1) {
            const uint32_t mid = bisect_mid(klo, khi);
            const float v = order_value(mid), vhi = order_value(khi);
            double mass = 0.0;
            float below = -INFINITY, above = INFINITY;          // the largest deviation <= v, the smallest in (v, vhi]
            for (int c = threadIdx.x; c < a.tot; c += NT) {
                const float y = x[c];
                if (!col_allowed(a, b, c, y)) continue;
                const double xs = scaled(y, a.T);
                if (!survives(q, xs)) continue;
                const float d = deviation(xs, q.m, q.logZ, q.H);
                if (d <= v) {
                    mass += exp(xs - q.m);
                    below = fmaxf(below, d);
                } else if (d <= vhi) {
                    above = fminf(above, d);
                }
            }
            const bool enough = block_sum(mass, rd) >= a.typical_p * Z;
            block_minmax(below, above, rmx, rmn);
            narrow(klo, khi, mid, enough, below, above);
        }
        q.dstar = order_value(khi);
        q.typical = true;
    }
    Tail r{};
    r.thr = -1.0;
    if (a.eps > 0.0 || a.eta > 0.0) {
        float bv = -INFINITY;
        int bc = INT_MAX;
        for (int c = threadIdx.x; c < a.tot; c += NT) {
            const float y = x[c];
            if (col_allowed(a, b, c, y) && survives(q, scaled(y, a.T)) && before(y, c, bv, bc)) { bv = y; bc = c; }
        }
        block_best(bv, bc, rmx, rc);
        r.best = bc;
        r.m2 = scaled(bv, a.T);
        double E;
        block_moments(a, x, b, q, r.m2, rd, r.Z2, E);
        r.thr = tail_threshold(a.eps, a.eta, entropy(r.Z2, E));
    }
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (!col_allowed(a, b, c, y)) continue;
        const double xs = scaled(y, a.T);
        if (!(survives(q, xs) && survives_tail(r, xs, c))) x[c] = -INFINITY;
    }
}

}  // namespace

extern "C" int gtos_truncate_block(int N, int k, int t, int V, int tot, int min_time_step, float temperature, float min_p,
                                   float typical_p, float epsilon_cutoff, float eta_cutoff, float* ll, int64_t ld,
                                   const uint8_t* flag_shared, const uint8_t* flag_local, const uint8_t* owned_local,
                                   const int* slot_state, const int* active, void* stream) {
    if (N <= 0) return 0;
    if (k < 1 || N % k || t < 0 || V < 1 || tot < V || ld < tot || !(temperature > 0.0f && temperature < INFINITY) ||
        !(min_p >= 0.0f && min_p <= 1.0f) || !(typical_p > 0.0f && typical_p <= 1.0f) ||
        !(epsilon_cutoff >= 0.0f && epsilon_cutoff < 1.0f) || !(eta_cutoff >= 0.0f && eta_cutoff < 1.0f) ||
        (min_p == 0.0f && typical_p == 1.0f && epsilon_cutoff == 0.0f && eta_cutoff == 0.0f))
        return -10;
    if (!ll || !flag_shared || (tot > V && (!flag_local || !owned_local)) || !slot_state || !active) return -23;
    TruncArgs a{};
    a.N = N; a.k = k; a.t = t; a.V = V; a.tot = tot; a.min_t = min_time_step;
    a.T = (double)temperature; a.min_p = (double)min_p; a.typical_p = (double)typical_p; a.eps = (double)epsilon_cutoff;
    a.eta = (double)eta_cutoff; a.ll = ll; a.ld = ld; a.flag_shared = flag_shared; a.flag_local = flag_local;
    a.owned_local = owned_local; a.state = slot_state; a.active_t = active + active_read(t);
    hipLaunchKernelGGL(truncate_block_kernel, dim3((unsigned)N), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
