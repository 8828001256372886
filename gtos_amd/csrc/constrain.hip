// Lexically constrained beam search on the device (gtos_amd.search.beam_search_device with constraints): the advance of every beam by
// the rule of csrc/constrain_kernels.h (shared with the host check).  The top-k pass and the reorder are gtos_beam_topk /
// gtos_beam_reorder; nothing here synchronises with the host.
#include "constrain_kernels.h"
#include "slot_device.h"

using namespace gtos_constrain;

namespace {

struct ConstrainArgs {
    int B, k, Cw, t, V, tot, min_t, max_t;
    const float* topv;
    const int* topi;
    const float* ll;
    int64_t ld;
    const int* cons;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    double* slot_score;
    int* state;
    int* bp_parent;
    int* bp_token;
    int* comp_step;
    int* comp_parent;
    double* comp_score;
    int* met;
    int* active;
};

// One workgroup per beam.  The pool (at most MAX_POOL = 32 x 48 entries, 35 KB of LDS with its masks, banks and ranks) is filled by all
// threads, strided; the rank within the bank and then the final position are two O(P^2) counting passes, each behind a barrier -- the
// second only for entries whose q is below the cut, since an entry's final position is never below its q; the cut is placed by one
// thread.  The active[3] rotation of csrc/slot_kernels.h; the flag: did some not-done beam have a live slot when this iteration ended?
__global__ __launch_bounds__(NT) void constrain_advance_kernel(ConstrainArgs a) {
    __shared__ double ps[MAX_POOL];
    __shared__ int pt[MAX_POOL];
    __shared__ int pm[MAX_POOL];         // mask'
    __shared__ int pq[MAX_POOL];         // rank within the bank
    __shared__ uint8_t pf[MAX_POOL];
    __shared__ signed char pb[MAX_POOL]; // bank, -1: absent
    __shared__ int order[MAX_K];
    __shared__ int present;
    const int b = blockIdx.x, t = a.t;
    if (b == 0 && threadIdx.x == 0) a.active[active_clear(t)] = 0;
    const int* st = a.state + (int64_t)b * BS_WORDS;
    if (!a.active[active_read(t)] || st[BS_DONE]) return;
    const int nlive = st[BS_NLIVE], ncomp = st[BS_NCOMP];
    if (nlive < 0 || nlive > a.k || ncomp < 0 || ncomp >= a.k) return;        // (words outside a beam's range: left alone)
    const int64_t N = (int64_t)a.B * a.k;
    const int* met_t = a.met + (t % 2) * N;
    const int W = a.k + a.Cw, P = nlive * W;
    if (threadIdx.x == 0) present = 0;
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        const bool here = pool_entry(b, a.k, a.Cw, p, a.topv, a.topi, a.ll, a.ld, a.cons, a.slot_score, met_t, a.flag_shared,
                                     a.flag_local, a.V, a.tot, ps + p, pt + p, pf + p, pm + p);
        pb[p] = here ? (signed char)bank_of(pm[p]) : (signed char)-1;
        if (here) atomicAdd(&present, 1);
    }
    __syncthreads();
    const int m = cut_size(present, a.k, ncomp);
    for (int p = threadIdx.x; p < P; p += NT)
        if (pb[p] >= 0) pq[p] = rank_in_bank(ps, pb, P, p);
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        if (pb[p] < 0 || pq[p] >= m) continue;
        const int r = final_position(pq, pb, P, p);
        if (r < m) order[r] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (place(b, a.k, W, a.min_t, a.max_t, order, m, ps, pt, pf, pm, t, a.state, a.bp_parent + t * N, a.bp_token + t * N,
                  a.slot_score, a.comp_step, a.comp_parent, a.comp_score, a.met + ((t + 1) % 2) * N))
            atomicOr(a.active + active_set(t), 1);
    }
}

}  // namespace

extern "C" int gtos_constrain_advance(int B, int k, int Cw, int t, int V, int tot, int min_time_step, int max_time_step,
                                      const float* topv, const int* topi, const float* ll, int64_t ld, const int* cons,
                                      const uint8_t* flag_shared, const uint8_t* flag_local, double* slot_score, int* beam_state,
                                      int* bp_parent, int* bp_token, int* comp_step, int* comp_parent, double* comp_score, int* met,
                                      int* active, void* stream) {
    if (B <= 0) return 0;
    if (k < 1 || k > MAX_K || Cw < 0 || Cw > MAX_CONS || t < 0 || t >= max_time_step || V < 1 || tot < V || ld < tot) return -10;
    if (!topv || !topi || !ll || (Cw > 0 && !cons) || !flag_shared || (tot > V && !flag_local) || !slot_score || !beam_state ||
        !bp_parent || !bp_token || !comp_step || !comp_parent || !comp_score || !met || !active)
        return -23;
    ConstrainArgs a{};
    a.B = B; a.k = k; a.Cw = Cw; a.t = t; a.V = V; a.tot = tot; a.min_t = min_time_step; a.max_t = max_time_step;
    a.topv = topv; a.topi = topi; a.ll = ll; a.ld = ld; a.cons = cons; a.flag_shared = flag_shared; a.flag_local = flag_local;
    a.slot_score = slot_score; a.state = beam_state; a.bp_parent = bp_parent; a.bp_token = bp_token; a.comp_step = comp_step;
    a.comp_parent = comp_parent; a.comp_score = comp_score; a.met = met; a.active = active;
    hipLaunchKernelGGL(constrain_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
