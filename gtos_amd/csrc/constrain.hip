// Lexically constrained beam search on the device (gtos_amd.search.beam_search_device with constraints): the advance of every beam by
// the rule of csrc/constrain_kernels.h (shared with the host check).  The top-k pass and the reorder are gtos_beam_topk /
// gtos_beam_reorder; nothing here synchronises with the host.
#include "beam_device.h"
#include "constrain_kernels.h"
#include "slot_device.h"

using namespace gtos_constrain;

namespace {

struct ConstrainArgs {
    BeamTables tb;
    int Cw;
    const float* ll;
    int64_t ld;
    const int* cons;
    int* met;
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
    const BeamTables& tb = a.tb;
    const int b = blockIdx.x, t = tb.t, k = tb.k;
    if (b == 0 && threadIdx.x == 0) tb.active[active_clear(t)] = 0;
    const int* st = tb.state + (int64_t)b * BS_WORDS;
    if (!tb.active[active_read(t)] || st[BS_DONE]) return;
    const int nlive = st[BS_NLIVE], ncomp = st[BS_NCOMP];
    if (!words_in_range(nlive, ncomp, k)) return;
    const int64_t N = (int64_t)tb.B * k;
    const int* met_t = a.met + (t % 2) * N;
    const int W = k + a.Cw, P = nlive * W;
    if (threadIdx.x == 0) present = 0;
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        const bool here = pool_entry(b, k, a.Cw, p, tb.topv, tb.topi, a.ll, a.ld, a.cons, tb.slot_score, met_t, tb.flag_shared,
                                     tb.flag_local, tb.V, tb.tot, ps + p, pt + p, pf + p, pm + p);
        pb[p] = here ? (signed char)bank_of(pm[p]) : (signed char)-1;
        if (here) atomicAdd(&present, 1);
    }
    __syncthreads();
    const int m = cut_size(present, k, ncomp);
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
        if (place(b, k, W, tb.min_t, tb.max_t, order, m, ps, pt, pf, pm, t, tb.state, tb.bp_parent + t * N, tb.bp_token + t * N,
                  tb.slot_score, tb.comp_step, tb.comp_parent, tb.comp_score, a.met + ((t + 1) % 2) * N))
            atomicOr(tb.active + active_set(t), 1);
    }
}

}  // namespace

extern "C" int gtos_constrain_advance(int B, int k, int Cw, int t, int V, int tot, int min_time_step, int max_time_step,
                                      const float* topv, const int* topi, const float* ll, int64_t ld, const int* cons,
                                      const uint8_t* flag_shared, const uint8_t* flag_local, double* slot_score, int* beam_state,
                                      int* bp_parent, int* bp_token, int* comp_step, int* comp_parent, double* comp_score, int* met,
                                      int* active, void* stream) {
    if (B <= 0) return 0;
    const ConstrainArgs a{{B, k, t, V, tot, min_time_step, max_time_step, topv, topi, flag_shared, flag_local, slot_score, beam_state,
                           bp_parent, bp_token, comp_step, comp_parent, comp_score, active}, Cw, ll, ld, cons, met};
    if (!sizes_ok(a.tb) || Cw < 0 || Cw > MAX_CONS || ld < tot) return -10;
    if (!tables_ok(a.tb) || !ll || (Cw > 0 && !cons) || !met) return -23;
    hipLaunchKernelGGL(constrain_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
