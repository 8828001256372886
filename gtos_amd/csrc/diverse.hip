// Diverse (group) beam search on the device (gtos_amd.search.beam_search_device with groups / diversity): the advance of every
// graph's groups (selection rule in csrc/diverse_kernels.h, shared with the host check) and the reorder with per-group liveness
// (csrc/reorder_device.h, the kernel of gtos_beam_reorder).  The top-k pass is gtos_beam_topk; nothing here synchronises with the host.
#include "beam_device.h"
#include "diverse_kernels.h"
#include "reorder_device.h"
#include "slot_device.h"

#include <string.h>

using namespace gtos_diverse;

namespace {

struct DiverseArgs {
    BeamTables tb;                      // state: one row per group
    int G;
    double lambda;
};

// One workgroup per graph, its groups one after the other: the pool is filled (the count over the chosen list a linear scan of
// LDS) and ranked by all threads, strided when it is larger than the workgroup (G = 1, k = 32: 1024 entries), the cut is placed by
// one thread, which also appends to the chosen list; the barrier after it publishes the list to the next group's fill.  The
// active[3] rotation of csrc/slot_kernels.h; the flag: did some not-done group have a live slot when this iteration ended?
__global__ __launch_bounds__(NT) void diverse_advance_kernel(DiverseArgs a) {
    __shared__ double pk[MAX_POOL];      // selection key
    __shared__ double pm[MAX_POOL];      // model score
    __shared__ int pt[MAX_POOL];
    __shared__ uint8_t pf[MAX_POOL];
    __shared__ int order[MAX_K];
    __shared__ int chosen[MAX_K];
    __shared__ int n_chosen;
    const BeamTables& tb = a.tb;
    const int b = blockIdx.x, t = tb.t, k = tb.k, g = k / a.G;
    if (b == 0 && threadIdx.x == 0) tb.active[active_clear(t)] = 0;
    if (!tb.active[active_read(t)]) return;
    if (threadIdx.x == 0) n_chosen = 0;
    __syncthreads();
    bool go = false;                     // thread 0's
    for (int j = 0; j < a.G; ++j) {
        const int q = b * a.G + j;
        const int* st = tb.state + (int64_t)q * BS_WORDS;
        // the group's words are written by thread 0 only, behind the two barriers below: every thread reads the same values
        const int nlive = st[BS_NLIVE], ncomp = st[BS_NCOMP];
        if (st[BS_DONE] || !words_in_range(nlive, ncomp, g)) continue;
        const int P = nlive * k, nc = n_chosen;
        const int m = cut_size(P, g, ncomp);
        for (int p = threadIdx.x; p < P; p += NT)
            pool_entry(b, q, g, k, p, tb.topv, tb.topi, tb.slot_score, tb.flag_shared, tb.flag_local, tb.V, tb.tot, a.lambda, chosen, nc,
                       pm + p, pk + p, pt + p, pf + p);
        __syncthreads();
        for (int p = threadIdx.x; p < P; p += NT) {
            const int r = rank_of(pk, P, p);
            if (r < m) order[r] = p;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int64_t N = (int64_t)tb.B * k;
            int n = nc;
            go |= place(q, g, k, tb.min_t, tb.max_t, order, m, pm, pt, pf, t, tb.state, tb.bp_parent + t * N, tb.bp_token + t * N,
                        tb.slot_score, tb.comp_step, tb.comp_parent, tb.comp_score, chosen, &n);
            n_chosen = n;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && go) atomicOr(tb.active + active_set(t), 1);
}

}  // namespace

extern "C" int gtos_diverse_advance(int B, int k, int groups, uint64_t diversity_bits, int t, int V, int tot, int min_time_step,
                                    int max_time_step, const float* topv, const int* topi, const uint8_t* flag_shared,
                                    const uint8_t* flag_local, double* slot_score, int* group_state, int* bp_parent, int* bp_token,
                                    int* comp_step, int* comp_parent, double* comp_score, int* active, void* stream) {
    if (B <= 0) return 0;
    double lambda;
    static_assert(sizeof lambda == sizeof diversity_bits, "the penalty travels as the bit pattern of an fp64");
    memcpy(&lambda, &diversity_bits, sizeof lambda);
    const DiverseArgs a{{B, k, t, V, tot, min_time_step, max_time_step, topv, topi, flag_shared, flag_local, slot_score, group_state,
                         bp_parent, bp_token, comp_step, comp_parent, comp_score, active}, groups, lambda};
    if (!sizes_ok(a.tb) || groups < 1 || k % groups || !lambda_ok(lambda)) return -10;
    if (!tables_ok(a.tb)) return -23;
    hipLaunchKernelGGL(diverse_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_diverse_reorder(int n_caches, void* const* src, void* const* dst, int64_t row_bytes, int N, int k, int g, int t,
                                    int max_time_step, const int* bp_parent, const int* bp_token, const int* group_state,
                                    const int* active, int V, int tot, const int64_t* tok_shared, const int64_t* tok_local,
                                    const int64_t* char_shared, const int64_t* char_local, int C, int64_t dead_tok,
                                    const int64_t* dead_char, int64_t* tok_out, int64_t* char_out, void* stream) {
    return reorder_launch(n_caches, src, dst, row_bytes, N, k, g, t, max_time_step, bp_parent, bp_token, group_state, active, V, tot,
                          NextInput{tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char, C, tok_out, char_out}, stream);
}
