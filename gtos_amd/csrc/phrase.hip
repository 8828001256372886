// Phrase-constrained beam search on the device (gtos_amd.search.beam_search_device with phrases): the advance of every beam by the rule
// of csrc/phrase_kernels.h (shared with the host check).  The top-k pass and the reorder are gtos_beam_topk / gtos_beam_reorder; nothing
// here synchronises with the host.
#include "beam_device.h"
#include "phrase_kernels.h"
#include "slot_device.h"

using namespace gtos_phrase;

namespace {

struct PhraseArgs {
    BeamTables tb;
    int Cw, Lw;
    const float* ll;
    int64_t ld;
    const int* phr;
    int* pst;
};

// One workgroup per beam, laid out as constrain_advance_kernel (csrc/constrain.hip): the pool (at most MAX_POOL = 32 x 48 entries, 35 KB
// of LDS with its next states, banks and ranks) is filled by all threads, strided; the rank within the bank and then the final position
// are two O(P^2) counting passes, each behind a barrier -- the second only for entries whose q is below the cut, since an entry's final
// position is never below its q; the cut is placed by one thread.  Before the pool, one thread reads the graph's phrase lengths into
// LDS (at most 16 x 16 ids); the entries then read single ids of phr.  The active[3] rotation of csrc/slot_kernels.h.
__global__ __launch_bounds__(NT) void phrase_advance_kernel(PhraseArgs a) {
    __shared__ double ps[MAX_POOL];
    __shared__ int pt[MAX_POOL];
    __shared__ int pn[MAX_POOL];         // packed next state
    __shared__ int pq[MAX_POOL];         // rank within the bank
    __shared__ uint8_t pf[MAX_POOL];
    __shared__ signed char pb[MAX_POOL]; // bank (at most MAX_TOKENS), -1: absent
    __shared__ int order[MAX_K];
    __shared__ int present;
    __shared__ PhraseSet set;
    const BeamTables& tb = a.tb;
    const int b = blockIdx.x, t = tb.t, k = tb.k;
    if (b == 0 && threadIdx.x == 0) tb.active[active_clear(t)] = 0;
    const int* st = tb.state + (int64_t)b * BS_WORDS;
    if (!tb.active[active_read(t)] || st[BS_DONE]) return;
    const int nlive = st[BS_NLIVE], ncomp = st[BS_NCOMP];
    if (!words_in_range(nlive, ncomp, k)) return;
    const int64_t N = (int64_t)tb.B * k;
    const int* pst_t = a.pst + (t % 2) * N;
    const int W = k + a.Cw, P = nlive * W;
    if (threadIdx.x == 0) {
        present = 0;
        load_phrases(&set, a.Cw ? a.phr + (int64_t)b * a.Cw * a.Lw : nullptr, a.Cw, a.Lw, tb.tot);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        const bool here = pool_entry(b, k, a.Cw, p, tb.topv, tb.topi, a.ll, a.ld, set, tb.slot_score, pst_t, tb.flag_shared,
                                     tb.flag_local, tb.V, tb.tot, ps + p, pt + p, pf + p, pn + p);
        pb[p] = here ? (signed char)bank_of_state(set, pn[p]) : (signed char)-1;
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
        if (place(b, k, W, tb.min_t, tb.max_t, order, m, ps, pt, pf, pn, t, tb.state, tb.bp_parent + t * N, tb.bp_token + t * N,
                  tb.slot_score, tb.comp_step, tb.comp_parent, tb.comp_score, a.pst + ((t + 1) % 2) * N))
            atomicOr(tb.active + active_set(t), 1);
    }
}

}  // namespace

extern "C" int gtos_phrase_advance(int B, int k, int Cw, int Lw, int t, int V, int tot, int min_time_step, int max_time_step,
                                   const float* topv, const int* topi, const float* ll, int64_t ld, const int* phr,
                                   const uint8_t* flag_shared, const uint8_t* flag_local, double* slot_score, int* beam_state,
                                   int* bp_parent, int* bp_token, int* comp_step, int* comp_parent, double* comp_score, int* pst,
                                   int* active, void* stream) {
    if (B <= 0) return 0;
    const PhraseArgs a{{B, k, t, V, tot, min_time_step, max_time_step, topv, topi, flag_shared, flag_local, slot_score, beam_state,
                        bp_parent, bp_token, comp_step, comp_parent, comp_score, active}, Cw, Lw, ll, ld, phr, pst};
    if (!sizes_ok(a.tb) || Cw < 0 || Cw > MAX_PHR || Lw < 0 || Lw > MAX_LEN || (Cw > 0 && Lw < 1) || ld < tot) return -10;
    if (!tables_ok(a.tb) || !ll || (Cw > 0 && !phr) || !pst) return -23;
    hipLaunchKernelGGL(phrase_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
