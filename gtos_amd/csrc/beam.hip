// Device-resident beam search (gtos_amd.search.beam_search_device): top-k of the log-likelihood rows, the beams' advance (selection
// rule in csrc/beam_kernels.h, shared with the host check), and the reorder of the self-attention caches by parent slot together with
// the next step's input token ids and character rows.  Nothing here synchronises with the host; the per-beam state, back-pointers and
// completions stay on the device until the search ends.
#include "beam_device.h"
#include "beam_kernels.h"
#include "reorder_device.h"
#include "slot_device.h"

using namespace gtos_beam;

namespace {

static_assert(MAX_K <= TOPK_MAX, "beam_topk_kernel ranks its rows with row_topk");

// One workgroup per row: row_topk over every column, the sorted list stored
template <int KM>
__global__ __launch_bounds__(NT) void beam_topk_kernel(int tot, int k, const float* __restrict__ ll, int64_t ld,
                                                       float* __restrict__ val, int* __restrict__ idx) {
    __shared__ float lv[MAX_K];
    __shared__ int lc[MAX_K];
    const int row = blockIdx.x;
    row_topk<KM>(ll + (int64_t)row * ld, tot, k, [](int, float) { return true; }, lv, lc);
    if (threadIdx.x < k && lc[threadIdx.x] != INT_MAX) {
        val[(int64_t)row * k + threadIdx.x] = lv[threadIdx.x];
        idx[(int64_t)row * k + threadIdx.x] = lc[threadIdx.x];
    }
}

// One workgroup per beam.  The active[3] rotation of csrc/slot_kernels.h; the flag: did any not-done beam have a live slot when this
// iteration started?
__global__ __launch_bounds__(NT) void beam_advance_kernel(BeamTables a) {
    __shared__ double ps[MAX_K * MAX_K];
    __shared__ int pt[MAX_K * MAX_K];
    __shared__ uint8_t pf[MAX_K * MAX_K];
    __shared__ int order[MAX_K];
    const int b = blockIdx.x, t = a.t;
    if (b == 0 && threadIdx.x == 0) a.active[active_clear(t)] = 0;
    const int* st = a.state + (int64_t)b * BS_WORDS;
    if (!a.active[active_read(t)] || st[BS_DONE]) return;
    const int nlive = st[BS_NLIVE], ncomp = st[BS_NCOMP];
    if (!words_in_range(nlive, ncomp, a.k)) return;
    const int P = nlive * a.k;
    const int m = cut_size(P, a.k, ncomp);
    for (int p = threadIdx.x; p < P; p += NT)
        pool_entry(b, a.k, p, a.topv, a.topi, a.slot_score, a.flag_shared, a.flag_local, a.V, a.tot, ps + p, pt + p, pf + p);
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        const int r = rank_of(ps, P, p);
        if (r < m) order[r] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t N = (int64_t)a.B * a.k;
        if (place(b, a.k, a.min_t, a.max_t, order, m, ps, pt, pf, t, a.state, a.bp_parent + t * N, a.bp_token + t * N, a.slot_score,
                  a.comp_step, a.comp_parent, a.comp_score))
            atomicOr(a.active + active_set(t), 1);
    }
}

}  // namespace

extern "C" int gtos_beam_topk(int rows, int tot, int k, const float* ll, int64_t ld, float* val, int* idx, void* stream) {
    if (rows <= 0) return 0;
    if (k < 1 || k > MAX_K || tot < k || ld < tot) return -10;
    if (!ll || !val || !idx) return -23;
    dispatch_km(k, [&](auto km) {
        hipLaunchKernelGGL(beam_topk_kernel<decltype(km)::value>, dim3((unsigned)rows), dim3(NT), 0, static_cast<hipStream_t>(stream),
                           tot, k, ll, ld, val, idx);
    });
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_beam_advance(int B, int k, int t, int V, int tot, int min_time_step, int max_time_step, const float* topv,
                                 const int* topi, const uint8_t* flag_shared, const uint8_t* flag_local, double* slot_score,
                                 int* beam_state, int* bp_parent, int* bp_token, int* comp_step, int* comp_parent,
                                 double* comp_score, int* active, void* stream) {
    if (B <= 0) return 0;
    const BeamTables a{B, k, t, V, tot, min_time_step, max_time_step, topv, topi, flag_shared, flag_local, slot_score, beam_state,
                       bp_parent, bp_token, comp_step, comp_parent, comp_score, active};
    if (!sizes_ok(a)) return -10;
    if (!tables_ok(a)) return -23;
    hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_beam_reorder(int n_caches, void* const* src, void* const* dst, int64_t row_bytes, int N, int k, int t,
                                 int max_time_step, const int* bp_parent, const int* bp_token, const int* beam_state,
                                 const int* active, int V, int tot, const int64_t* tok_shared, const int64_t* tok_local,
                                 const int64_t* char_shared, const int64_t* char_local, int C, int64_t dead_tok,
                                 const int64_t* dead_char, int64_t* tok_out, int64_t* char_out, void* stream) {
    return reorder_launch(n_caches, src, dst, row_bytes, N, k, k, t, max_time_step, bp_parent, bp_token, beam_state, active, V, tot,
                          NextInput{tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char, C, tok_out, char_out}, stream);
}
