// Coverage-penalised beam search on the device (gtos_amd.search.beam_search_device with coverage; the host search and
// Generator.coverage launch the first kernel too): the per-slot coverage of the graph nodes with its penalty, and the beams' advance
// ranked by score + beta * penalty (rule in csrc/coverage_kernels.h, shared with the host check).  The top-k pass is gtos_beam_topk,
// the reorder gtos_beam_reorder; nothing here synchronises with the host.
#include "beam_device.h"
#include "common.h"
#include "coverage_kernels.h"
#include "slot_device.h"

#include <string.h>

using namespace gtos_coverage;

namespace {

static_assert(CP_LANES == NT, "one partial sum of a penalty per thread");

struct StepArgs {
    int N, n;
    const float* align;                 // [N, n]
    const uint8_t* pad;                 // [n, N]
    const int* parent;                  // [N] or null: a slot is its own parent
    const float* cov_prev;              // [N, n]
    float* cov_cur;                     // [N, n]
    double* cp;                         // [N]
    const int* active_t;                // the flag step t's kernels read
};

// One workgroup per slot: the parent's row gathered and added to (a strided loop over the nodes, any n) and the penalty -- thread l
// sums the terms of the nodes l, l + NT, ... it stores, the partial sums are folded by halving in LDS.
__global__ __launch_bounds__(NT) void coverage_step_kernel(StepArgs a) {
    __shared__ double part[NT];
    if (!*a.active_t) return;
    const int s = blockIdx.x, l = threadIdx.x;
    const int p = a.parent ? a.parent[s] : s;
    float* dst = a.cov_cur + (int64_t)s * a.n;
    if (p < 0 || p >= a.N) {            // a dead slot
        for (int i = l; i < a.n; i += NT) dst[i] = 0.0f;
        if (l == 0) a.cp[s] = 0.0;
        return;
    }
    const float* src = a.cov_prev + (int64_t)p * a.n;
    const float* al = a.align + (int64_t)s * a.n;
    const uint8_t* pad_s = a.pad + s;
    double acc = 0.0;
    for (int i = l; i < a.n; i += NT) {
        const float c = src[i] + al[i];
        dst[i] = c;
        if (!pad_s[(int64_t)i * a.N]) acc += (double)cp_term(c);
    }
    part[l] = acc;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (l < o) part[l] += part[l + o];
        __syncthreads();
    }
    if (l == 0) a.cp[s] = part[0];
}

struct AdvanceArgs {
    BeamTables tb;
    int n;
    double beta;
    const double* cp;
    const float* cov_cur;
    double* slot_cp;
    double* comp_cp;
    float* comp_cov;
    float* slot_cov;
};

// One workgroup per beam, as beam_advance_kernel: the pool and its keys filled and ranked by all threads, the cut placed by one, which
// leaves in LDS which rows of cov_cur the workgroup then copies: those of the parents of this step's completions into comp_cov (at the
// completions' indices) and those of the survivors' parents into slot_cov (at the survivors' slots).
__global__ __launch_bounds__(NT) void coverage_advance_kernel(AdvanceArgs a) {
    __shared__ double ps[MAX_K * MAX_K];     // model score
    __shared__ double pk[MAX_K * MAX_K];     // selection key
    __shared__ int pt[MAX_K * MAX_K];
    __shared__ uint8_t pf[MAX_K * MAX_K];
    __shared__ int order[MAX_K];
    __shared__ int row_src[2 * MAX_K];       // slot whose cov_cur row is copied ...
    __shared__ int row_dst[2 * MAX_K];       // ... to row r of comp_cov (r < N) or row r - N of slot_cov
    __shared__ int n_rows;
    const BeamTables& tb = a.tb;
    const int b = blockIdx.x, t = tb.t, k = tb.k;
    if (b == 0 && threadIdx.x == 0) tb.active[active_clear(t)] = 0;
    const int* st = tb.state + (int64_t)b * BS_WORDS;
    if (!tb.active[active_read(t)] || st[BS_DONE]) return;
    const int nlive0 = st[BS_NLIVE], ncomp0 = st[BS_NCOMP];
    if (!words_in_range(nlive0, ncomp0, k)) return;
    const int P = nlive0 * k;
    const int m = cut_size(P, k, ncomp0);
    const int64_t N = (int64_t)tb.B * k;
    for (int p = threadIdx.x; p < P; p += NT) {
        pool_entry(b, k, p, tb.topv, tb.topi, tb.slot_score, tb.flag_shared, tb.flag_local, tb.V, tb.tot, ps + p, pt + p, pf + p);
        pk[p] = key_of(ps[p], a.beta, a.cp[b * k + p / k]);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        const int r = rank_of(pk, P, p);
        if (r < m) order[r] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int* bp_parent_t = tb.bp_parent + t * N;
        if (place(b, k, tb.min_t, tb.max_t, order, m, ps, pt, pf, t, tb.state, bp_parent_t, tb.bp_token + t * N, tb.slot_score,
                  tb.comp_step, tb.comp_parent, tb.comp_score, a.cp, a.slot_cp, a.comp_cp))
            atomicOr(tb.active + active_set(t), 1);
        const int* st1 = tb.state + (int64_t)b * BS_WORDS;
        int nr = 0;
        for (int j = ncomp0; j < st1[BS_NCOMP] && j < k; ++j) {
            row_src[nr] = tb.comp_parent[b * k + j];
            row_dst[nr++] = b * k + j;
        }
        for (int j = 0; j < st1[BS_NLIVE] && j < k; ++j) {
            row_src[nr] = bp_parent_t[b * k + j];
            row_dst[nr++] = (int)N + b * k + j;
        }
        n_rows = nr;
    }
    __syncthreads();
    for (int r = 0; r < n_rows; ++r) {
        const int src = row_src[r], dst = row_dst[r];
        if (src < 0 || src >= N) continue;
        const float* from = a.cov_cur + (int64_t)src * a.n;
        float* to = dst < N ? a.comp_cov + (int64_t)dst * a.n : a.slot_cov + (int64_t)(dst - N) * a.n;
        for (int i = threadIdx.x; i < a.n; i += NT) to[i] = from[i];
    }
}

}  // namespace

extern "C" int gtos_coverage_step(int N, int k, int t, int n, const float* align, const uint8_t* pad, const int* parent,
                                  const float* cov_prev, float* cov_cur, double* cp, const int* active, void* stream) {
    if (N <= 0) return 0;
    if (k < 1 || N % k || t < 0 || n < 1) return -10;
    if (!align || !pad || !cov_prev || !cov_cur || !cp || !active) return -23;
    if (cov_prev == cov_cur) return -10;            // a slot reads its parent's row while the parent's owner rewrites its own
    StepArgs a{};
    a.N = N; a.n = n; a.align = align; a.pad = pad; a.parent = parent; a.cov_prev = cov_prev; a.cov_cur = cov_cur; a.cp = cp;
    a.active_t = active + active_read(t);
    hipLaunchKernelGGL(coverage_step_kernel, dim3((unsigned)N), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_coverage_advance(int B, int k, int t, int V, int tot, int min_time_step, int max_time_step, uint64_t beta_bits,
                                     int n, const float* topv, const int* topi, const uint8_t* flag_shared, const uint8_t* flag_local,
                                     double* slot_score, int* beam_state, int* bp_parent, int* bp_token, int* comp_step,
                                     int* comp_parent, double* comp_score, const double* cp, const float* cov_cur, double* slot_cp,
                                     double* comp_cp, float* comp_cov, float* slot_cov, int* active, void* stream) {
    if (B <= 0) return 0;
    double beta;
    static_assert(sizeof beta == sizeof beta_bits, "the penalty weight travels as the bit pattern of an fp64");
    memcpy(&beta, &beta_bits, sizeof beta);
    const AdvanceArgs a{{B, k, t, V, tot, min_time_step, max_time_step, topv, topi, flag_shared, flag_local, slot_score, beam_state,
                         bp_parent, bp_token, comp_step, comp_parent, comp_score, active},
                        n, beta, cp, cov_cur, slot_cp, comp_cp, comp_cov, slot_cov};
    if (!sizes_ok(a.tb) || n < 1 || !beta_ok(beta)) return -10;
    if ((int64_t)B * k * 2 > INT_MAX) return -10;
    if (!tables_ok(a.tb) || !cp || !cov_cur || !slot_cp || !comp_cp || !comp_cov || !slot_cov) return -23;
    hipLaunchKernelGGL(coverage_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
