// Device-resident beam search (gtos_amd.search.beam_search_device): top-k of the log-likelihood rows, the beams' advance (selection
// rule in csrc/beam_kernels.h, shared with the host check), and the reorder of the self-attention caches by parent slot together with
// the next step's input token ids and character rows.  Nothing here synchronises with the host; the per-beam state, back-pointers and
// completions stay on the device until the search ends.
#include "beam_kernels.h"
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

struct AdvanceArgs {
    int B, k, t, V, tot, min_t, max_t;
    const float* topv;
    const int* topi;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    double* slot_score;
    int* state;
    int* bp_parent;
    int* bp_token;
    int* comp_step;
    int* comp_parent;
    double* comp_score;
    int* active;
};

// One workgroup per beam.  The active[3] rotation of csrc/slot_kernels.h; the flag: did any not-done beam have a live slot when this
// iteration started?
__global__ __launch_bounds__(NT) void beam_advance_kernel(AdvanceArgs a) {
    __shared__ double ps[MAX_K * MAX_K];
    __shared__ int pt[MAX_K * MAX_K];
    __shared__ uint8_t pf[MAX_K * MAX_K];
    __shared__ int order[MAX_K];
    const int b = blockIdx.x, t = a.t;
    if (b == 0 && threadIdx.x == 0) a.active[active_clear(t)] = 0;
    const int* st = a.state + (int64_t)b * BS_WORDS;
    if (!a.active[active_read(t)] || st[BS_DONE]) return;
    const int P = st[BS_NLIVE] * a.k;
    const int m = cut_size(P, a.k, st[BS_NCOMP]);
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

constexpr int MAX_CACHES = 32;

struct ReorderArgs {
    int n, N, k, t, V, tot;
    int64_t q;                          // 16-byte pieces per cache row
    const uint4* src[MAX_CACHES];
    uint4* dst[MAX_CACHES];
    const int* bp_parent_t;             // row t of the back-pointer tables
    const int* bp_token_t;
    const int* state;
    const int* active_t;                // the flag step t's advance read
    NextInput next;
};

__device__ __forceinline__ bool slot_live(const ReorderArgs& a, int s) {
    return a.bp_parent_t[s] >= 0 && !a.state[(int64_t)(s / a.k) * BS_WORDS + BS_DONE];
}

// blockIdx.y < n: cache y, rows [0, t] gathered by parent slot into the other buffer of its pair (dead slots: zero rows);
// blockIdx.y == n: the next step's input token id and character row of every slot (dead slots: the padding input).
// After an iteration that did not run, the caches are left as they are and every slot gets the padding input.
__global__ __launch_bounds__(NT) void beam_reorder_kernel(ReorderArgs a) {
    const bool act = *a.active_t != 0;
    const int64_t stride = (int64_t)gridDim.x * NT;
    if ((int)blockIdx.y == a.n) {
        const int C1 = a.next.C + 1;
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < (int64_t)a.N * C1; e += stride) {
            const int s = (int)(e / C1);
            write_next_input(a.next, a.V, a.tot, s / a.k, s, (int)(e % C1) - 1, act && slot_live(a, s) ? a.bp_token_t[s] : -1);
        }
        return;
    }
    if (!act) return;
    const uint4* src = a.src[blockIdx.y];
    uint4* dst = a.dst[blockIdx.y];
    const int64_t total = (int64_t)(a.t + 1) * a.N * a.q;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += stride) {
        const int64_t rowi = e / a.q, c = e % a.q;
        const int s = (int)(rowi % a.N);
        const int64_t r = rowi / a.N;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (slot_live(a, s)) v = src[(r * a.N + a.bp_parent_t[s]) * a.q + c];
        dst[e] = v;
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
    if (k < 1 || k > MAX_K || t < 0 || t >= max_time_step || V < 1 || tot < V) return -10;
    if (!topv || !topi || !flag_shared || (tot > V && !flag_local) || !slot_score || !beam_state || !bp_parent || !bp_token ||
        !comp_step || !comp_parent || !comp_score || !active)
        return -23;
    AdvanceArgs a{};
    a.B = B; a.k = k; a.t = t; a.V = V; a.tot = tot; a.min_t = min_time_step; a.max_t = max_time_step;
    a.topv = topv; a.topi = topi; a.flag_shared = flag_shared; a.flag_local = flag_local; a.slot_score = slot_score;
    a.state = beam_state; a.bp_parent = bp_parent; a.bp_token = bp_token; a.comp_step = comp_step; a.comp_parent = comp_parent;
    a.comp_score = comp_score; a.active = active;
    hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_beam_reorder(int n_caches, void* const* src, void* const* dst, int64_t row_bytes, int N, int k, int t,
                                 int max_time_step, const int* bp_parent, const int* bp_token, const int* beam_state,
                                 const int* active, int V, int tot, const int64_t* tok_shared, const int64_t* tok_local,
                                 const int64_t* char_shared, const int64_t* char_local, int C, int64_t dead_tok,
                                 const int64_t* dead_char, int64_t* tok_out, int64_t* char_out, void* stream) {
    if (N <= 0) return 0;
    if (n_caches < 0 || n_caches > MAX_CACHES || row_bytes <= 0 || row_bytes % 16 || k < 1 || k > MAX_K || N % k || t < 0 ||
        t >= max_time_step || V < 1 || tot < V || C < 1)
        return -10;
    ReorderArgs a{};
    a.next = NextInput{tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char, C, tok_out, char_out};
    if ((n_caches && (!src || !dst)) || !bp_parent || !bp_token || !beam_state || !active || !next_input_ok(a.next, V, tot)) return -23;
    a.n = n_caches; a.N = N; a.k = k; a.t = t; a.V = V; a.tot = tot; a.q = row_bytes / 16;
    for (int i = 0; i < n_caches; ++i) {
        if (!src[i] || !dst[i] || (uintptr_t)src[i] % 16 || (uintptr_t)dst[i] % 16 || src[i] == dst[i]) return -25;
        a.src[i] = static_cast<const uint4*>(src[i]);
        a.dst[i] = static_cast<uint4*>(dst[i]);
    }
    a.bp_parent_t = bp_parent + (int64_t)t * N; a.bp_token_t = bp_token + (int64_t)t * N; a.state = beam_state;
    a.active_t = active + active_read(t);
    const int64_t work = (int64_t)(t + 1) * N * a.q;
    const int64_t blocks = (work + NT - 1) / NT;
    const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(gx, (unsigned)n_caches + 1), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
