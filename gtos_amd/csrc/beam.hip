// Device-resident beam search (gtos_amd.search.beam_search_device): top-k of the log-likelihood rows, the beams' advance (selection
// rule in csrc/beam_kernels.h, shared with the host check), and the reorder of the self-attention caches by parent slot together with
// the next step's input token ids and character rows.  Nothing here synchronises with the host; the per-beam state, back-pointers and
// completions stay on the device until the search ends.
#include "common.h"
#include "beam_kernels.h"

#include <limits.h>

using namespace gtos_beam;

namespace {

constexpr int NT = 256;                 // 4 waves

// (value, index) a goes before b: larger value first, equal values lower index first
__device__ __forceinline__ bool tk_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// One workgroup per row.  Every lane keeps its KM best (value, column) in registers, sorted, scanning columns lane, lane + NT, ...;
// each wave then pops its k best by k butterfly arg-max rounds over the lanes' heads, and the 4 x k wave winners are ranked in LDS.
template <int KM>
__global__ __launch_bounds__(NT) void beam_topk_kernel(int tot, int k, const float* __restrict__ ll, int64_t ld,
                                                       float* __restrict__ val, int* __restrict__ idx) {
    __shared__ float sv[NT / 64][MAX_K];
    __shared__ int si[NT / 64][MAX_K];
    const int row = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* x = ll + (int64_t)row * ld;
    float v[KM];
    int ix[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) { v[j] = -__builtin_inff(); ix[j] = INT_MAX; }
    for (int c = threadIdx.x; c < tot; c += NT) {
        const float y = x[c];
        if (tk_before(y, c, v[KM - 1], ix[KM - 1])) {
            v[KM - 1] = y; ix[KM - 1] = c;
#pragma unroll
            for (int j = KM - 1; j > 0; --j) {
                if (tk_before(v[j], ix[j], v[j - 1], ix[j - 1])) {
                    const float tv = v[j]; v[j] = v[j - 1]; v[j - 1] = tv;
                    const int ti = ix[j]; ix[j] = ix[j - 1]; ix[j - 1] = ti;
                }
            }
        }
    }
    for (int r = 0; r < k; ++r) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (tk_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (ix[0] == bi) {             // the winning lane pops its head (columns are unique; an all-sentinel wave pops sentinels)
#pragma unroll
            for (int j = 0; j < KM - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
            v[KM - 1] = -__builtin_inff(); ix[KM - 1] = INT_MAX;
        }
        if (lane == 0) { sv[w][r] = bv; si[w][r] = bi; }
    }
    __syncthreads();
    const int n = (NT / 64) * k;
    if (threadIdx.x < n) {
        const int wi = threadIdx.x / k, ri = threadIdx.x % k;
        const float a = sv[wi][ri];
        const int ai = si[wi][ri];
        int rank = 0;
        for (int q = 0; q < n; ++q) rank += tk_before(sv[q / k][q % k], si[q / k][q % k], a, ai);
        if (rank < k && ai != INT_MAX) {
            val[(int64_t)row * k + rank] = a;
            idx[(int64_t)row * k + rank] = ai;
        }
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

// One workgroup per beam.  active[3] rotates: step t reads active[t % 3] (did any not-done beam have a live slot when this iteration
// started?), ORs its own answer into active[(t + 1) % 3] and clears active[(t + 2) % 3] for step t + 1.  An iteration that does
// not run (search.py's loop would have stopped) changes nothing, and the flag stays 0 from then on.
__global__ __launch_bounds__(NT) void beam_advance_kernel(AdvanceArgs a) {
    __shared__ double ps[MAX_K * MAX_K];
    __shared__ int pt[MAX_K * MAX_K];
    __shared__ uint8_t pf[MAX_K * MAX_K];
    __shared__ int order[MAX_K];
    const int b = blockIdx.x, t = a.t;
    if (b == 0 && threadIdx.x == 0) a.active[(t + 2) % 3] = 0;
    const int* st = a.state + (int64_t)b * BS_WORDS;
    if (!a.active[t % 3] || st[BS_DONE]) return;
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
            atomicOr(a.active + (t + 1) % 3, 1);
    }
}

constexpr int MAX_CACHES = 32;

struct ReorderArgs {
    int n, N, k, t, V, tot, C;
    int64_t q;                          // 16-byte pieces per cache row
    const uint4* src[MAX_CACHES];
    uint4* dst[MAX_CACHES];
    const int* bp_parent_t;             // row t of the back-pointer tables
    const int* bp_token_t;
    const int* state;
    const int* active_t;                // the flag step t's advance read
    const int64_t* tok_shared;
    const int64_t* tok_local;
    const int64_t* char_shared;
    const int64_t* char_local;
    int64_t dead_tok;
    const int64_t* dead_char;
    int64_t* tok_out;
    int64_t* char_out;
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
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < (int64_t)a.N * (a.C + 1); e += stride) {
            const int s = (int)(e / (a.C + 1)), c = (int)(e % (a.C + 1)) - 1;      // c == -1: the token id
            int64_t out;
            if (act && slot_live(a, s)) {
                const int id = a.bp_token_t[s];
                const int64_t lid = (int64_t)(s / a.k) * (a.tot - a.V) + (id - a.V);
                if (c < 0) out = id < a.V ? a.tok_shared[id] : a.tok_local[lid];
                else out = id < a.V ? a.char_shared[(int64_t)id * a.C + c] : a.char_local[lid * a.C + c];
            } else {
                out = c < 0 ? a.dead_tok : a.dead_char[c];
            }
            if (c < 0) a.tok_out[s] = out;
            else a.char_out[(int64_t)s * a.C + c] = out;
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
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 g((unsigned)rows), blk(NT);
    if (k <= 4) hipLaunchKernelGGL(beam_topk_kernel<4>, g, blk, 0, s, tot, k, ll, ld, val, idx);
    else if (k <= 8) hipLaunchKernelGGL(beam_topk_kernel<8>, g, blk, 0, s, tot, k, ll, ld, val, idx);
    else if (k <= 16) hipLaunchKernelGGL(beam_topk_kernel<16>, g, blk, 0, s, tot, k, ll, ld, val, idx);
    else hipLaunchKernelGGL(beam_topk_kernel<32>, g, blk, 0, s, tot, k, ll, ld, val, idx);
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
    if ((n_caches && (!src || !dst)) || !bp_parent || !bp_token || !beam_state || !active || !tok_shared || !char_shared ||
        (tot > V && (!tok_local || !char_local)) || !dead_char || !tok_out || !char_out)
        return -23;
    ReorderArgs a{};
    a.n = n_caches; a.N = N; a.k = k; a.t = t; a.V = V; a.tot = tot; a.C = C; a.q = row_bytes / 16;
    for (int i = 0; i < n_caches; ++i) {
        if (!src[i] || !dst[i] || (uintptr_t)src[i] % 16 || (uintptr_t)dst[i] % 16 || src[i] == dst[i]) return -25;
        a.src[i] = static_cast<const uint4*>(src[i]);
        a.dst[i] = static_cast<uint4*>(dst[i]);
    }
    a.bp_parent_t = bp_parent + (int64_t)t * N; a.bp_token_t = bp_token + (int64_t)t * N; a.state = beam_state;
    a.active_t = active + t % 3;
    a.tok_shared = tok_shared; a.tok_local = tok_local; a.char_shared = char_shared; a.char_local = char_local;
    a.dead_tok = dead_tok; a.dead_char = dead_char; a.tok_out = tok_out; a.char_out = char_out;
    const int64_t work = (int64_t)(t + 1) * N * a.q;
    const int64_t blocks = (work + NT - 1) / NT;
    const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(gx, (unsigned)n_caches + 1), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
