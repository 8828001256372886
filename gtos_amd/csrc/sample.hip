// Device-resident sampling decode (gtos_amd.search.sample_device): one step of every sample slot, selection rule in
// csrc/sample_kernels.h (shared with the host check).  One workgroup per slot row: a register top-k pass (top_k > 0) or a max / min
// pass, a threshold bisection for top-p with fp64 block sums over the row, a Gumbel arg-max, then the slot's bookkeeping and its next
// input.  Rows are read from global memory as often as the passes need (they stay in L2 / MALL); nothing is staged in LDS but the
// partial results.  Nothing here synchronises with the host.
#include "sample_kernels.h"
#include "slot_device.h"

using namespace gtos_sample;

namespace {

static_assert(MAX_TOPK <= TOPK_MAX, "select_topk ranks its row with row_topk");

struct SampleArgs {
    int N, k, t, V, tot, min_t, max_t, top_k;
    double T, top_p;
    uint64_t seed;
    const float* ll;
    int64_t ld;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    const uint8_t* owned_local;
    double* score;
    int* state;
    int* tokens;
    int* active;
    NextInput next;
};

__device__ __forceinline__ bool col_allowed(const SampleArgs& a, int b, int c, float y) {
    return allowed(a.flag_shared, a.flag_local, a.owned_local, a.V, a.tot, b, c, a.t, a.min_t, y);
}

// arg-max of (key, column) by wins(); the winner's column goes to every thread
__device__ int block_argmax(double bk, int bc, double* rk, int* rc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ok = __shfl_xor(bk, o);
        const int oc = __shfl_xor(bc, o);
        if (wins(ok, oc, bk, bc)) { bk = ok; bc = oc; }
    }
    if ((threadIdx.x & 63) == 0) { rk[threadIdx.x >> 6] = bk; rc[threadIdx.x >> 6] = bc; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w)
        if (wins(rk[w], rc[w], bk, bc)) { bk = rk[w]; bc = rc[w]; }
    __syncthreads();
    return bc;
}

// Rules 2-4 with top_k > 0: row_topk over the allowed columns, then one wave draws among the top-p survivors of the sorted list.
template <int KM>
__device__ int select_topk(const SampleArgs& a, const float* x, int b, uint64_t key) {
    __shared__ float lv[MAX_TOPK];
    __shared__ int lc[MAX_TOPK];
    __shared__ int s_n;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, k = a.top_k;
    row_topk<KM>(x, a.tot, k, [&](int c, float y) { return col_allowed(a, b, c, y); }, lv, lc);
    if (threadIdx.x == 0) {
        int m = 0;
        while (m < k && lc[m] != INT_MAX) ++m;
        s_n = topp_keep_sorted(lv, m, a.T, a.top_p);
    }
    __syncthreads();
    int bc = INT_MAX;
    if (w == 0) {
        double bk = -INFINITY;
        if (lane < s_n) { bk = draw_key(lv[lane], a.T, key, lc[lane]); bc = lc[lane]; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ok = __shfl_xor(bk, o);
            const int oc = __shfl_xor(bc, o);
            if (wins(ok, oc, bk, bc)) { bk = ok; bc = oc; }
        }
    }
    return bc == INT_MAX ? -1 : bc;     // valid in wave 0 (thread 0 uses it)
}

// Rules 1, 3, 4 with top_k == 0 over the whole row
__device__ int select_row(const SampleArgs& a, const float* x, int b, uint64_t key) {
    __shared__ double rd[NW];
    __shared__ float rmx[NW], rmn[NW];
    __shared__ int rc[NW];
    float mx = -INFINITY, mn = INFINITY;
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (col_allowed(a, b, c, y)) { mx = fmaxf(mx, y); mn = fminf(mn, y); }
    }
    block_minmax(mx, mn, rmx, rmn);
    if (!(mx > -INFINITY)) return -1;
    float vstar = mn;
    if (a.top_p < 1.0) {
        double z = 0.0;
        for (int c = threadIdx.x; c < a.tot; c += NT) {
            const float y = x[c];
            if (col_allowed(a, b, c, y)) z += weight(y, mx, a.T);
        }
        const double Z = block_sum(z, rd);
        uint32_t klo = order_key(mn), khi = order_key(mx) + 1;
        while (khi - klo > 1) {
            const uint32_t mid = bisect_mid(klo, khi);
            const float v = order_value(mid);
            double s = 0.0;
            for (int c = threadIdx.x; c < a.tot; c += NT) {
                const float y = x[c];
                if (y >= v && col_allowed(a, b, c, y)) s += weight(y, mx, a.T);
            }
            if (block_sum(s, rd) >= a.top_p * Z) klo = mid;
            else khi = mid;
        }
        vstar = order_value(klo);
    }
    double bk = -INFINITY;
    int bc = INT_MAX;
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (y >= vstar && col_allowed(a, b, c, y)) {
            const double dk = draw_key(y, a.T, key, c);
            if (wins(dk, c, bk, bc)) { bk = dk; bc = c; }
        }
    }
    bc = block_argmax(bk, bc, rd, rc);
    return bc == INT_MAX ? -1 : bc;
}

// One workgroup per slot.  The active[3] rotation of csrc/slot_kernels.h; the flag: does some slot sample again?  Every slot, live
// or not, gets its next input (a dead slot the padding input).
template <int KM>
__global__ __launch_bounds__(NT) void sample_step_kernel(SampleArgs a) {
    __shared__ int s_run, s_next;
    const int s = blockIdx.x, b = s / a.k, j = s % a.k, t = a.t;
    if (threadIdx.x == 0) {
        if (s == 0) a.active[active_clear(t)] = 0;
        s_run = a.active[active_read(t)] && !a.state[(int64_t)s * SS_WORDS + SS_DEAD];
        s_next = -1;
    }
    __syncthreads();
    if (s_run) {
        const float* x = a.ll + (int64_t)s * a.ld;
        const uint64_t key = row_key(a.seed, b, j, t);
        const int w = a.top_k > 0 ? select_topk<KM>(a, x, b, key) : select_row(a, x, b, key);
        if (threadIdx.x == 0) {
            const uint8_t f = w < 0 ? (uint8_t)TOK_PLAIN : token_flag(a.flag_shared, a.flag_local, a.V, a.tot, b, w);
            const bool on = update(s, t, a.max_t, w, w < 0 ? 0.0f : x[w], f, a.score, a.state, a.tokens + (int64_t)t * a.N);
            if (on) {
                atomicOr(a.active + active_set(t), 1);
                s_next = w;
            }
        }
        __syncthreads();
    }
    const int id = s_next;
    for (int c = (int)threadIdx.x - 1; c < a.next.C; c += NT) write_next_input(a.next, a.V, a.tot, b, s, c, id);
}

}  // namespace

extern "C" int gtos_sample_step(int N, int k, int t, int V, int tot, int min_time_step, int max_time_step, float temperature, int top_k,
                                float top_p, uint64_t seed, const float* ll, int64_t ld, const uint8_t* flag_shared,
                                const uint8_t* flag_local, const uint8_t* owned_local, double* score, int* slot_state, int* tokens,
                                int* active, const int64_t* tok_shared, const int64_t* tok_local, const int64_t* char_shared,
                                const int64_t* char_local, int C, int64_t dead_tok, const int64_t* dead_char, int64_t* tok_out,
                                int64_t* char_out, void* stream) {
    if (N <= 0) return 0;
    if (k < 1 || N % k || t < 0 || t >= max_time_step || V < 1 || tot < V || ld < tot || C < 1 || top_k < 0 || top_k > MAX_TOPK ||
        !(temperature > 0.0f && temperature < INFINITY) || !(top_p > 0.0f && top_p <= 1.0f))
        return -10;
    SampleArgs a{};
    a.next = NextInput{tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char, C, tok_out, char_out};
    if (!ll || !flag_shared || (tot > V && (!flag_local || !owned_local)) || !score || !slot_state || !tokens || !active ||
        !next_input_ok(a.next, V, tot))
        return -23;
    a.N = N; a.k = k; a.t = t; a.V = V; a.tot = tot; a.min_t = min_time_step; a.max_t = max_time_step; a.top_k = top_k;
    a.T = (double)temperature; a.top_p = (double)top_p; a.seed = seed; a.ll = ll; a.ld = ld;
    a.flag_shared = flag_shared; a.flag_local = flag_local; a.owned_local = owned_local; a.score = score; a.state = slot_state;
    a.tokens = tokens; a.active = active;
    dispatch_km(top_k, [&](auto km) {
        hipLaunchKernelGGL(sample_step_kernel<decltype(km)::value>, dim3((unsigned)N), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    });
    GTOS_CHECK_LAUNCH();
    return 0;
}
