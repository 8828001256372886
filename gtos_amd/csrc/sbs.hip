// Stochastic beam search on the device (gtos_amd.search.stochastic_beam_search_device): one step of every live slot's row and the
// advance of every graph's pool, selection rule in csrc/sbs_kernels.h (shared with the host check).  The step ends with
// gtos_beam_reorder (csrc/beam.hip), which reads the tables written here as it reads gtos_beam_advance's.  The step kernel is
// sample_step_kernel's shape, one workgroup per slot row: a max pass, an fp64 sum for the row's normaliser, a key pass that keeps
// the k best by fp64 key, and the conditioning of those <= k candidates.  Rows are read from global memory once per pass (they stay in
// L2 / MALL); nothing is staged in LDS but the partial results.  Nothing here synchronises with the host.
#include "sbs_kernels.h"
#include "slot_device.h"

using namespace gtos_sbs;

namespace {

static_assert(MAX_K <= TOPK_MAX, "the key lists are sized like row_topk's");

struct StepArgs {
    int N, k, t, V, tot, min_t;
    double T;
    uint64_t seed;
    const float* ll;
    int64_t ld;
    const uint8_t* flag_shared;
    const uint8_t* flag_local;
    const uint8_t* owned_local;
    const double* slot_logq;
    const double* slot_gumbel;
    const int* state;
    const int* active;
    int* cand_tok;
    float* cand_ll;
    double* cand_logq;
    double* cand_gumbel;
};

// row_topk (csrc/slot_device.h) for fp64 keys: the k best (key, column) by wins() among the columns c of [0, tot) for which
// key_of(c, key) holds, by one workgroup of NT threads.  Every lane keeps its KM >= k best in registers, sorted; each wave pops its k
// best by k butterfly arg-max rounds; the NW x k wave winners are ranked by counting.  On return (a barrier) the sorted list is in
// the LDS arrays lk / lc [k]; with fewer than k columns the rest of lc holds INT_MAX.
template <int KM, class KeyOf>
__device__ void row_topk_keys(int tot, int k, KeyOf key_of, double* lk, int* lc) {
    __shared__ double sk[NW][TOPK_MAX];
    __shared__ int si[NW][TOPK_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double v[KM];
    int ix[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) { v[j] = -__builtin_inf(); ix[j] = INT_MAX; }
    for (int c = threadIdx.x; c < tot; c += NT) {
        double y;
        if (key_of(c, y) && wins(y, c, v[KM - 1], ix[KM - 1])) {
            v[KM - 1] = y; ix[KM - 1] = c;
#pragma unroll
            for (int j = KM - 1; j > 0; --j) {
                if (wins(v[j], ix[j], v[j - 1], ix[j - 1])) {
                    const double tv = v[j]; v[j] = v[j - 1]; v[j - 1] = tv;
                    const int ti = ix[j]; ix[j] = ix[j - 1]; ix[j - 1] = ti;
                }
            }
        }
    }
    for (int r = 0; r < k; ++r) {
        double bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (wins(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (ix[0] == bi) {              // the winning lane pops its head (columns are unique; an all-sentinel wave pops sentinels)
#pragma unroll
            for (int j = 0; j < KM - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
            v[KM - 1] = -__builtin_inf(); ix[KM - 1] = INT_MAX;
        }
        if (lane == 0) { sk[w][r] = bv; si[w][r] = bi; }
    }
    if (threadIdx.x < k) lc[threadIdx.x] = INT_MAX;
    __syncthreads();
    const int n = NW * k;
    if (threadIdx.x < n) {
        const double a = sk[threadIdx.x / k][threadIdx.x % k];
        const int ai = si[threadIdx.x / k][threadIdx.x % k];
        int rank = 0;
        for (int q = 0; q < n; ++q) rank += wins(sk[q / k][q % k], si[q / k][q % k], a, ai);
        if (rank < k && ai != INT_MAX) { lk[rank] = a; lc[rank] = ai; }
    }
    __syncthreads();
}

// One workgroup per slot.  A dead slot, or a step whose active word is clear, writes nothing; a live row without an allowed column
// writes k absent candidates.
template <int KM>
__global__ __launch_bounds__(NT) void sbs_step_kernel(StepArgs a) {
    __shared__ double rd[NW];
    __shared__ float rmx[NW], rmn[NW];
    __shared__ double lk[MAX_K];
    __shared__ int lc[MAX_K];
    const int s = blockIdx.x, b = s / a.k, j = s % a.k, t = a.t, k = a.k;
    if (!a.active[active_read(t)] || !slot_is_live(a.state + (int64_t)b * BS_WORDS, j)) return;      // the same for every thread
    const float* x = a.ll + (int64_t)s * a.ld;
    const auto ok = [&](int c, float y) {
        return allowed(a.flag_shared, a.flag_local, a.owned_local, a.V, a.tot, b, c, t, a.min_t, y);
    };
    float mx = -INFINITY, mn = INFINITY;
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (ok(c, y)) mx = fmaxf(mx, y);
    }
    block_minmax(mx, mn, rmx, rmn);
    const int64_t at = (int64_t)s * k;
    if (!(mx > -INFINITY)) {
        if ((int)threadIdx.x < k) a.cand_tok[at + threadIdx.x] = -1;
        return;
    }
    double z = 0.0;
    for (int c = threadIdx.x; c < a.tot; c += NT) {
        const float y = x[c];
        if (ok(c, y)) z += weight(y, mx, a.T);
    }
    const double lse = log(block_sum(z, rd));
    const double logq_s = a.slot_logq[s], G_s = a.slot_gumbel[s];
    const uint64_t rk = row_key(a.seed, b, j, t);
    row_topk_keys<KM>(a.tot, k, [&](int c, double& key) {
        const float y = x[c];
        if (!ok(c, y)) return false;
        key = child_logq(logq_s, y, mx, a.T, lse) + gumbel(rk, c);
        return true;
    }, lk, lc);
    const int r = threadIdx.x;
    if (r < k) {
        if (lc[r] == INT_MAX) a.cand_tok[at + r] = -1;
        else emit(x, lc[r], lk[r], lk[0], logq_s, G_s, mx, a.T, lse, a.cand_tok + at + r, a.cand_ll + at + r, a.cand_logq + at + r,
                  a.cand_gumbel + at + r);
    }
}

// One workgroup per graph: the pool filled and ranked by counting by all threads, the cut placed by one.  The active[3] rotation of
// csrc/slot_kernels.h; the flag: does some not-done graph have a live slot?
__global__ __launch_bounds__(NT) void sbs_advance_kernel(Tables a) {
    __shared__ double G[MAX_POOL];
    __shared__ uint8_t present[MAX_POOL];
    __shared__ int order[MAX_K], c_step[MAX_K], c_parent[MAX_K];
    __shared__ double c_score[MAX_K], c_logq[MAX_K], s_score[MAX_K];
    const int b = blockIdx.x, t = a.t, k = a.k;
    if (b == 0 && threadIdx.x == 0) a.active[active_clear(t)] = 0;
    const int* st = a.state + (int64_t)b * BS_WORDS;
    if (!a.active[active_read(t)] || st[BS_DONE]) return;
    const int nlive = st[BS_NLIVE], ncomp = st[BS_NCOMP];
    if (nlive < 0 || nlive > k || ncomp < 0 || ncomp > k) return;       // no search produces such words; the pool is sized by them
    const int P = k + nlive * k;
    const Stage stage{c_step, c_parent, c_score, c_logq, s_score};
    for (int p = threadIdx.x; p < P; p += NT) pool_entry(a, b, p, ncomp, G + p, present + p);
    if ((int)threadIdx.x < k) {
        stage_row(a, b, threadIdx.x, stage);
        order[threadIdx.x] = -1;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += NT) {
        if (!present[p]) continue;
        const int r = rank_of(G, present, P, p);
        if (r < k) order[r] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0 && place(a, b, order, G, stage)) atomicOr(a.active + active_set(t), 1);
}

}  // namespace

extern "C" int gtos_sbs_step(int N, int k, int t, int V, int tot, int min_time_step, int max_time_step, float temperature,
                             uint64_t seed, const float* ll, int64_t ld, const uint8_t* flag_shared, const uint8_t* flag_local,
                             const uint8_t* owned_local, const double* slot_logq, const double* slot_gumbel, const int* beam_state,
                             const int* active, int* cand_tok, float* cand_ll, double* cand_logq, double* cand_gumbel, void* stream) {
    if (N <= 0) return 0;
    if (k < 1 || k > MAX_K || N % k || t < 0 || t >= max_time_step || V < 1 || tot < V || ld < tot ||
        !(temperature > 0.0f && temperature < INFINITY))
        return -10;
    if (!ll || !flag_shared || (tot > V && (!flag_local || !owned_local)) || !slot_logq || !slot_gumbel || !beam_state || !active ||
        !cand_tok || !cand_ll || !cand_logq || !cand_gumbel)
        return -23;
    const StepArgs a{N, k, t, V, tot, min_time_step, (double)temperature, seed, ll, ld, flag_shared, flag_local, owned_local, slot_logq,
                     slot_gumbel, beam_state, active, cand_tok, cand_ll, cand_logq, cand_gumbel};
    dispatch_km(k, [&](auto km) {
        hipLaunchKernelGGL(sbs_step_kernel<decltype(km)::value>, dim3((unsigned)N), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    });
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_sbs_advance(int B, int k, int t, int V, int tot, int min_time_step, int max_time_step, const int* cand_tok,
                                const float* cand_ll, const double* cand_logq, const double* cand_gumbel, const uint8_t* flag_shared,
                                const uint8_t* flag_local, double* slot_score, double* slot_logq, double* slot_gumbel, int* beam_state,
                                int* bp_parent, int* bp_token, int* comp_step, int* comp_parent, double* comp_score, double* comp_logq,
                                double* comp_gumbel, int* active, void* stream) {
    if (B <= 0) return 0;
    if (k < 1 || k > MAX_K || t < 0 || t >= max_time_step || V < 1 || tot < V) return -10;
    if (!cand_tok || !cand_ll || !cand_logq || !cand_gumbel || !flag_shared || (tot > V && !flag_local) || !slot_score || !slot_logq ||
        !slot_gumbel || !beam_state || !bp_parent || !bp_token || !comp_step || !comp_parent || !comp_score || !comp_logq ||
        !comp_gumbel || !active)
        return -23;
    const Tables a{B, k, t, V, tot, min_time_step, max_time_step, cand_tok, cand_ll, cand_logq, cand_gumbel, flag_shared, flag_local,
                   slot_score, slot_logq, slot_gumbel, beam_state, bp_parent, bp_token, comp_step, comp_parent, comp_score, comp_logq,
                   comp_gumbel, active};
    hipLaunchKernelGGL(sbs_advance_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
