// Device half of the fixed-slot decode contract (csrc/slot_kernels.h), for the .hip files only: the register top-k pass over one
// ll row, the block reductions of the row kernels (csrc/sample.hip, csrc/sbs.hip) and the write of a slot's next input, with the
// host-side helpers of their entry points.
#pragma once
#include "common.h"
#include "slot_kernels.h"

#include <limits.h>
#include <type_traits>

namespace gtos_slot {

constexpr int NT = 256;                 // 4 waves
constexpr int NW = NT / 64;
constexpr int TOPK_MAX = 32;            // the largest k of row_topk (its LDS, and the widest KM of dispatch_km)

// The k best (value, column) by before() among the columns c of x[0, tot) with allowed(c, x[c]), by one workgroup of NT threads:
// every lane keeps its KM >= k best in registers, sorted, scanning columns lane, lane + NT, ...; each wave then pops its k best by k
// butterfly arg-max rounds over the lanes' heads, and the NW x k wave winners are ranked by counting.  On return (a barrier) the list
// is in the LDS arrays lv / lc [k], sorted; with fewer than k allowed columns the rest of lc holds INT_MAX.  Inlining is left to
// the compiler (it does inline it, predicate included): forced, sample_step_kernel<16> takes 92 VGPRs instead of 75.
template <int KM, class Allowed>
__device__ void row_topk(const float* x, int tot, int k, Allowed allowed, float* lv, int* lc) {
    __shared__ float sv[NW][TOPK_MAX];
    __shared__ int si[NW][TOPK_MAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float v[KM];
    int ix[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) { v[j] = -__builtin_inff(); ix[j] = INT_MAX; }
    for (int c = threadIdx.x; c < tot; c += NT) {
        const float y = x[c];
        if (allowed(c, y) && before(y, c, v[KM - 1], ix[KM - 1])) {
            v[KM - 1] = y; ix[KM - 1] = c;
#pragma unroll
            for (int j = KM - 1; j > 0; --j) {
                if (before(v[j], ix[j], v[j - 1], ix[j - 1])) {
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
            if (before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (ix[0] == bi) {              // the winning lane pops its head (columns are unique; an all-sentinel wave pops sentinels)
#pragma unroll
            for (int j = 0; j < KM - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
            v[KM - 1] = -__builtin_inff(); ix[KM - 1] = INT_MAX;
        }
        if (lane == 0) { sv[w][r] = bv; si[w][r] = bi; }
    }
    if (threadIdx.x < k) lc[threadIdx.x] = INT_MAX;
    __syncthreads();
    const int n = NW * k;
    if (threadIdx.x < n) {
        const float a = sv[threadIdx.x / k][threadIdx.x % k];
        const int ai = si[threadIdx.x / k][threadIdx.x % k];
        int rank = 0;
        for (int q = 0; q < n; ++q) rank += before(sv[q / k][q % k], si[q / k][q % k], a, ai);
        if (rank < k && ai != INT_MAX) { lv[rank] = a; lc[rank] = ai; }
    }
    __syncthreads();
}

// Block-wide reductions: every thread gets the result.  red: NW-entry LDS scratch, free again on return.
__device__ inline double block_sum(double x, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    __syncthreads();
    return s;
}

__device__ inline void block_minmax(float& mx, float& mn, float* rmx, float* rmn) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        mn = fminf(mn, __shfl_xor(mn, o));
    }
    if ((threadIdx.x & 63) == 0) { rmx[threadIdx.x >> 6] = mx; rmn[threadIdx.x >> 6] = mn; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) { mx = fmaxf(mx, rmx[w]); mn = fminf(mn, rmn[w]); }
    __syncthreads();
}

// launch(std::integral_constant<int, KM>) with the narrowest KM >= k of row_topk's instantiations (k <= TOPK_MAX)
template <class Launch>
void dispatch_km(int k, Launch launch) {
    if (k <= 4) launch(std::integral_constant<int, 4>());
    else if (k <= 8) launch(std::integral_constant<int, 8>());
    else if (k <= 16) launch(std::integral_constant<int, 16>());
    else launch(std::integral_constant<int, TOPK_MAX>());
}

// What the next step's input of a slot is read from and written to: token id and character row [C] of every output id, shared
// [V] / [V,C] and per graph [B,tot-V] / [B,tot-V,C] (local_index), the padding input of a dead slot, and the outputs [N] / [N,C]
struct NextInput {
    const int64_t* tok_shared;
    const int64_t* tok_local;
    const int64_t* char_shared;
    const int64_t* char_local;
    int64_t dead_tok;
    const int64_t* dead_char;
    int C;
    int64_t* tok_out;
    int64_t* char_out;
};

// the entry points' null check (-23) of a NextInput
static inline bool next_input_ok(const NextInput& n, int V, int tot) {
    return n.tok_shared && n.char_shared && (tot <= V || (n.tok_local && n.char_local)) && n.dead_char && n.tok_out && n.char_out;
}

// Element c of the next input of slot s of graph b (c == -1: the token id, else character c), the slot's new token being output id
// `id`; id < 0: a dead slot, which gets the padding input.  A slot's whole input is c = -1 .. C-1.
__device__ __forceinline__ void write_next_input(const NextInput& n, int V, int tot, int b, int s, int c, int id) {
    int64_t out;
    if (id < 0) {
        out = c < 0 ? n.dead_tok : n.dead_char[c];
    } else {
        const int64_t lid = local_index(V, tot, b, id);
        if (c < 0) out = id < V ? n.tok_shared[id] : n.tok_local[lid];
        else out = id < V ? n.char_shared[(int64_t)id * n.C + c] : n.char_local[lid * n.C + c];
    }
    if (c < 0) n.tok_out[s] = out;
    else n.char_out[(int64_t)s * n.C + c] = out;
}

}  // namespace gtos_slot
