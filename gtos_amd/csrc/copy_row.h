// The logits-row pass the generate/copy kernels share (csrc/copy_nll.hip, csrc/copy_eval.hip): one 256-thread workgroup per row,
// max and sum-exp in fp32 with DPP wave reductions and an LDS cross-wave step.  The reduction order is fixed by this code, so two
// kernels that call row_lse on the same row get the same bits -- gtos_copy_eval_fwd's nll is bitwise gtos_copy_nll_fwd's.
#pragma once
#include "common.h"

namespace gtos_row {

constexpr int NT = 256;

__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
    v = is_max ? wave_max(v) : wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                               // red may still be read from a previous call
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// this thread's maximum over its slice of the row; with ARG also the lowest column that holds it (INT_MAX for an empty slice)
template <typename T, bool ARG>
__device__ __forceinline__ float slice_max(const T* __restrict__ lp, int V, bool vec, int& col) {
    float m = -INFINITY;
    if (vec) {
        for (int v = threadIdx.x * 8; v < V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (ARG && x[e] > m) col = v + e;      // columns ascend within a slice: strict > keeps the lowest
                m = fmaxf(m, x[e]);
            }
        }
    } else {
        for (int v = threadIdx.x; v < V; v += NT) {
            const float x = to_f<T>(lp[v]);
            if (ARG && x > m) col = v;
            m = fmaxf(m, x);
        }
    }
    return m;
}

// m + log(sum exp(x - m)) given the row's maximum m
template <typename T>
__device__ __forceinline__ float lse_from_max(const T* __restrict__ lp, int V, bool vec, float m, float* red) {
    float s = 0.f;
    if (vec) {
        for (int v = threadIdx.x * 8; v < V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += __expf(x[e] - m);
        }
    } else {
        for (int v = threadIdx.x; v < V; v += NT) s += __expf(to_f<T>(lp[v]) - m);
    }
    s = block_reduce(s, false, red);
    return m + __logf(s);
}

template <typename T>
__device__ __forceinline__ float row_lse(const T* __restrict__ lp, int V, bool vec, float* red) {
    int unused = 0;
    const float m = block_reduce(slice_max<T, false>(lp, V, vec, unused), true, red);
    return lse_from_max<T>(lp, V, vec, m, red);
}

__device__ __forceinline__ int block_min(int v, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) redi[wave] = v;
    __syncthreads();
    int r = redi[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = min(r, redi[w]);
    return r;
}

// row_lse that also carries the argmax through the max reduction: *col = the lowest column holding the row's largest logit and
// *top = that logit.  The maximum is exact in any order, so lse has the bits row_lse gives.
template <typename T>
__device__ __forceinline__ float row_lse_argmax(const T* __restrict__ lp, int V, bool vec, float* red, int* redi, float* top,
                                                int* col) {
    int mine = 0x7fffffff;
    const float mt = slice_max<T, true>(lp, V, vec, mine);
    const float m = block_reduce(mt, true, red);
    *col = block_min(mt == m ? mine : 0x7fffffff, redi);
    *top = m;
    return lse_from_max<T>(lp, V, vec, m, red);
}

}  // namespace gtos_row
