// Label-smoothed generate/copy loss of TokenGenerator (label_smoothed_nll_loss applied to the ll row of generator/decoder.py:40-63)
// for gfx950.  The per-row arithmetic is csrc/copy_ls_kernels.h (shared with a host statement the CPU tests compile).
//
// Smoothing needs sum_k log p_k over the whole extended row [0, C), C = max(V, 1 + max(cp_seq)), not just p(target), but the row is
// still never materialised:
//   _prep (one workgroup per graph): C, and per graph the groups of equal copy ids (ids, member lists in ascending position, the group
//          of every position), how many distinct ids lie at or above V, and a bitmap of the vocabulary columns that are copy ids;
//   _fwd  (one workgroup per (t, b) row): lse in two passes over the logits, a third pass over the non-copy vocabulary columns, one
//          thread per copy group for the copy columns (the C - V - nbig empty columns add only a constant); writes the loss, lse and the two
//          row sums (Sw, Sc) that make the backward a single pass;
//   _bwd  (one workgroup per row): the groups' dloss/dp into LDS, then one pass writing d(logits), dense d(alignment) and d(diverter).
// C is read from the workspace on the device: a captured graph replayed on a batch with other copy ids stays correct.
#include "common.h"
#include "copy_ls_kernels.h"

namespace {

using namespace gtos_ls;
constexpr int NT = 256;

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r = fmaxf(r, red[w]);
    return r;
}

// four block sums at once (one pair of barriers)
__device__ __forceinline__ void block_sum4(float (&v)[4], float* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[i * (NT / 64) + wave] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float r = red[i * (NT / 64)];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) r += red[i * (NT / 64) + w];
        v[i] = r;
    }
}

template <typename T>
__device__ __forceinline__ float row_lse(const T* __restrict__ lp, int V, bool vec, float* red) {
    float m = -INFINITY;
    if (vec) {
        for (int v = threadIdx.x * 8; v < V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fmaxf(m, x[e]);
        }
    } else {
        for (int v = threadIdx.x; v < V; v += NT) m = fmaxf(m, to_f<T>(lp[v]));
    }
    m = block_max(m, red);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        for (int v = threadIdx.x * 8; v < V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[0] += __expf(x[e] - m);
        }
    } else {
        for (int v = threadIdx.x; v < V; v += NT) s[0] += __expf(to_f<T>(lp[v]) - m);
    }
    block_sum4(s, red);
    return m + __logf(s[0]);
}

struct LsArgs {
    int T, B, V, S;
    float eps;
    const void* logits; int64_t ld; const void* div; const float* align; const int64_t* target; int64_t pad_idx;
    const int* ws;
    float* loss; float* lse; float* sums;                                     // forward outputs (sums [T,B,2] = Sw, Sc)
    const float* d_loss; void* d_logits; void* d_div; float* d_align;        // backward
};

struct RowTables {
    const int *gid, *gstart, *gpos, *grp, *bm;
    int ng, C;
    __device__ RowTables(const int* ws, int B, int S, int V, int b) {
        const Layout L(B, S, V);
        gid = ws + L.gid + (int64_t)b * S; gstart = ws + L.gstart + (int64_t)b * (S + 1); gpos = ws + L.gpos + (int64_t)b * S;
        grp = ws + L.grp + (int64_t)b * S; bm = ws + L.bm + (int64_t)b * L.W;
        ng = ws[L.ngrp + b]; C = ws[0];
    }
};

__global__ __launch_bounds__(NT) void ls_prep_kernel(int B, int S, int V, const int64_t* __restrict__ cp, int* __restrict__ ws) {
    __shared__ int lead[MAX_S], size_or_start[MAX_S], gix[MAX_S];
    __shared__ int n_grp, n_big, n_valid;
    __shared__ long long red[NT];
    const int b = blockIdx.x;
    const Layout L(B, S, V);
    if (b == 0) {                                   // C = max(V, 1 + max(cp_seq)) over the whole batch
        long long m = -1;
        for (int64_t i = threadIdx.x; i < (int64_t)S * B; i += NT) m = cp[i] > m ? cp[i] : m;
        red[threadIdx.x] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < NT; ++i) m = red[i] > m ? red[i] : m;
            ws[0] = (int)(m + 1 > V ? m + 1 : V);
        }
    }
    int* gid = ws + L.gid + (int64_t)b * S;
    int* gstart = ws + L.gstart + (int64_t)b * (S + 1);
    int* gpos = ws + L.gpos + (int64_t)b * S;
    int* grp = ws + L.grp + (int64_t)b * S;
    int* bm = ws + L.bm + (int64_t)b * L.W;
    for (int64_t w = threadIdx.x; w < L.W; w += NT) bm[w] = 0;
    if (threadIdx.x == 0) { n_grp = 0; n_big = 0; n_valid = 0; }
    for (int s = threadIdx.x; s < S; s += NT) {
        lead[s] = leader_of(cp, B, b, s);
        size_or_start[s] = lead[s] == s ? group_size(cp, B, S, b, s) : 0;
    }
    __threadfence_block();                          // the bitmap's zero stores before the ORs below
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += NT) {
        if (lead[s] < 0) continue;
        atomicAdd(&n_valid, 1);
        if (lead[s] != s) continue;
        int gi = 0, start = 0;
        for (int j = 0; j < s; ++j)
            if (lead[j] == j) { ++gi; start += size_or_start[j]; }
        const int64_t id = cp_id(cp, B, b, s);
        gix[s] = gi;
        gid[gi] = (int)id;
        gstart[gi] = start;
        atomicAdd(&n_grp, 1);
        if (id >= V) atomicAdd(&n_big, 1);
        else atomicOr(bm + (id >> 5), (int)(1u << (id & 31)));
    }
    __threadfence_block();                          // gstart before the member lists below
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += NT) {
        const int l = lead[s];
        if (l < 0) { grp[s] = -1; continue; }
        const int gi = gix[l];
        grp[s] = gi;
        gpos[gstart[gi] + rank_in_group(cp, B, b, s)] = s;
    }
    if (threadIdx.x == 0) {
        gstart[n_grp] = n_valid;
        ws[L.ngrp + b] = n_grp;
        ws[L.nbig + b] = n_big;
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void ls_fwd_kernel(LsArgs a) {
    __shared__ float red[4 * (NT / 64)];
    const int row = blockIdx.x, b = row % a.B;
    const T* lp = static_cast<const T*>(a.logits) + (int64_t)row * a.ld;
    const bool vec = (a.V % 8 == 0) && (a.ld % 8 == 0) && ((uintptr_t)a.logits % 16 == 0);
    const float lse = row_lse<T>(lp, a.V, vec, red);
    const RowTables R(a.ws, a.B, a.S, a.V, b);
    const float eps_c = a.eps / (float)R.C;
    const T* dp = static_cast<const T*>(a.div) + (int64_t)row * 2;
    float g, c;
    gates(to_f<T>(dp[0]), to_f<T>(dp[1]), g, c);
    const int64_t y = a.target[row];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};            // sum of ll offsets, Sw, Sc, p(target)
    if (vec) {
        for (int v = threadIdx.x * 8; v < a.V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
            const uint32_t bits = ((uint32_t)R.bm[v >> 5]) >> (v & 31);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if ((bits >> e) & 1u) continue;
                const float s = __expf(x[e] - lse), p = g * s;
                const bool tg = (int64_t)(v + e) == y;
                acc[0] += col_off(p);
                acc[1] += col_w(p, tg, a.eps, eps_c) * s;
                if (tg) acc[3] = p;
            }
        }
    } else {
        for (int v = threadIdx.x; v < a.V; v += NT) {
            if (bit(R.bm, v)) continue;
            const float s = __expf(to_f<T>(lp[v]) - lse), p = g * s;
            const bool tg = (int64_t)v == y;
            acc[0] += col_off(p);
            acc[1] += col_w(p, tg, a.eps, eps_c) * s;
            if (tg) acc[3] = p;
        }
    }
    const float* al = a.align + (int64_t)row * a.S;
    for (int gi = threadIdx.x; gi < R.ng; gi += NT) {
        const int id = R.gid[gi];
        const float m = group_mass(R.gstart, R.gpos, gi, al);
        const float s = id < a.V ? __expf(to_f<T>(lp[id]) - lse) : 0.f;
        const float p = g * s + c * m, w = col_w(p, (int64_t)id == y, a.eps, eps_c);
        acc[0] += col_off(p);
        acc[1] += w * s;
        acc[2] += m * w;
        if ((int64_t)id == y) acc[3] = p;
    }
    block_sum4(acc, red);
    if (threadIdx.x == 0) {
        a.loss[row] = y == a.pad_idx ? 0.f : row_loss(acc[3], acc[0], a.eps, eps_c);
        a.lse[row] = lse;
        a.sums[2 * (int64_t)row] = acc[1];
        a.sums[2 * (int64_t)row + 1] = acc[2];
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void ls_bwd_kernel(LsArgs a) {
    extern __shared__ float lds[];                  // [ngrp] group ids, [ngrp] their dloss/dp
    int* gid_l = reinterpret_cast<int*>(lds);
    float* w_l = lds + a.S;
    const int row = blockIdx.x, b = row % a.B;
    const T* lp = static_cast<const T*>(a.logits) + (int64_t)row * a.ld;
    T* dl = static_cast<T*>(a.d_logits) + (int64_t)row * a.V;
    const bool vec = (a.V % 8 == 0) && (a.ld % 8 == 0) && ((uintptr_t)a.logits % 16 == 0) && ((uintptr_t)a.d_logits % 16 == 0);
    const RowTables R(a.ws, a.B, a.S, a.V, b);
    const float eps_c = a.eps / (float)R.C;
    const int64_t y = a.target[row];
    const float lse = a.lse[row], sw = a.sums[2 * (int64_t)row], sc = a.sums[2 * (int64_t)row + 1];
    const float u = y == a.pad_idx ? 0.f : a.d_loss[row];
    const T* dp = static_cast<const T*>(a.div) + (int64_t)row * 2;
    float g, c;
    gates(to_f<T>(dp[0]), to_f<T>(dp[1]), g, c);
    const float* al = a.align + (int64_t)row * a.S;
    for (int gi = threadIdx.x; gi < R.ng; gi += NT) {
        const int id = R.gid[gi];
        const float m = group_mass(R.gstart, R.gpos, gi, al);
        const float s = id < a.V ? __expf(to_f<T>(lp[id]) - lse) : 0.f;
        gid_l[gi] = id;
        w_l[gi] = col_w(g * s + c * m, (int64_t)id == y, a.eps, eps_c);
    }
    __syncthreads();
    if (vec) {
        for (int v = threadIdx.x * 8; v < a.V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
            const uint32_t bits = ((uint32_t)R.bm[v >> 5]) >> (v & 31);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float s = __expf(x[e] - lse);
                float w;
                if ((bits >> e) & 1u) {
                    int gi = 0;
                    while (gi < R.ng - 1 && gid_l[gi] != v + e) ++gi;
                    w = w_l[gi];
                } else {
                    w = col_w(g * s, (int64_t)(v + e) == y, a.eps, eps_c);
                }
                x[e] = d_logit(u, g, s, w, sw);
            }
            Vec8<T>::store(dl + v, x);
        }
    } else {
        for (int v = threadIdx.x; v < a.V; v += NT) {
            const float s = __expf(to_f<T>(lp[v]) - lse);
            float w;
            if (bit(R.bm, v)) {
                int gi = 0;
                while (gi < R.ng - 1 && gid_l[gi] != v) ++gi;
                w = w_l[gi];
            } else {
                w = col_w(g * s, (int64_t)v == y, a.eps, eps_c);
            }
            dl[v] = from_f<T>(d_logit(u, g, s, w, sw));
        }
    }
    for (int s = threadIdx.x; s < a.S; s += NT) {
        const int gi = R.grp[s];
        a.d_align[(int64_t)row * a.S + s] = gi >= 0 ? u * c * w_l[gi] : 0.f;
    }
    if (threadIdx.x == 0) {
        float dd0, dd1;
        d_gates(u, g, c, sw, sc, dd0, dd1);
        T* dd = static_cast<T*>(a.d_div) + (int64_t)row * 2;
        dd[0] = from_f<T>(dd0);
        dd[1] = from_f<T>(dd1);
    }
}

int check_shape(int T, int B, int V, int S, int64_t ld_logits, float eps, int64_t ws_words) {
    if (V <= 0 || S < 0 || S > MAX_S || ld_logits < V || !(eps >= 0.f && eps <= 1.f)) return -24;
    if ((int64_t)T * B > 0x7fffffff || ws_words < Layout(B, S, V).total) return -24;
    return 0;
}

}  // namespace

extern "C" int gtos_copy_nll_ls_prep(int B, int S, int V, const int64_t* cp_seq, int* ws, int64_t ws_words, void* stream) {
    if (B <= 0) return 0;
    if (V <= 0 || S < 0 || S > MAX_S || ws_words < Layout(B, S, V).total) return -24;
    if (!ws || (S > 0 && !cp_seq)) return -23;
    hipLaunchKernelGGL(ls_prep_kernel, dim3((unsigned)B), dim3(NT), 0, static_cast<hipStream_t>(stream), B, S, V, cp_seq, ws);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_copy_nll_ls_fwd(int dtype, int T, int B, int V, int S, const void* logits, int64_t ld_logits, const void* div,
                                    const float* align, const int64_t* target, int64_t pad_idx, float eps, const int* ws,
                                    int64_t ws_words, float* loss, float* lse, float* sums, void* stream) {
    if (T <= 0 || B <= 0) return 0;
    if (int rc = check_shape(T, B, V, S, ld_logits, eps, ws_words)) return rc;
    if (!logits || !div || !target || !ws || !loss || !lse || !sums || (S > 0 && !align)) return -23;
    LsArgs a{};
    a.T = T; a.B = B; a.V = V; a.S = S; a.eps = eps; a.logits = logits; a.ld = ld_logits; a.div = div; a.align = align;
    a.target = target; a.pad_idx = pad_idx; a.ws = ws; a.loss = loss; a.lse = lse; a.sums = sums;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == GTOS_BF16) hipLaunchKernelGGL(ls_fwd_kernel<bf16_t>, dim3((unsigned)(T * B)), dim3(NT), 0, s, a);
    else hipLaunchKernelGGL(ls_fwd_kernel<float>, dim3((unsigned)(T * B)), dim3(NT), 0, s, a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_copy_nll_ls_bwd(int dtype, int T, int B, int V, int S, const void* logits, int64_t ld_logits, const void* div,
                                    const float* align, const int64_t* target, int64_t pad_idx, float eps, const int* ws,
                                    int64_t ws_words, const float* lse, const float* sums, const float* d_loss, void* d_logits,
                                    void* d_div, float* d_align, void* stream) {
    if (T <= 0 || B <= 0) return 0;
    if (int rc = check_shape(T, B, V, S, ld_logits, eps, ws_words)) return rc;
    if (!logits || !div || !target || !ws || !lse || !sums || !d_loss || !d_logits || !d_div || (S > 0 && (!align || !d_align)))
        return -23;
    LsArgs a{};
    a.T = T; a.B = B; a.V = V; a.S = S; a.eps = eps; a.logits = logits; a.ld = ld_logits; a.div = div; a.align = align;
    a.target = target; a.pad_idx = pad_idx; a.ws = ws; a.lse = const_cast<float*>(lse); a.sums = const_cast<float*>(sums);
    a.d_loss = d_loss; a.d_logits = d_logits; a.d_div = d_div; a.d_align = d_align;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)(S > 0 ? S : 1) * 8;
    if (dtype == GTOS_BF16) hipLaunchKernelGGL(ls_bwd_kernel<bf16_t>, dim3((unsigned)(T * B)), dim3(NT), lds, s, a);
    else hipLaunchKernelGGL(ls_bwd_kernel<float>, dim3((unsigned)(T * B)), dim3(NT), lds, s, a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
