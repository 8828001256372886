// Token-level attribution of TokenGenerator's generate/copy mixture for gfx950: per teacher-forced row, where the target's probability
// came from (copy gate, share of it that was copied, the graph position it was copied from), how sure the model was (entropy of the
// mixture) and how many columns it preferred (rank) -- without the [T,B,V+copies] row.  The rule is in copy_explain_kernels.h.
//
// copy_explain_fwd_kernel: ONE workgroup per (t, b) row, the shape of copy_eval_fwd_kernel.  The two logits passes of the lse and the
// loss tail are copy_eval_fwd_kernel's, so nll has its bits.  cp_seq column b and the row's alignment are staged in LDS; one scan over
// the positions gives focus, source and the mass of the target's group, ONE further pass over the logits row (L2-resident) gives Z, E
// and the vocabulary part of the rank, and the scan over the leading positions corrects entropy and rank at the columns that carry
// copy mass.  Every reduction runs in a fixed order: two launches give the same bits.  Per row it reads the logits three times (twice
// through L2) and writes 36 bytes.
#include "copy_row.h"
#include "copy_explain_kernels.h"

namespace {

using namespace gtos_row;

struct ExplainArgs {
    int T, B, V, S;
    const void* logits; int64_t ld; const void* div; const float* align; const int64_t* cp_seq; const int64_t* target;
    int64_t pad_idx;
    float* nll; float* entropy; float* gate; float* copy_share; int* source; float* source_weight; int* focus; float* focus_weight;
    int* rank;
};

// the heaviest (weight, position) of the block in every thread, gtos_explain::heavier deciding
__device__ __forceinline__ void block_heaviest(float& w, int& s, float* red, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float w2 = __shfl_xor(w, o);
        const int s2 = __shfl_xor(s, o);
        if (gtos_explain::heavier(w2, s2, w, s)) { w = w2; s = s2; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                   // red / redi may still be read
    if (lane == 0) { red[wave] = w; redi[wave] = s; }
    __syncthreads();
    w = red[0];
    s = redi[0];
#pragma unroll
    for (int k = 1; k < NT / 64; ++k)
        if (gtos_explain::heavier(red[k], redi[k], w, s)) { w = red[k]; s = redi[k]; }
}

__device__ __forceinline__ int block_sum_int(int v, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) redi[wave] = v;
    __syncthreads();
    int r = redi[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) r += redi[w];
    return r;
}

template <typename T>
__global__ __launch_bounds__(NT) void copy_explain_fwd_kernel(ExplainArgs a) {
    extern __shared__ int64_t ids[];                   // [S] copy ids of graph b, then [S] fp32 alignment of the row
    float* al = reinterpret_cast<float*>(ids + a.S);
    __shared__ float red[NT / 64];
    __shared__ int redi[NT / 64];
    __shared__ float mass_sh;                          // alignment mass of the target's group, members in ascending position
    const int row = blockIdx.x, b = row % a.B;
    const T* lp = static_cast<const T*>(a.logits) + (int64_t)row * a.ld;
    const bool vec = (a.V % 8 == 0) && (a.ld % 8 == 0) && ((uintptr_t)a.logits % 16 == 0);
    int unused = 0;
    const float m = block_reduce(slice_max<T, false>(lp, a.V, vec, unused), true, red);      // (row_lse, keeping the maximum)
    const float lse = lse_from_max<T>(lp, a.V, vec, m, red);
    // ---- the loss, as copy_nll_fwd_kernel computes it
    const int64_t tgt = a.target[row];
    float mass = 0.f;
    for (int s = threadIdx.x; s < a.S; s += NT)
        if (a.cp_seq[(int64_t)s * a.B + b] == tgt) mass += a.align[(int64_t)row * a.S + s];
    mass = block_reduce(mass, false, red);
    if (threadIdx.x == 0) {                            // (textually copy_nll_fwd_kernel's tail: the compiler must see the same expression)
        const T* dp = static_cast<const T*>(a.div) + (int64_t)row * 2;
        const float d0 = to_f<T>(dp[0]), d1 = to_f<T>(dp[1]);
        const float g = 1.f / (1.f + __expf(d1 - d0)), c = 1.f - g;
        const float sig = (tgt >= 0 && tgt < a.V) ? __expf(to_f<T>(lp[tgt]) - lse) : 0.f;
        float p = g * sig + c * mass;
        asm volatile("" : "+v"(p));                    // copy_nll_fwd_kernel stores p (p_tgt): keep it a value here too, or fast-math folds
                                                       // the 1e-12 into the mixture and the logarithm sees another rounding
        a.nll[row] = tgt == a.pad_idx ? 0.f : -__logf(p + 1e-12f);
        mass_sh = 0.f;
    }
    // ---- the alignment: focus, source and the mass of the target's group
    for (int s = threadIdx.x; s < a.S; s += NT) {
        ids[s] = a.cp_seq[(int64_t)s * a.B + b];
        al[s] = a.align[(int64_t)row * a.S + s];
    }
    __syncthreads();
    const T* dp = static_cast<const T*>(a.div) + (int64_t)row * 2;
    float g, c;
    gtos_eval::gates(to_f<T>(dp[0]), to_f<T>(dp[1]), g, c);
    // the same bits as the loss's gates, but opaque to the optimiser: sharing subexpressions with the loss tail would change the form
    // fast-math gives it and with it nll's last bit (see copy_eval_fwd_kernel)
    asm volatile("" : "+v"(g), "+v"(c));
    float gs = g * GTOS_EV_EXP(m - lse);
    asm volatile("" : "+v"(gs));                       // one value per row: q of a column is gs * col_e at every site
    const bool live = tgt != a.pad_idx && tgt >= 0;
    float fw = -INFINITY, sw = -INFINITY;
    int f = gtos_explain::NONE, src = gtos_explain::NONE;
    for (int s = threadIdx.x; s < a.S; s += NT) {
        const float w = al[s];
        if (gtos_explain::heavier(w, s, fw, f)) { fw = w; f = s; }
        if (live && ids[s] == tgt) {
            if (gtos_explain::heavier(w, s, sw, src)) { sw = w; src = s; }
            if (gtos_eval::leads(ids, 1, s)) mass_sh = gtos_eval::group_mass(ids, 1, a.S, s, al);      // one thread of the block at most
        }
    }
    block_heaviest(fw, f, red, redi);
    block_heaviest(sw, src, red, redi);                // (its barriers also publish mass_sh)
    const float mass_y = mass_sh;
    const bool reachable = live && (tgt < a.V || src != gtos_explain::NONE);
    const float q_y = (reachable && tgt < a.V) ? gs * gtos_explain::col_e(to_f<T>(lp[tgt]), m) : 0.f;
    float p_y = gtos_eval::group_p(1.f, c, q_y, mass_y);
    asm volatile("" : "+v"(p_y));                      // a value: every comparison below sees these bits
    // ---- the logits row once more: Z, E and the vocabulary columns above the target
    float Z = 0.f, E = 0.f;
    int above = 0;
    if (vec) {
        for (int v = threadIdx.x * 8; v < a.V; v += NT * 8) {
            float x[8];
            Vec8<T>::load(lp + v, x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float ex = gtos_explain::col_e(x[e], m);
                Z += ex;
                E += ex * (x[e] - m);
                above += (v + e != tgt) && (gs * ex > p_y);
            }
        }
    } else {
        for (int v = threadIdx.x; v < a.V; v += NT) {
            const float x = to_f<T>(lp[v]);
            const float ex = gtos_explain::col_e(x, m);
            Z += ex;
            E += ex * (x - m);
            above += (v != tgt) && (gs * ex > p_y);
        }
    }
    // ---- the columns that carry copy mass: entropy and rank corrected at the leading positions
    float H = 0.f;
    for (int s = threadIdx.x; s < a.S; s += NT) {
        if (!gtos_eval::leads(ids, 1, s)) continue;
        const int64_t id = ids[s];
        const float q = id < a.V ? gs * gtos_explain::col_e(to_f<T>(lp[id]), m) : 0.f;
        const float p = gtos_eval::group_p(1.f, c, q, gtos_eval::group_mass(ids, 1, a.S, s, al));
        H += gtos_explain::h(p) - gtos_explain::h(q);
        if (id != tgt) above += (int)(p > p_y) - (int)(id < a.V && q > p_y);
    }
    Z = block_reduce(Z, false, red);
    E = block_reduce(E, false, red);
    H = block_reduce(H, false, red);
    above = block_sum_int(above, redi);
    if (threadIdx.x == 0) {
        a.entropy[row] = gtos_explain::vocab_entropy(g, Z, E) + H;
        a.gate[row] = c;
        a.copy_share[row] = reachable ? gtos_explain::share(q_y, c * mass_y) : 0.f;
        a.source[row] = src == gtos_explain::NONE ? -1 : src;
        a.source_weight[row] = src == gtos_explain::NONE ? 0.f : sw;
        a.focus[row] = f == gtos_explain::NONE ? -1 : f;
        a.focus_weight[row] = f == gtos_explain::NONE ? 0.f : fw;
        a.rank[row] = reachable ? above : -1;
    }
}

}  // namespace

extern "C" int gtos_copy_explain_fwd(int dtype, int T, int B, int V, int S, const void* logits, int64_t ld_logits, const void* div,
                                     const float* align, const int64_t* cp_seq, const int64_t* target, int64_t pad_idx, float* nll,
                                     float* entropy, float* gate, float* copy_share, int* source, float* source_weight, int* focus,
                                     float* focus_weight, int* rank, void* stream) {
    if (T <= 0 || B <= 0) return 0;
    if (V <= 0 || S < 0 || S > gtos_eval::MAX_S || ld_logits < V) return -24;
    if (!logits || !div || !target || !nll || !entropy || !gate || !copy_share || !source || !source_weight || !focus || !focus_weight ||
        !rank || (S > 0 && (!align || !cp_seq)))
        return -23;
    ExplainArgs a{};
    a.T = T; a.B = B; a.V = V; a.S = S; a.logits = logits; a.ld = ld_logits; a.div = div; a.align = align; a.cp_seq = cp_seq;
    a.target = target; a.pad_idx = pad_idx; a.nll = nll; a.entropy = entropy; a.gate = gate; a.copy_share = copy_share;
    a.source = source; a.source_weight = source_weight; a.focus = focus; a.focus_weight = focus_weight; a.rank = rank;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)S * (sizeof(int64_t) + sizeof(float));
    if (dtype == GTOS_BF16) hipLaunchKernelGGL(copy_explain_fwd_kernel<bf16_t>, dim3((unsigned)(T * B)), dim3(NT), lds, s, a);
    else hipLaunchKernelGGL(copy_explain_fwd_kernel<float>, dim3((unsigned)(T * B)), dim3(NT), lds, s, a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
