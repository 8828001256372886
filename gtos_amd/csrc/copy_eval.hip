// Teacher-forced scoring of TokenGenerator's generate/copy mixture (the reference's generator/decoder.py:42-64 with work=True, then the
// gather at the target and the argmax a scorer takes from that row) for gfx950, without the [T,B,V+copies] row.
//
// copy_eval_fwd_kernel: ONE workgroup per (t, b) row, like copy_nll_fwd_kernel and with its code for the loss (row_lse of copy_row.h,
// the target's alignment mass, the gates): nll comes out bitwise as gtos_copy_nll_fwd writes it.  The max reduction of the lse pass
// carries the column of the largest logit, and the row's copy groups are found in LDS (copy_eval_kernels.h states the rule and which
// columns compete), so pred / p_pred cost no second pass over the logits.  Per row it reads the logits once (twice through L2) and
// writes 12 bytes.
// eval_accumulate_kernel: one workgroup folds nll / pred of a batch into per-sentence sums and the running totals of an evaluation
// in a fixed order, so that many batches make one host read.
#include "copy_row.h"
#include "copy_eval_kernels.h"

namespace {

using namespace gtos_row;

struct EvalArgs {
    int T, B, V, S;
    const void* logits; int64_t ld; const void* div; const float* align; const int64_t* cp_seq; const int64_t* target;
    int64_t pad_idx;
    float* nll; int* pred; float* p_pred;
};

template <typename T>
__global__ __launch_bounds__(NT) void copy_eval_fwd_kernel(EvalArgs a) {
    extern __shared__ int64_t ids[];                   // [S] copy ids of graph b, then [S] fp32 alignment of the row
    float* al = reinterpret_cast<float*>(ids + a.S);
    __shared__ float red[NT / 64];
    __shared__ int redi[NT / 64];
    const int row = blockIdx.x, b = row % a.B;
    const T* lp = static_cast<const T*>(a.logits) + (int64_t)row * a.ld;
    const bool vec = (a.V % 8 == 0) && (a.ld % 8 == 0) && ((uintptr_t)a.logits % 16 == 0);
    float top;
    int amax;
    const float lse = row_lse_argmax<T>(lp, a.V, vec, red, redi, &top, &amax);
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
    }
    // ---- the best copy group
    for (int s = threadIdx.x; s < a.S; s += NT) {
        ids[s] = a.cp_seq[(int64_t)s * a.B + b];
        al[s] = a.align[(int64_t)row * a.S + s];
    }
    __syncthreads();
    const T* dp = static_cast<const T*>(a.div) + (int64_t)row * 2;
    float g, c;
    gtos_eval::gates(to_f<T>(dp[0]), to_f<T>(dp[1]), g, c);
    // the same bits as the loss's gates, but opaque to the optimiser: under fast-math it evaluates the loss's g * sig + (1 - g) * mass
    // in a form of its own choosing, and sharing subexpressions with the code below would change that form and with it nll's last bit
    asm volatile("" : "+v"(g), "+v"(c));
    const float sig_top = GTOS_EV_EXP(top - lse);
    float best = -1.f;                                 // below every probability
    int col = gtos_eval::NO_COL;
    for (int s = threadIdx.x; s < a.S; s += NT) {
        if (!gtos_eval::leads(ids, 1, s)) continue;
        const int64_t id = ids[s];
        if (id >= gtos_eval::NO_COL) continue;         // not an int32 column
        const float sig = id < a.V ? gtos_eval::column_sig(to_f<T>(lp[id]), top, sig_top, lse) : 0.f;
        const float p = gtos_eval::group_p(g, c, sig, gtos_eval::group_mass(ids, 1, a.S, s, al));
        if (gtos_eval::better(p, (int)id, best, col)) { best = p; col = (int)id; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float q = __shfl_xor(best, o);
        const int k = __shfl_xor(col, o);
        if (gtos_eval::better(q, k, best, col)) { best = q; col = k; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                   // red / redi may still be read
    if (lane == 0) { red[wave] = best; redi[wave] = col; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (amax < 0 || amax >= a.V) amax = 0;         // (a row without a finite logit)
        float p = g * sig_top;
        int k = amax;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w)
            if (gtos_eval::better(red[w], redi[w], p, k)) { p = red[w]; k = redi[w]; }
        a.pred[row] = k;
        a.p_pred[row] = p;
    }
}

struct AccArgs {
    int T, B;
    const float* nll; const int* pred; const int64_t* target; int64_t pad_idx;
    double* sent_nll; int* sent_tokens; int* sent_correct; double* totals;
};

// One workgroup.  Column b is summed by one thread in t order; the totals are then formed by one thread over the columns in column
// order, so neither depends on scheduling.  A column without a non-pad target is no sentence: it adds nothing to totals[3] / totals[4].
__global__ __launch_bounds__(NT) void eval_accumulate_kernel(AccArgs a) {
    for (int b = threadIdx.x; b < a.B; b += NT) {
        double s = 0.0;
        int n = 0, ok = 0;
        for (int t = 0; t < a.T; ++t) {
            const int64_t r = (int64_t)t * a.B + b;
            const int64_t y = a.target[r];
            if (y == a.pad_idx) continue;
            s += (double)a.nll[r];
            ++n;
            ok += (int64_t)a.pred[r] == y;
        }
        a.sent_nll[b] = s;
        a.sent_tokens[b] = n;
        a.sent_correct[b] = ok;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, n = 0.0, ok = 0.0, sents = 0.0, norm = 0.0;
        for (int b = 0; b < a.B; ++b) {
            const int nb = a.sent_tokens[b];
            if (nb == 0) continue;
            s += a.sent_nll[b];
            n += (double)nb;
            ok += (double)a.sent_correct[b];
            sents += 1.0;
            norm += a.sent_nll[b] / (double)nb;
        }
        a.totals[0] += s;
        a.totals[1] += n;
        a.totals[2] += ok;
        a.totals[3] += sents;
        a.totals[4] += norm;
    }
}

}  // namespace

extern "C" int gtos_copy_eval_fwd(int dtype, int T, int B, int V, int S, const void* logits, int64_t ld_logits, const void* div,
                                  const float* align, const int64_t* cp_seq, const int64_t* target, int64_t pad_idx, float* nll,
                                  int* pred, float* p_pred, void* stream) {
    if (T <= 0 || B <= 0) return 0;
    if (V <= 0 || S < 0 || S > gtos_eval::MAX_S || ld_logits < V) return -24;
    if (!logits || !div || !target || !nll || !pred || !p_pred || (S > 0 && (!align || !cp_seq))) return -23;
    EvalArgs a{};
    a.T = T; a.B = B; a.V = V; a.S = S; a.logits = logits; a.ld = ld_logits; a.div = div; a.align = align; a.cp_seq = cp_seq;
    a.target = target; a.pad_idx = pad_idx; a.nll = nll; a.pred = pred; a.p_pred = p_pred;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)S * (sizeof(int64_t) + sizeof(float));
    if (dtype == GTOS_BF16) hipLaunchKernelGGL(copy_eval_fwd_kernel<bf16_t>, dim3((unsigned)(T * B)), dim3(NT), lds, s, a);
    else hipLaunchKernelGGL(copy_eval_fwd_kernel<float>, dim3((unsigned)(T * B)), dim3(NT), lds, s, a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

extern "C" int gtos_eval_accumulate(int T, int B, const float* nll, const int* pred, const int64_t* target, int64_t pad_idx,
                                    double* sent_nll, int* sent_tokens, int* sent_correct, double* totals, void* stream) {
    if (T < 0 || B < 0) return -24;
    if (!totals || (B > 0 && (!sent_nll || !sent_tokens || !sent_correct)) || (T > 0 && B > 0 && (!nll || !pred || !target))) return -23;
    if (B == 0) return 0;
    AccArgs a{};
    a.T = T; a.B = B; a.nll = nll; a.pred = pred; a.target = target; a.pad_idx = pad_idx;
    a.sent_nll = sent_nll; a.sent_tokens = sent_tokens; a.sent_correct = sent_correct; a.totals = totals;
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
