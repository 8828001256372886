// Clipped n-gram overlap of sequence pairs (gtos_amd.metrics: BLEU and chrF++ of decoded text), rule in csrc/overlap_kernels.h
// (shared with the host check).  R sequences of int32 symbols in CSR form (sym, off [R+1]) and a list of P (hypothesis row,
// reference row) pairs; one 256-thread workgroup per pair.  Both rows are staged in LDS (at most 2 x 16 KiB), the hypothesis
// positions are strided over the threads -- lane l of a wave reads h[i + l + c], consecutive words, and every lane the same
// reference word, a broadcast: no bank conflicts on either side -- the per-order counters of a position and the thread's running
// totals stay in registers, and one workgroup reduction (shuffles inside a wave, a [4][8] table across the waves) ends in one
// store of the pair's 3 * n_max integers.  Integer arithmetic throughout and no atomics: two launches give the same values, and
// they equal the host's.  Nothing here synchronises with the host.
#include "common.h"
#include "overlap_kernels.h"

using namespace gtos_overlap;

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;

struct OverlapArgs {
    const int* sym;                     // the symbols of all rows
    const int* off;                     // [R + 1]
    const int* pairs;                   // [P, 2]
    int R, n_max;
    int* out;                           // [P, n_max, 3]
};

__global__ __launch_bounds__(NT) void ngram_overlap_kernel(OverlapArgs a) {
    __shared__ int h[MAX_SYMBOLS];
    __shared__ int r[MAX_SYMBOLS];
    __shared__ int part[WAVES][MAX_ORDER];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int hrow = a.pairs[2 * (int64_t)p], rrow = a.pairs[2 * (int64_t)p + 1];
    // the entry point has checked the host copies of off and pairs; a device copy that disagrees with them stores nothing
    if (hrow < 0 || hrow >= a.R || rrow < 0 || rrow >= a.R) return;
    const int h0 = a.off[hrow], Lh = a.off[hrow + 1] - h0, r0 = a.off[rrow], Lr = a.off[rrow + 1] - r0;
    if (h0 < 0 || r0 < 0 || Lh < 0 || Lh > MAX_SYMBOLS || Lr < 0 || Lr > MAX_SYMBOLS) return;
    for (int i = tid; i < Lh; i += NT) h[i] = a.sym[h0 + i];
    for (int i = tid; i < Lr; i += NT) r[i] = a.sym[r0 + i];
    __syncthreads();
    int total[MAX_ORDER];
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) total[n] = 0;
    for (int i = tid; i < Lh; i += NT) {
        int counts[MAX_ORDER];
        position_counts(h, Lh, r, Lr, a.n_max, i, counts);
#pragma unroll
        for (int n = 0; n < MAX_ORDER; ++n) total[n] += counts[n];
    }
#pragma unroll
    for (int n = 0; n < MAX_ORDER; ++n) {
        int v = total[n];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((tid & 63) == 0) part[tid >> 6][n] = v;
    }
    __syncthreads();
    if (tid < a.n_max * STATS) {
        const int n = tid / STATS, s = tid % STATS;
        int v;
        if (s == 0) {
            v = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) v += part[w][n];
        } else {
            v = n_grams(s == 1 ? Lh : Lr, n + 1);
        }
        a.out[(int64_t)p * a.n_max * STATS + tid] = v;
    }
}

}  // namespace

extern "C" int gtos_ngram_overlap(const int* sym, const int* off, int R, const int* pairs, int P, int n_max, const int* off_host,
                                  const int* pairs_host, int* out, void* stream) {
    if (R < 0 || P < 0 || !off_host || (P > 0 && !pairs_host)) return -10;
    if (check_launch(off_host, R, pairs_host, P, n_max)) return -10;
    if (P == 0) return 0;
    if (!off || !pairs || !out || (!sym && off_host[R] > 0)) return -10;
    OverlapArgs a{};
    a.sym = sym; a.off = off; a.pairs = pairs; a.R = R; a.n_max = n_max; a.out = out;
    hipLaunchKernelGGL(ngram_overlap_kernel, dim3((unsigned)P), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
