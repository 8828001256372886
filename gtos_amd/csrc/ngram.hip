// Repeat-n-gram blocking for the device-resident decoders (gtos_amd.search._slot_decode), rule in csrc/ngram_kernels.h (shared with
// the host check).  One launch per step t >= 1, after the decoder's ll and before the step's selection (gtos_beam_topk /
// gtos_sample_step): every live slot's history row is rebuilt from its parent's row of the other buffer plus the token the slot
// took at step t - 1, and the columns that row bans are set to -inf in the slot's ll row.  One workgroup per slot, the row staged
// in LDS, one history position per lane: O(N t) loads per step, none of them dependent on another -- no walk along the
// back-pointers.  Nothing here synchronises with the host.
#include "common.h"
#include "ngram_kernels.h"

using namespace gtos_ngram;

namespace {

constexpr int NT = 256;

struct NgramArgs {
    int N, t, max_t, n, tot;
    float* ll;
    int64_t ld;
    const int* parent;                  // [N] or null: a slot is its own parent
    const int* token;                   // [N]
    const int* hist_prev;               // [N, max_t]
    int* hist_cur;                      // [N, max_t]
    const int* active_t;                // the flag step t's kernels read
};

__global__ __launch_bounds__(NT) void ngram_block_kernel(NgramArgs a) {
    __shared__ int y[MAX_T];
    if (!*a.active_t) return;
    const int s = blockIdx.x, t = a.t;
    const int p = a.parent ? a.parent[s] : s;
    const int tk = a.token[s];
    if (p < 0 || p >= a.N || tk < 0) return;        // a dead slot: its rows stay as they are
    const int* src = a.hist_prev + (int64_t)p * a.max_t;
    int* dst = a.hist_cur + (int64_t)s * a.max_t;
    for (int i = threadIdx.x; i < t; i += NT) {
        const int v = i < t - 1 ? src[i] : tk;
        y[i] = v;
        dst[i] = v;
    }
    __syncthreads();
    float* x = a.ll + (int64_t)s * a.ld;
    for (int i = threadIdx.x; i + a.n <= t; i += NT) {
        const int id = ban_at(y, t, a.n, i);
        if (id >= 0 && id < a.tot) x[id] = -__builtin_inff();
    }
}

}  // namespace

extern "C" int gtos_ngram_block(int N, int k, int t, int max_time_step, int n, int tot, float* ll, int64_t ld, const int* parent,
                                const int* token, const int* hist_prev, int* hist_cur, const int* active, void* stream) {
    if (N <= 0) return 0;
    if (k < 1 || N % k || n < 1 || t < 1 || t >= max_time_step || max_time_step > MAX_T || tot < 1 || ld < tot) return -10;
    if (!ll || !token || !hist_prev || !hist_cur || !active) return -23;
    NgramArgs a{};
    a.N = N; a.t = t; a.max_t = max_time_step; a.n = n; a.tot = tot; a.ll = ll; a.ld = ld; a.parent = parent; a.token = token;
    a.hist_prev = hist_prev; a.hist_cur = hist_cur; a.active_t = active + active_read(t);
    hipLaunchKernelGGL(ngram_block_kernel, dim3((unsigned)N), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
