// The reorder step of the device-resident beam searches, for the .hip files only: the self-attention caches gathered by parent slot
// and the next step's input of every slot.  csrc/beam.hip (gtos_beam_reorder: one beam per graph, liveness width g = k) and
// csrc/diverse.hip (gtos_diverse_reorder: G groups per graph, g = k / G) launch the same kernel; a slot's state words are those of
// its group s / g, its copy tables those of its graph s / k.
#pragma once
#include "beam_kernels.h"
#include "slot_device.h"

namespace gtos_beam {

constexpr int MAX_CACHES = 32;

struct ReorderArgs {
    int n, N, k, g, t, V, tot;
    int64_t q;                          // 16-byte pieces per cache row
    const uint4* src[MAX_CACHES];
    uint4* dst[MAX_CACHES];
    const int* bp_parent_t;             // row t of the back-pointer tables
    const int* bp_token_t;
    const int* state;                   // [N / g, BS_WORDS]
    const int* active_t;                // the flag step t's advance read
    NextInput next;
};

namespace {

__device__ __forceinline__ bool slot_live(const ReorderArgs& a, int s) {
    return a.bp_parent_t[s] >= 0 && !a.state[(int64_t)(s / a.g) * BS_WORDS + BS_DONE];
}

// blockIdx.y < n: cache y, rows [0, t] gathered by parent slot into the other buffer of its pair (dead slots: zero rows);
// blockIdx.y == n: the next step's input token id and character row of every slot (dead slots: the padding input).
// After an iteration that did not run, the caches are left as they are and every slot gets the padding input.
__global__ __launch_bounds__(NT) void beam_reorder_kernel(ReorderArgs a) {
    const bool act = *a.active_t != 0;
    const int64_t stride = (int64_t)gridDim.x * NT;
    if ((int)blockIdx.y == a.n) {
        const int C1 = a.next.C + 1;
        for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < (int64_t)a.N * C1; e += stride) {
            const int s = (int)(e / C1);
            write_next_input(a.next, a.V, a.tot, s / a.k, s, (int)(e % C1) - 1, act && slot_live(a, s) ? a.bp_token_t[s] : -1);
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

// The argument checks and the launch behind both entry points; g: slots per state row (k, or the group width)
inline int reorder_launch(int n_caches, void* const* src, void* const* dst, int64_t row_bytes, int N, int k, int g, int t,
                          int max_time_step, const int* bp_parent, const int* bp_token, const int* state, const int* active, int V,
                          int tot, const NextInput& next, void* stream) {
    if (N <= 0) return 0;
    if (n_caches < 0 || n_caches > MAX_CACHES || row_bytes <= 0 || row_bytes % 16 || k < 1 || k > MAX_K || N % k || g < 1 || k % g ||
        t < 0 || t >= max_time_step || V < 1 || tot < V || next.C < 1)
        return -10;
    ReorderArgs a{};
    a.next = next;
    if ((n_caches && (!src || !dst)) || !bp_parent || !bp_token || !state || !active || !next_input_ok(a.next, V, tot)) return -23;
    a.n = n_caches; a.N = N; a.k = k; a.g = g; a.t = t; a.V = V; a.tot = tot; a.q = row_bytes / 16;
    for (int i = 0; i < n_caches; ++i) {
        if (!src[i] || !dst[i] || (uintptr_t)src[i] % 16 || (uintptr_t)dst[i] % 16 || src[i] == dst[i]) return -25;
        a.src[i] = static_cast<const uint4*>(src[i]);
        a.dst[i] = static_cast<uint4*>(dst[i]);
    }
    a.bp_parent_t = bp_parent + (int64_t)t * N; a.bp_token_t = bp_token + (int64_t)t * N; a.state = state;
    a.active_t = active + active_read(t);
    const int64_t work = (int64_t)(t + 1) * N * a.q;
    const int64_t blocks = (work + NT - 1) / NT;
    const unsigned gx = (unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(gx, (unsigned)n_caches + 1), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}

}  // namespace

}  // namespace gtos_beam
