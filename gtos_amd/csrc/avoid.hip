// Negative constraints for the device-resident decoders (gtos_amd.search._slot_decode), rule in csrc/avoid_kernels.h (shared with
// the host check).  One launch per step t >= 0, after the decoder's ll and before the step's selection (gtos_beam_topk /
// gtos_sample_step): every live slot's matcher word is stepped from its parent's word of the other buffer with the token the slot took
// at step t - 1, and the columns that word bans are set to -inf in the slot's ll row.  One wave per slot, lane i holding pat[i] of
// the slot's graph: MASK(token) is one ballot, and the lanes whose bit is set in the ban word store.  No history is read, nothing
// depends on t but the first step, and nothing here synchronises with the host.
#include "common.h"
#include "avoid_kernels.h"

using namespace gtos_avoid;

namespace {

constexpr int NT = 256;
constexpr int SLOTS = NT / MAX_POS;     // slots per workgroup: one per wave

struct AvoidArgs {
    int N, k, t, tot;
    float* ll;
    int64_t ld;
    const int* parent;                  // [N] or null: a slot is its own parent
    const int* token;                   // [N]; not read at t == 0
    const int* pat;                     // [B, MAX_POS]
    const uint64_t* init;               // [B]
    const uint64_t* last;               // [B]
    const int* n_pos;                   // [B]
    const uint64_t* state_prev;         // [N]
    uint64_t* state_cur;                // [N]
    const int* active_t;                // the flag step t's kernels read
};

__global__ __launch_bounds__(NT) void avoid_block_kernel(AvoidArgs a) {
    if (!*a.active_t) return;
    const int lane = threadIdx.x % MAX_POS;
    const int s = blockIdx.x * SLOTS + threadIdx.x / MAX_POS;
    if (s >= a.N) return;
    const int b = s / a.k;
    const uint64_t init = a.init[b];
    const int mine = lane < a.n_pos[b] ? a.pat[(int64_t)b * MAX_POS + lane] : -1;
    uint64_t d = 0;                                 // t == 0: no parent, no token
    if (a.t > 0) {
        const int p = a.parent ? a.parent[s] : s;
        const int tk = a.token[s];
        if (p < 0 || p >= a.N || tk < 0) return;    // a dead slot (the whole wave): its row and its word stay as they are
        d = next_state(a.state_prev[p], init, __ballot(mine == tk));
    }
    if (lane == 0) a.state_cur[s] = d;
    const int id = ban_at(ban_word(d, init, a.last[b]), lane, mine);
    if (id >= 0 && id < a.tot) a.ll[(int64_t)s * a.ld + id] = -__builtin_inff();
}

}  // namespace

extern "C" int gtos_avoid_block(int N, int k, int t, int tot, float* ll, int64_t ld, const int* parent, const int* token,
                                const int* pat, const uint64_t* init, const uint64_t* last, const int* n_pos,
                                const uint64_t* state_prev, uint64_t* state_cur, const int* active, void* stream) {
    if (N <= 0) return 0;
    if (k < 1 || N % k || t < 0 || tot < 1 || ld < tot || state_prev == state_cur) return -10;
    if (!ll || (t > 0 && !token) || !pat || !init || !last || !n_pos || !state_prev || !state_cur || !active) return -23;
    AvoidArgs a{};
    a.N = N; a.k = k; a.t = t; a.tot = tot; a.ll = ll; a.ld = ld; a.parent = parent; a.token = token; a.pat = pat; a.init = init;
    a.last = last; a.n_pos = n_pos; a.state_prev = state_prev; a.state_cur = state_cur; a.active_t = active + active_read(t);
    hipLaunchKernelGGL(avoid_block_kernel, dim3((unsigned)((N + SLOTS - 1) / SLOTS)), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
