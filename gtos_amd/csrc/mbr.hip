// All-pairs clipped n-gram overlap inside groups of candidates (gtos_amd.metrics.pairwise: the count under minimum-Bayes-risk
// selection), rule and schedule in csrc/mbr_kernels.h (shared with the host check).  R rows of int32 symbols in CSR form (sym, off
// [R+1]), grp [G+1] row offsets of the groups; out int32 [cells, n_max, 3], cells = sum n_g^2, every cell equal to what
// gtos_ngram_overlap stores for that (hypothesis row, reference row).
//
// One 256-thread workgroup per candidate row (grid R).  THE GROUP IS FOUND BY THE WORKGROUP from the device copy of grp: its threads
// walk the G groups once, strided, and that one pass gives the group that holds the row, the cells in front of it (the sum of n^2
// over the groups before: where the group's block of the output starts) and the total, which must equal the host's.  No per-row
// index and no pair list travel to the device.
//
// The workgroup then
//   1. stages its own row in LDS once (h), and the first reference of its half circle (r[0]);
//   2. computes earlier[] of its positions once -- position p = tid + 256 q, q < 4 -- packed 10 bits per order into 3 registers
//      per position (mbr_kernels.h: a row holds at most 1024 symbols);
//   3. per reference k of the half circle: inref_counts against r[k & 1], the decision earlier < inref, a reduction as in
//      ngram_overlap_kernel (shuffles inside a wave, a [4][8] table across the waves), and one store of the two mirrored cells;
//   4. stores its diagonal cell without a scan.
// LDS reads are those of ngram_overlap_kernel: lane l of a wave reads h[p + l + c], 32 consecutive words per half wave on the 32
// banks of a ds_read_b32, and every lane the same reference word, a broadcast: no bank conflicts on either side.
//
// The next reference is prefetched: its symbols are loaded into registers before the scan of reference k and written to r[(k+1)&1]
// after it, so the global latency hides under the scan and one barrier per reference remains.  Race reasoning, with B(k) the
// barrier at the end of iteration k and B(-1) the one after the first staging:
//   r[b], b = k & 1, is read by the scan of iteration k and written in iteration k - 1 (before B(k-1): visible) and again in
//     iteration k + 1, after B(k), which every thread passes only once its own scan of iteration k is over.
//   part[b] is written by the wave leaders in iteration k before B(k), read by the storing threads after B(k), and written again in
//     iteration k + 2, after B(k+1), which the storing threads reach only after their reads of iteration k.
// Integer arithmetic throughout, every ordered cell has one owner (mbr_kernels.h), no atomics: two launches store identical values.
// Nothing here synchronises with the host.
#include "common.h"
#include "mbr_kernels.h"

using namespace gtos_mbr;

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;
constexpr int SLOTS = GROUP_MAX_SYMBOLS / NT;       // positions a thread owns: 4
static_assert(GROUP_MAX_SYMBOLS % NT == 0 && GROUP_MAX_SYMBOLS <= 1024 && MAX_ORDER <= 9, "earlier[] packs 10 bits x 3 per register");
static_assert(MAX_GROUP + 1 <= NT && 2 * MAX_ORDER * STATS <= NT, "one thread per group row offset / per stored integer");

struct GroupArgs {
    const int* sym;                     // the symbols of all rows
    const int* off;                     // [R + 1]
    const int* grp;                     // [G + 1]
    int R, G, n_max;
    int n_sym;                          // off_host[R]: no row may end behind it
    int cells;                          // sum n_g^2 of the host copy
    int* out;                           // [cells, n_max, 3]
};

__device__ __forceinline__ int block_sum(int v, int (&table)[WAVES], int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) table[tid >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += table[w];
    return s;
}

__global__ __launch_bounds__(NT) void ngram_overlap_groups_kernel(GroupArgs a) {
    __shared__ int h[GROUP_MAX_SYMBOLS];
    __shared__ int r[2][GROUP_MAX_SYMBOLS];
    __shared__ int part[2][WAVES][MAX_ORDER];
    __shared__ int goff[MAX_GROUP + 1];
    __shared__ int sum_before[WAVES], sum_all[WAVES];
    __shared__ int found[4];                                    // group, bad flag, its first row, its size
    const int row = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { found[0] = -1; found[1] = 0; }
    __syncthreads();
    // ---- the group of this row.  The entry point has checked the host copy of grp; the device copy is checked again here (every
    // thread that finds a fault stores the same 1), and a copy that is no grouping of R rows into the host's number of cells stores
    // nothing.  cells <= MAX_OUT / 3 on the host and n <= 64 here: a partial sum of a VALID copy fits an int; an invalid one's
    // may wrap, and is then refused by its flag.
    int before = 0, all = 0;
    for (int g = tid; g < a.G; g += NT) {
        const int lo = a.grp[g], hi = a.grp[g + 1], n = hi - lo;
        if (lo < 0 || hi > a.R || n < 0 || n > MAX_GROUP || (g == 0 && lo != 0) || (g == a.G - 1 && hi != a.R)) { found[1] = 1; continue; }
        all += n * n;
        if (hi <= row) before += n * n;
        else if (lo <= row) { found[0] = g; found[2] = lo; found[3] = n; }
    }
    before = block_sum(before, sum_before, tid);
    all = block_sum(all, sum_all, tid);
    if (found[1] || found[0] < 0 || all != a.cells) return;    // (uniform: every thread reads the same words after a barrier)
    const int g0 = found[2], n = found[3], i = row - g0;
    // ---- the row offsets of the group, checked like grp
    if (tid <= n) goff[tid] = a.off[g0 + tid];
    __syncthreads();
    if (tid < n) {
        const int s = goff[tid], L = goff[tid + 1] - s;
        if (s < 0 || L < 0 || L > GROUP_MAX_SYMBOLS || s > a.n_sym - L) found[1] = 1;
    }
    __syncthreads();
    if (found[1]) return;
    const int h0 = goff[i], Lh = goff[i + 1] - h0;
    const int count = scan_count(i, n);
    // ---- 1. the own row, and the first reference
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int p = tid + q * NT;
        if (p < Lh) h[p] = a.sym[h0 + p];
    }
    if (count > 0) {
        const int j = scan_ref(i, n, 0), r0 = goff[j], Lr = goff[j + 1] - r0;
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) {
            const int p = tid + q * NT;
            if (p < Lr) r[0][p] = a.sym[r0 + p];
        }
    }
    __syncthreads();                                            // B(-1)
    // ---- 2. earlier[] of the own positions, once
    unsigned packed[SLOTS][3];
#pragma unroll
    for (int q = 0; q < SLOTS; ++q) {
        const int p = tid + q * NT;
        packed[q][0] = packed[q][1] = packed[q][2] = 0u;
        if (p < Lh) {
            int e[MAX_ORDER];
            earlier_counts(h, Lh, a.n_max, p, e);
#pragma unroll
            for (int m = 0; m < MAX_ORDER; ++m) packed[q][m / 3] |= (unsigned)e[m] << (10 * (m % 3));
        }
    }
    const int W = a.n_max * STATS;
    int* const block = a.out + before * W;                      // (before + n * n) * W <= cells * W <= MAX_OUT
    // ---- 4. the diagonal: every n-gram of a row matches itself
    if (tid < W) block[(i * n + i) * W + tid] = n_grams(Lh, tid / STATS + 1);
    // ---- 3. the half circle
    for (int k = 0; k < count; ++k) {
        const int b = k & 1;
        const int j = scan_ref(i, n, k), Lr = goff[j + 1] - goff[j];
        int next[SLOTS], Ln = 0;
        if (k + 1 < count) {
            const int jn = scan_ref(i, n, k + 1), rn = goff[jn];
            Ln = goff[jn + 1] - rn;
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                const int p = tid + q * NT;
                next[q] = p < Ln ? a.sym[rn + p] : 0;
            }
        }
        int total[MAX_ORDER];
#pragma unroll
        for (int m = 0; m < MAX_ORDER; ++m) total[m] = 0;
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) {
            const int p = tid + q * NT;
            if (p < Lh) {
                int e[MAX_ORDER], in[MAX_ORDER], counts[MAX_ORDER];
#pragma unroll
                for (int m = 0; m < MAX_ORDER; ++m) e[m] = (int)((packed[q][m / 3] >> (10 * (m % 3))) & 1023u);
                inref_counts(h, Lh, r[b], Lr, a.n_max, p, in);
                position_matches(Lh, a.n_max, p, e, in, counts);
#pragma unroll
                for (int m = 0; m < MAX_ORDER; ++m) total[m] += counts[m];
            }
        }
#pragma unroll
        for (int m = 0; m < MAX_ORDER; ++m) {
            int v = total[m];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((tid & 63) == 0) part[b][tid >> 6][m] = v;
        }
        if (k + 1 < count) {
#pragma unroll
            for (int q = 0; q < SLOTS; ++q) {
                const int p = tid + q * NT;
                if (p < Ln) r[b ^ 1][p] = next[q];
            }
        }
        __syncthreads();                                        // B(k)
        if (tid < 2 * W) {
            const int mirror = tid >= W, t = mirror ? tid - W : tid, m = t / STATS, s = t % STATS;
            int v;
            if (s == 0) {
                v = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) v += part[b][w][m];
            } else {
                v = n_grams((s == 1) != mirror ? Lh : Lr, m + 1);
            }
            block[(mirror ? j * n + i : i * n + j) * W + t] = v;
        }
    }
}

}  // namespace

extern "C" int gtos_ngram_overlap_groups(const int* sym, const int* off, int R, const int* grp, int G, int n_max, const int* off_host,
                                         const int* grp_host, int* out, void* stream) {
    if (R < 0 || G < 0 || !off_host || !grp_host) return -10;
    if (check_groups(off_host, R, grp_host, G, n_max)) return -10;
    if (G == 0 || R == 0) return 0;
    if (!off || !grp || !out || (!sym && off_host[R] > 0)) return -10;
    int64_t cells = 0;
    for (int g = 0; g < G; ++g) cells += (int64_t)(grp_host[g + 1] - grp_host[g]) * (grp_host[g + 1] - grp_host[g]);
    GroupArgs a{};
    a.sym = sym; a.off = off; a.grp = grp; a.R = R; a.G = G; a.n_max = n_max; a.n_sym = off_host[R]; a.cells = (int)cells; a.out = out;
    hipLaunchKernelGGL(ngram_overlap_groups_kernel, dim3((unsigned)R), dim3(NT), 0, static_cast<hipStream_t>(stream), a);
    GTOS_CHECK_LAUNCH();
    return 0;
}
