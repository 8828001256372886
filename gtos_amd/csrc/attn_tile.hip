// Relation-free (mode 0) bf16 multi-head attention on MFMA tiles for gfx950: forward and backward of
// MultiheadAttention.forward (the reference's generator/transformer.py:120-162) for the decoder's self- and cross-attention.
//
// rel_attn.hip gives one workgroup a (query, graph) row and streams every key row past it: the right shape when each pair carries
// its own 2d-wide relation row, but with no relation operand every query workgroup only re-reads the same K/V panel from L2
// (T*B*S*2 KB of L2 traffic for a problem of a few MB) and no MFMA is involved.  Here a workgroup owns 64 rows of ONE head of ONE
// graph and the other axis comes through LDS once per workgroup:
//
//   forward     one workgroup per (graph b, head h, 64 queries); K row-major and V transposed in LDS, NT keys at a time
//   backward    ONE launch, two kinds of workgroup: (b, h, 64 keys) accumulates dK, dV over all query tiles, (b, h, 64 queries)
//               accumulates dQ over all key tiles.  Both recompute P from lse and dS from dO, V, O (the flops are free at these sizes);
//               nothing goes through global scratch and there are no atomics.
//
// Lane map (v_mfma_f32_16x16x32_bf16; A: lane l holds A[l&15][8(l>>4)+0..7], B likewise, D: lane l holds D[4(l>>4)+0..3][l&15]).
// A wave owns 16 "own" rows x (queries in the forward and the query-major backward, keys in the key-major backward); its 16-byte
// operand fragments come straight from global memory, once.  A score block is computed TRANSPOSED, D[streamed row][own row], and the
// 16 MFMA rows of block (kb, t) are the streamed rows kb*32 + (r>>2)*8 + t*4 + (r&3): lane (n = l&15, g = l>>4) then holds, for ITS
// own row n, the 8 consecutive streamed rows kb*32 + 8g .. 8g+7 in the registers of the two blocks t = 0, 1 -- exactly the B-operand
// fragment of the second product (contraction over the streamed rows), so P and dS never move between lanes.  The second product is
// transposed too, D[channel][own row] = Yt[channel][streamed] * P[streamed][own], with Yt the streamed operand stored TRANSPOSED in
// LDS: its fragment is one 16-byte read, and a lane ends up with 4 consecutive channels of its own row (8-byte stores).
// Row statistics (running max / sum, lse, delta) are per own row = per lane n, replicated over the four g.
//
// Precision: scores, softmax, lse and every accumulator are fp32.  P~ and dS are fp32 values that the second product takes as bf16:
// each is split into hi + lo bf16 and multiplied by two MFMAs, which keeps ~16 mantissa bits, so the results carry the rounding of the
// bf16 outputs only, like the streaming kernels.  Dropout uses the streaming kernels' counter, drop_keep(seed, ((i*S+j)*B+b)*H+h, p)
// after live_seed: a forward on one path and a backward on the other see one mask.
//
// LDS: row-major tiles have 16 bytes of padding per row; transposed tiles XOR the 8-row chunk index with the channel's chunk index
// (by the bank arithmetic conflict-free 2-byte transposing writes at hd = 64, 2-way otherwise -- not measured; fragment reads stay
// 16-byte aligned).
#include "common.h"
#include "attn_tile.h"
#include <cstdlib>
#include <type_traits>

namespace {

constexpr int OWN = 64;     // own rows per workgroup: 16 per wave

template <int HD> struct Cfg {
    static constexpr int NT = HD == 128 ? 32 : 64;   // streamed rows per LDS tile
    static constexpr int RS = HD + 8;                // row-major row stride in elements (16 B of padding)
    static constexpr int CH = HD / 8;                // 16-byte chunks per row
    static constexpr int KC = HD / 32;               // k steps of the score product
    static constexpr int CB = HD / 16;               // 16-channel blocks of the second product
    static constexpr int NB = NT / 32;               // 32-row blocks of a tile
    static constexpr int DS = NT + 4;                // row stride of the dead-pair bytes
};

// block -> (graph, head, tile): the graph -> XCD map of rel_attn.hip (blocks are dealt to the 8 XCDs round-robin), so a graph's
// panels stay in one private L2
__device__ __forceinline__ void map_block(int B, int H, int& b, int& h, int& tile) {
    const int blk = blockIdx.x;
    int rest;
    if ((B & 7) == 0) { const int x = blk & 7, w = blk >> 3, gpx = B >> 3; b = x * gpx + (w % gpx); rest = w / gpx; }
    else { b = blk % B; rest = blk / B; }
    h = rest % H; tile = rest / H;
}

__device__ __forceinline__ f32x4_t mfma(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// NT rows [r0, r0+NT) of one head slice (base already at graph b, head h; row stride rstride elements) -> LDS, row-major and / or
// transposed; rows past nrows are zero
template <int HD, bool RM, bool TR>
__device__ __forceinline__ void stage(const bf16_t* __restrict__ base, int64_t rstride, int r0, int nrows, bf16_t* rm, bf16_t* tr) {
    using C = Cfg<HD>;
    constexpr int IT = C::NT * C::CH / 256;
    uint4 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = it * 256 + threadIdx.x, y = idx / C::CH, c = idx % C::CH;
        v[it] = make_uint4(0, 0, 0, 0);
        if (r0 + y < nrows) v[it] = *reinterpret_cast<const uint4*>(base + (int64_t)(r0 + y) * rstride + c * 8);
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = it * 256 + threadIdx.x, y = idx / C::CH, c = idx % C::CH;
        if (RM) *reinterpret_cast<uint4*>(rm + y * C::RS + c * 8) = v[it];
        if (TR) {
            const int yc = (((y >> 3) ^ (c & (C::NT / 8 - 1))) << 3) | (y & 7);
            const uint32_t ww[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) tr[(c * 8 + e) * C::NT + yc] = (bf16_t)(ww[e >> 1] >> ((e & 1) * 16));
        }
    }
}

// A operand of a score block: streamed rows kb*32 + (r>>2)*8 + t*4 + (r&3), channels kc*32 + 8g .. +7
template <int HD> __device__ __forceinline__ bf16x8_t frag_rows(const bf16_t* rm, int kb, int t, int kc, int lane) {
    const int r = lane & 15, row = kb * 32 + (r >> 2) * 8 + t * 4 + (r & 3);
    return *reinterpret_cast<const bf16x8_t*>(rm + row * Cfg<HD>::RS + kc * 32 + (lane >> 4) * 8);
}
// A operand of the second product: channel cb*16 + n, streamed rows kb*32 + 8g .. +7
template <int HD> __device__ __forceinline__ bf16x8_t frag_tr(const bf16_t* tr, int cb, int kb, int lane) {
    constexpr int NT = Cfg<HD>::NT;
    const int cc = cb * 16 + (lane & 15), chunk = (kb * 4 + (lane >> 4)) ^ ((cc >> 3) & (NT / 8 - 1));
    return *reinterpret_cast<const bf16x8_t*>(tr + cc * NT + chunk * 8);
}
// own-row operand: row x of a [rows,B,ld] buffer, channels kc*32 + 8g .. +7, straight from global memory
template <int HD> __device__ __forceinline__ void load_own(const bf16_t* __restrict__ base, int64_t rstride, int x, bool valid, int lane,
                                                            bf16x8_t (&f)[Cfg<HD>::KC]) {
#pragma unroll
    for (int kc = 0; kc < Cfg<HD>::KC; ++kc) {
        U128 v = {0, 0, 0, 0};
        if (valid) v = *reinterpret_cast<const U128*>(base + (int64_t)x * rstride + kc * 32 + (lane >> 4) * 8);
        f[kc] = __builtin_bit_cast(bf16x8_t, v);
    }
}
// 8 fp32 -> hi + lo bf16 fragments (hi = rn(p), lo = rn(p - hi))
__device__ __forceinline__ void split8(const float (&p)[8], bf16x8_t& hi, bf16x8_t& lo) {
    uint32_t hw[4], lw[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hw[e] = pack_bf(p[2 * e], p[2 * e + 1]);
        lw[e] = pack_bf(p[2 * e] - lo_bf(hw[e]), p[2 * e + 1] - hi_bf(hw[e]));
    }
    const U128 a = {hw[0], hw[1], hw[2], hw[3]}, b = {lw[0], lw[1], lw[2], lw[3]};
    hi = __builtin_bit_cast(bf16x8_t, a); lo = __builtin_bit_cast(bf16x8_t, b);
}
// 4 fp32 -> 4 bf16, one 8-byte store
__device__ __forceinline__ void store4(bf16_t* p, const f32x4_t& v, float s) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf(v[0] * s, v[1] * s), pack_bf(v[2] * s, v[3] * s));
}

// dead[own][streamed] bytes of one tile pair: key padding, attention mask, rows past T / S (key_dead of rel_attn.hip plus the tile edges).
// KM: the own rows are keys, the streamed rows queries.
template <int HD, bool KM>
__device__ __forceinline__ void fill_dead(const AttnTileArgs& a, int b, int x0, int y0, unsigned char* sdead) {
    using C = Cfg<HD>;
    // (clamped, unconditional byte loads in a fully unrolled loop: all of a thread's loads are in flight together)
#pragma unroll
    for (int it = 0; it < OWN * C::NT / 256; ++it) {
        const int idx = it * 256 + threadIdx.x, xo = idx / C::NT, ys = idx % C::NT;
        const int i = KM ? y0 + ys : x0 + xo, j = KM ? x0 + xo : y0 + ys;
        const int ic = min(i, a.T - 1), jc = min(j, a.S - 1);
        const unsigned char kp = a.key_pad ? a.key_pad[(int64_t)jc * a.B + b] : 0;
        const unsigned char am = a.attn_mask ? a.attn_mask[(int64_t)ic * a.S + jc] : 0;
        sdead[xo * C::DS + ys] = (i >= a.T || j >= a.S || kp != 0 || am != 0) ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------- forward
template <int HD>
__global__ __launch_bounds__(256) void attn_tile_fwd_kernel(AttnTileArgs a) {
    using C = Cfg<HD>;
    if (a.p_drop > 0.f) a.seed = live_seed(a.seed);
    __shared__ __attribute__((aligned(16))) bf16_t sK[C::NT * C::RS];
    __shared__ __attribute__((aligned(16))) bf16_t sVt[HD * C::NT];
    __shared__ __attribute__((aligned(16))) unsigned char sdead[OWN * C::DS];
    int b, h, qt;
    map_block(a.B, a.H, b, h, qt);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int i0 = qt * OWN, xo = wv * 16 + n, i = i0 + xo;
    const bool iv = i < a.T;
    const int64_t hb = (int64_t)h * HD;
    const bf16_t* qb = static_cast<const bf16_t*>(a.q) + (int64_t)b * a.ldq + hb;
    const bf16_t* kb_ = static_cast<const bf16_t*>(a.k) + (int64_t)b * a.ldk + hb;
    const bf16_t* vb = static_cast<const bf16_t*>(a.v) + (int64_t)b * a.ldv + hb;
    const int64_t rsq = (int64_t)a.B * a.ldq, rsk = (int64_t)a.B * a.ldk, rsv = (int64_t)a.B * a.ldv;
    const float keep_scale = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;

    bf16x8_t xq[C::KC];
    load_own<HD>(qb, rsq, i, iv, lane, xq);
    float m = -INFINITY, l = 0.f;
    f32x4_t oacc[C::CB];
#pragma unroll
    for (int cb = 0; cb < C::CB; ++cb) oacc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < a.S; j0 += C::NT) {
        __syncthreads();                                   // the previous tile's readers are done
        stage<HD, true, false>(kb_, rsk, j0, a.S, sK, nullptr);
        stage<HD, false, true>(vb, rsv, j0, a.S, nullptr, sVt);
        fill_dead<HD, false>(a, b, i0, j0, sdead);
        __syncthreads();
        float s[C::NB][8];
        float mt = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < C::NB; ++kb) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                // one MFMA per 32-channel step into a ZERO accumulator, the steps added on the VALU: chaining the steps through the MFMA's
                // C operand cost the returned fp32 weights a rounding per step (largest error against fp64 2.0 x the streaming kernels' at
                // hd = 128, 1.1-1.2 x at hd = 64, 1.06 x at hd = 32 where there is one step)
                f32x4_t part[C::KC];
#pragma unroll
                for (int kc = 0; kc < C::KC; ++kc) part[kc] = mfma(frag_rows<HD>(sK, kb, t, kc, lane), xq[kc], f32x4_t{0.f, 0.f, 0.f, 0.f});
                f32x4_t acc = part[0];
                if (C::KC == 2) acc = part[0] + part[1];
                if (C::KC == 4) acc = (part[0] + part[1]) + (part[2] + part[3]);
                const uint32_t dd = *reinterpret_cast<const uint32_t*>(sdead + xo * C::DS + kb * 32 + g * 8 + t * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool dead = ((dd >> (8 * e)) & 0xff) != 0;
                    const float sv = dead ? -INFINITY : acc[e] * a.scale;
                    s[kb][t * 4 + e] = sv;
                    mt = fmaxf(mt, sv);
                    const int j = j0 + kb * 32 + g * 8 + t * 4 + e;
                    if (a.w && iv && j < a.S) a.w[(((int64_t)i * a.S + j) * a.B + b) * a.H + h] = sv;      // raw score; normalised below
                }
            }
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        float alpha = 1.f, lsum = 0.f;
        if (mn != -INFINITY) alpha = __expf(m - mn);
#pragma unroll
        for (int kb = 0; kb < C::NB; ++kb) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float sv = s[kb][e];
                float pe = 0.f;
                if (mn != -INFINITY) pe = __expf(sv - mn);
                lsum += pe;
                if (a.p_drop > 0.f && sv != -INFINITY) {
                    const int j = j0 + kb * 32 + g * 8 + e;
                    pe = drop_keep(a.seed, (((uint64_t)i * a.S + j) * a.B + b) * a.H + h, a.p_drop) ? pe * keep_scale : 0.f;
                }
                s[kb][e] = pe;
            }
        }
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        l = l * alpha + lsum;
        m = mn;
#pragma unroll
        for (int cb = 0; cb < C::CB; ++cb) oacc[cb] *= alpha;
#pragma unroll
        for (int kb = 0; kb < C::NB; ++kb) {
            bf16x8_t ph, pl;
            split8(s[kb], ph, pl);
#pragma unroll
            for (int cb = 0; cb < C::CB; ++cb) {
                const bf16x8_t vt = frag_tr<HD>(sVt, cb, kb, lane);
                oacc[cb] = mfma(vt, ph, oacc[cb]);
                oacc[cb] = mfma(vt, pl, oacc[cb]);
            }
        }
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
    if (iv) {
        bf16_t* op = static_cast<bf16_t*>(a.o) + ((int64_t)i * a.B + b) * a.ldo + hb + g * 4;
#pragma unroll
        for (int cb = 0; cb < C::CB; ++cb) store4(op + cb * 16, oacc[cb], inv);
        if (g == 0) a.lse[((int64_t)i * a.B + b) * a.H + h] = (l > 0.f) ? m + __logf(l) : -INFINITY;
    }
    if (a.w && iv) {                                       // normalise the raw scores this same lane wrote above
        for (int jb = g * 8; jb < a.S; jb += 32) {
            for (int e = 0; e < 8 && jb + e < a.S; ++e) {
                const int64_t off = (((int64_t)i * a.S + jb + e) * a.B + b) * a.H + h;
                const float sv = a.w[off];
                float p = (sv == -INFINITY || inv <= 0.f) ? 0.f : __expf(sv - m) * inv;
                if (a.p_drop > 0.f && p > 0.f) p = drop_keep(a.seed, (uint64_t)off, a.p_drop) ? p * keep_scale : 0.f;
                a.w[off] = p;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- backward
// lse and delta = rowsum(dO * O) (+ sum_j w * dw when the weights carry a gradient) of `cnt` query rows from i0 -> LDS; 4 threads per row
template <int HD>
__device__ __forceinline__ void row_stats(const AttnTileArgs& a, int b, int h, int i0, int cnt, float* sLse, float* sD) {
    const int row = threadIdx.x >> 2, part = threadIdx.x & 3, i = i0 + row;
    const bool valid = row < cnt && i < a.T;
    float acc = 0.f;
    if (valid) {
        const int64_t hb = (int64_t)h * HD + part * (HD / 4);
        const bf16_t* dop = static_cast<const bf16_t*>(a.d_o) + ((int64_t)i * a.B + b) * a.lddo + hb;
        const bf16_t* op = static_cast<const bf16_t*>(a.o) + ((int64_t)i * a.B + b) * a.ldo + hb;
#pragma unroll
        for (int c = 0; c < HD / 32; ++c) {
            float x[8], y[8];
            Vec8<bf16_t>::load(dop + c * 8, x);
            Vec8<bf16_t>::load(op + c * 8, y);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(x[e], y[e], acc);
        }
        if (a.dw) {
            for (int j = part; j < a.S; j += 4) {
                const int64_t off = (((int64_t)i * a.S + j) * a.B + b) * a.H + h;
                acc = fmaf(a.w[off], a.dw[off], acc);
            }
        }
    }
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    if (part == 0 && row < cnt) {
        sD[row] = acc;
        sLse[row] = valid ? a.lse[((int64_t)i * a.B + b) * a.H + h] : -INFINITY;
    }
}

struct BwdSmem { bf16_t *y1, *y2, *y1t, *y2t; unsigned char* dead; float *lse, *dl; };

// KM: own rows are keys (dK, dV over all queries); else own rows are queries (dQ over all keys)
template <int HD, bool KM>
__device__ __forceinline__ void bwd_body(const AttnTileArgs& a, int b, int h, int tile, const BwdSmem& sm) {
    using C = Cfg<HD>;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int nX = KM ? a.S : a.T, nY = KM ? a.T : a.S;
    const int x0 = tile * OWN, xo = wv * 16 + n, x = x0 + xo;
    const bool xv = x < nX;
    const int64_t hb = (int64_t)h * HD;
    const bf16_t* qb = static_cast<const bf16_t*>(a.q) + (int64_t)b * a.ldq + hb;
    const bf16_t* kb_ = static_cast<const bf16_t*>(a.k) + (int64_t)b * a.ldk + hb;
    const bf16_t* vb = static_cast<const bf16_t*>(a.v) + (int64_t)b * a.ldv + hb;
    const bf16_t* dob = static_cast<const bf16_t*>(a.d_o) + (int64_t)b * a.lddo + hb;
    const int64_t rsq = (int64_t)a.B * a.ldq, rsk = (int64_t)a.B * a.ldk, rsv = (int64_t)a.B * a.ldv, rsdo = (int64_t)a.B * a.lddo;
    const float keep_scale = a.p_drop > 0.f ? 1.f / (1.f - a.p_drop) : 1.f;

    bf16x8_t x1[C::KC], x2[C::KC];                         // own operands of the score and the dP products
    if (KM) { load_own<HD>(kb_, rsk, x, xv, lane, x1); load_own<HD>(vb, rsv, x, xv, lane, x2); }
    else { load_own<HD>(qb, rsq, x, xv, lane, x1); load_own<HD>(dob, rsdo, x, xv, lane, x2); }
    f32x4_t acc1[C::CB], acc2[KM ? C::CB : 1];             // dK (or dQ), dV
#pragma unroll
    for (int cb = 0; cb < C::CB; ++cb) { acc1[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; if (KM) acc2[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    float lse_own = -INFINITY, d_own = 0.f;
    if (!KM) {
        row_stats<HD>(a, b, h, x0, OWN, sm.lse, sm.dl);
        __syncthreads();
        lse_own = sm.lse[xo]; d_own = sm.dl[xo];
    }
    for (int y0 = 0; y0 < nY; y0 += C::NT) {
        __syncthreads();                                   // the previous tile's readers are done
        if (KM) {
            stage<HD, true, true>(qb, rsq, y0, a.T, sm.y1, sm.y1t);
            stage<HD, true, true>(dob, rsdo, y0, a.T, sm.y2, sm.y2t);
            row_stats<HD>(a, b, h, y0, C::NT, sm.lse, sm.dl);
        } else {
            stage<HD, true, true>(kb_, rsk, y0, a.S, sm.y1, sm.y1t);
            stage<HD, true, false>(vb, rsv, y0, a.S, sm.y2, nullptr);
        }
        fill_dead<HD, KM>(a, b, x0, y0, sm.dead);
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < C::NB; ++kb) {
            float pd[8], gs[8];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                f32x4_t sa = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < C::KC; ++kc) {
                    sa = mfma(frag_rows<HD>(sm.y1, kb, t, kc, lane), x1[kc], sa);
                    da = mfma(frag_rows<HD>(sm.y2, kb, t, kc, lane), x2[kc], da);
                }
                const int ys = kb * 32 + g * 8 + t * 4;
                const uint32_t dd = *reinterpret_cast<const uint32_t*>(sm.dead + xo * C::DS + ys);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int y = y0 + ys + e;
                    const int i = KM ? y : x, j = KM ? x : y;
                    const float lse = KM ? sm.lse[ys + e] : lse_own, dl = KM ? sm.dl[ys + e] : d_own;
                    const bool dead = ((dd >> (8 * e)) & 0xff) != 0 || lse == -INFINITY;
                    const float p = dead ? 0.f : __expf(sa[e] * a.scale - lse);
                    const bool inr = i < a.T && j < a.S;
                    const int64_t off = (((int64_t)i * a.S + j) * a.B + b) * a.H + h;
                    float keep = 1.f;
                    if (a.p_drop > 0.f) keep = drop_keep(a.seed, (uint64_t)off, a.p_drop) ? keep_scale : 0.f;
                    float dp = da[e];
                    if (a.dw && inr) dp += a.dw[off];
                    pd[t * 4 + e] = p * keep;
                    gs[t * 4 + e] = a.scale * p * (keep * dp - dl);
                }
            }
            bf16x8_t gh, gl;
            split8(gs, gh, gl);
#pragma unroll
            for (int cb = 0; cb < C::CB; ++cb) {
                const bf16x8_t yt = frag_tr<HD>(sm.y1t, cb, kb, lane);
                acc1[cb] = mfma(yt, gh, acc1[cb]);
                acc1[cb] = mfma(yt, gl, acc1[cb]);
            }
            if (KM) {
                bf16x8_t ph, pl;
                split8(pd, ph, pl);
#pragma unroll
                for (int cb = 0; cb < C::CB; ++cb) {
                    const bf16x8_t yt = frag_tr<HD>(sm.y2t, cb, kb, lane);
                    acc2[cb] = mfma(yt, ph, acc2[cb]);
                    acc2[cb] = mfma(yt, pl, acc2[cb]);
                }
            }
        }
    }
    if (xv) {
        if (KM) {
            bf16_t* dkp = static_cast<bf16_t*>(a.dk) + ((int64_t)x * a.B + b) * a.lddk + hb + g * 4;
            bf16_t* dvp = static_cast<bf16_t*>(a.dv) + ((int64_t)x * a.B + b) * a.lddv + hb + g * 4;
#pragma unroll
            for (int cb = 0; cb < C::CB; ++cb) { store4(dkp + cb * 16, acc1[cb], 1.f); store4(dvp + cb * 16, acc2[cb], 1.f); }
        } else {
            bf16_t* dqp = static_cast<bf16_t*>(a.dq) + ((int64_t)x * a.B + b) * a.lddq + hb + g * 4;
#pragma unroll
            for (int cb = 0; cb < C::CB; ++cb) store4(dqp + cb * 16, acc1[cb], 1.f);
        }
    }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_tile_bwd_kernel(AttnTileArgs a, int nkt) {
    using C = Cfg<HD>;
    if (a.p_drop > 0.f) a.seed = live_seed(a.seed);
    __shared__ __attribute__((aligned(16))) bf16_t sY1[C::NT * C::RS];
    __shared__ __attribute__((aligned(16))) bf16_t sY2[C::NT * C::RS];
    __shared__ __attribute__((aligned(16))) bf16_t sY1t[HD * C::NT];
    __shared__ __attribute__((aligned(16))) bf16_t sY2t[HD * C::NT];
    __shared__ __attribute__((aligned(16))) unsigned char sdead[OWN * C::DS];
    __shared__ __attribute__((aligned(16))) float sLse[OWN];
    __shared__ __attribute__((aligned(16))) float sDl[OWN];
    const BwdSmem sm = {sY1, sY2, sY1t, sY2t, sdead, sLse, sDl};
    int b, h, tile;
    map_block(a.B, a.H, b, h, tile);
    if (tile < nkt) bwd_body<HD, true>(a, b, h, tile, sm);              // the key-major workgroups (the longer ones) first
    else bwd_body<HD, false>(a, b, h, tile - nkt, sm);
}

bool aligned(const void* p, int n) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(n - 1)) == 0; }

template <typename K> int dispatch_hd(int hd, K&& f) {
    switch (hd) {
        case 32: return f(std::integral_constant<int, 32>());
        case 64: return f(std::integral_constant<int, 64>());
        case 128: return f(std::integral_constant<int, 128>());
    }
    return -11;
}

}  // namespace

bool gtosi_attn_tile_covers(int T_, int S, int B, int H, int d, const AttnTileArgs& a, bool backward) {
    const char* sw = getenv("GTOS_ATTN_TILE");             // read per call: the tests flip it inside one process
    if (sw && sw[0] == '0') return false;
    if (T_ < 16 || S < 1 || B < 1 || H < 1 || d > 512 || (d & (d - 1)) || d % H) return false;
    const int hd = d / H;
    if (hd != 32 && hd != 64 && hd != 128) return false;
    if (a.ldq % 8 || a.ldk % 8 || a.ldv % 8 || a.ldo % 4 || !aligned(a.q, 16) || !aligned(a.k, 16) || !aligned(a.v, 16) || !aligned(a.o, 16))
        return false;
    if (backward && (a.lddo % 8 || a.ldo % 8 || a.lddq % 4 || a.lddk % 4 || a.lddv % 4 || !aligned(a.d_o, 16) || !aligned(a.dq, 8) ||
                     !aligned(a.dk, 8) || !aligned(a.dv, 8)))
        return false;
    return true;
}

int gtosi_attn_tile_fwd(const AttnTileArgs& a, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nqt = (a.T + OWN - 1) / OWN;
    const dim3 grid(a.B * a.H * nqt);
    return dispatch_hd(a.d / a.H, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        hipLaunchKernelGGL((attn_tile_fwd_kernel<HD>), grid, dim3(256), 0, s, a);
        GTOS_CHECK_LAUNCH();
        return 0;
    });
}

int gtosi_attn_tile_bwd(const AttnTileArgs& a, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nqt = (a.T + OWN - 1) / OWN, nkt = (a.S + OWN - 1) / OWN;
    const dim3 grid(a.B * a.H * (nqt + nkt));
    return dispatch_hd(a.d / a.H, [&](auto hd) {
        constexpr int HD = decltype(hd)::value;
        hipLaunchKernelGGL((attn_tile_bwd_kernel<HD>), grid, dim3(256), 0, s, a, nkt);
        GTOS_CHECK_LAUNCH();
        return 0;
    });
}

GTOS_SEED_EPOCH_SETTER(attn_tile)
