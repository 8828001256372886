// Relation-free (mode 0) bf16 attention on MFMA tiles: the interface between the dispatch in rel_attn.hip and attn_tile.hip.
#pragma once
#include <stdint.h>

struct AttnTileArgs {
    const void *q, *k, *v; int64_t ldq, ldk, ldv;          // rows (t*B+b)*ld, element units
    const uint8_t* key_pad;     // [S,B] or null
    const uint8_t* attn_mask;   // [T,S] or null
    void* o; int64_t ldo;       // fwd out / bwd in [T,B,d]
    float* lse;                 // [T,B,H]
    float* w;                   // optional [T,S,B,H] post-dropout weights (fwd out; bwd in when dw given)
    const void* d_o; int64_t lddo;
    const float* dw;            // optional upstream grad on w, [T,S,B,H]
    void *dq, *dk, *dv; int64_t lddq, lddk, lddv;
    int T, S, B, H, d;
    float scale, p_drop; uint64_t seed;
};

// Shapes the tile kernels cover (bf16, mode 0 only; the caller checks those two): the power-of-two lane geometry of the streaming fast
// path, a head of 32, 64 or 128 channels, at least one MFMA tile of queries, 16-byte aligned rows.  GTOS_ATTN_TILE=0 sends everything
// back to the streaming kernels.
bool gtosi_attn_tile_covers(int T, int S, int B, int H, int d, const AttnTileArgs& a, bool backward);
int gtosi_attn_tile_fwd(const AttnTileArgs& a, void* stream);
int gtosi_attn_tile_bwd(const AttnTileArgs& a, void* stream);
