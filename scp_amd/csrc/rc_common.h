// Shared pieces of the row-chain kernels (rowchain.hip, lnlin2.hip): vector types, the hi / lo split of fp32 values, the lane geometry of a
// 128-row tile, the full-line row store through a wave's bounce buffer, LayerNorm statistics and the argument block of the LayerNorm + linear
// kernels.  Both files must produce the same bits from these, so there is one copy.
#pragma once
#include "scp_internal.h"

typedef __bf16 rbf16x8 __attribute__((ext_vector_type(8)));
typedef float rf32x16 __attribute__((ext_vector_type(16)));
typedef float rf32x4 __attribute__((ext_vector_type(4)));
typedef int ri32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void *rc_lds_ptr_t;
typedef const __attribute__((address_space(1))) void *rc_glb_ptr_t;

#define RC_ROWS 128                 // rows per workgroup tile
#define RC_BOUNCE 4096              // per wave: 32 rows x 32 channels fp32

__device__ __forceinline__ void rc_dma16(const void *g, char *l) {
    __builtin_amdgcn_global_load_lds((rc_glb_ptr_t)g, (rc_lds_ptr_t)l, 16, 0, 0);
}

// hi/lo split of fp32 values (the arithmetic of every producer of split operands: hi = bf16(x), lo = bf16(x - hi)), two at a time:
// v_cvt_pk_bf16_f32 packs the pair, so a fragment is assembled from four 32-bit words - element-wise conversion made the compiler
// hold every 16-bit half in a register of its own until a v_perm_b32 packed it (hundreds of spills in the LayerNorm section).
typedef float rf32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 rbf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned ru32x4 __attribute__((ext_vector_type(4)));
typedef unsigned ru32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned rc_pack2(float a, float b) {
    const rf32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, rbf16x2));
}
__device__ __forceinline__ void rc_split2(float a, float b, unsigned &hi, unsigned &lo) {
    asm volatile("" : "+v"(a), "+v"(b));        // the rounded fp32 values (no FMA contraction into the subtractions below)
    hi = rc_pack2(a, b);
    lo = rc_pack2(a - __builtin_bit_cast(float, hi << 16), b - __builtin_bit_cast(float, hi & 0xffff0000u));
}
__device__ __forceinline__ void rc_split8(const float *f, rbf16x8 &hi, rbf16x8 &lo) {
    ru32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) { unsigned a, b; rc_split2(f[2 * i], f[2 * i + 1], a, b); h[i] = a; l[i] = b; }
    hi = __builtin_bit_cast(rbf16x8, h);
    lo = __builtin_bit_cast(rbf16x8, l);
}

// A fragment of weight row (lane & 31) of a 32-row slot block, k-step s (16 k): the tiled image of scp_tile_weight_bf16
//   ROWCHUNK slot ([32 weight rows][256 k]):  plane = [2 row groups][8 k-slabs] x 1 KiB
//   KCHUNK   slot ([256 weight rows][32 k]):  plane = [16 row groups] x 1 KiB, m-block b = row groups 2b, 2b + 1
struct RcLane {
    int lane, col, h, w;
    int frag;          // byte offset of this lane's 16-byte chunk inside a 1 KiB block for k-chunk 0 (k-chunk 1: ^ 32)
    int rg;            // (col >> 4) : which 16-row group of a 32-row block
};

__device__ __forceinline__ RcLane rc_lane() {
    RcLane L;
    const int tid = threadIdx.x;
    L.lane = tid & 63; L.col = L.lane & 31; L.h = L.lane >> 5;
    L.w = __builtin_amdgcn_readfirstlane(tid >> 6);
    L.frag = (L.col & 15) * 64 + ((L.h ^ ((L.col >> 2) & 3)) << 4);
    L.rg = L.col >> 4;
    return L;
}

// Store one m-block (32 output channels x the wave's 32 rows, accumulator layout: lane = row, reg r = channel 8 (r >> 2) + 4 h +
// (r & 3)) as fp32 rows: through the wave's private 4 KiB bounce buffer (16-byte chunk c of row n at chunk c ^ (n & 7): conflict-free
// both ways), so that every global store instruction writes 8 rows x one whole 128-byte line.  `rs` addresses the tile's first
// row of the output (buffer resource: rows beyond M are dropped by the range check, no branch).
__device__ __forceinline__ void rc_store_block(const RcLane &L, char *bounce, const rf32x4 v[4], __amdgpu_buffer_rsrc_t rs, int ldo_bytes, int voff,
                                               int ch0) {
    // voff = (32 w + (lane >> 3)) * ldo_bytes + (lane & 7) * 16: the one per-lane offset; row group and channel block go into the scalar
    // offset of the store (32 per-lane offsets, one per store of a tile, were hoisted, spilled, and each store then waited for its
    // reload - and with it, vmcnt being in order, for every store before it: 20 k cycles per tile)
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *(rf32x4 *)(bounce + L.col * 128 + (((2 * q + L.h) ^ (L.col & 7)) << 4)) = v[q];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    rf32x4 y[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int rho = 8 * it + (L.lane >> 3), kap = L.lane & 7;
        y[it] = *(const rf32x4 *)(bounce + rho * 128 + ((kap ^ (rho & 7)) << 4));
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ri32x4, y[it]), rs, voff, it * 8 * ldo_bytes + ch0 * 4, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the bounce buffer is free again
}

// ---------------------------------------------------------------------------------------------------------------------------------
// LayerNorm statistics of the wave's rows: the lane holds 128 of its row's 256 channels, lane ^ 32 the other 128.  Two-pass
// (mean, then centred squares) in float32 like layernorm_rows_kernel; returns (mean, rstd).
__device__ __forceinline__ void rc_ln_stats(const float *v /*[128]*/, float eps, float &mean, float &rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 128; i += 4) s += (v[i] + v[i + 1]) + (v[i + 2] + v[i + 3]);
    s += __shfl_xor(s, 32);
    mean = s * (1.0f / 256.0f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 128; ++i) { const float d = v[i] - mean; q += d * d; }
    q += __shfl_xor(q, 32);
    rstd = rsqrtf(q * (1.0f / 256.0f) + eps);
}

struct RcLnLinArgs {
    const float *x; int64_t ldx;            // [M][ldx] fp32 rows, 256 channels
    const float *valid;                     // [M] multiplier applied AFTER LayerNorm (0 / 1) or null
    const __bf16 *Whi, *Wlo;                // tiled planes of W' = W diag(gamma), [Npad][256]
    const float *bias, *wbeta;              // [N]: b and W beta (either may be null)
    float *out; int64_t ldo;                // [M][ldo] fp32
    int M, N;                               // N % 128 == 0
    float eps;
    int probe;                              // timing probes (tools/mb_rowchain_probe.py, SCP_RC_PROBE; RESULTS ARE WRONG): 1 stores dropped, 2 no DMA, 8 no bounce / stores
    unsigned long long *dbg;                // diagnostic stamps (scp_rc_debug_buffer): per wave [barrier waits, steps, LayerNorm, drain, tiles]
    // rc_ln_linear_kernel<., KV = true> (scp_swin_ln_qkv): the first nq steps (64 channels each) are the query, written to `out` as above;
    // the next four are the key heads, the last four the value heads, written as bf16 hi / lo planes in the layout of the plane-fed
    // attention (csrc/attn.hip: swin_attn_planes_kernel): planes = [4][Tp][256] bf16 = K hi, K lo, V^T hi, V^T lo; plane_bytes = Tp * 512
    __bf16 *planes; int64_t plane_bytes; int nq;
    // Round 5, short launches (the decoder's one-window forwards: 4 - 64 tiles on 256 CUs, every launch as long as ONE tile's serial chain of
    // steps): `ngroups` workgroups share a tile, each runs LayerNorm on the tile's rows and then its own run of nsteps / ngroups steps (an even
    // number, never straddling query / key / value).  Every output channel is still one accumulation chain of one wave: identical bits.
    int ngroups;
};

// lnlin2.hip: the form of the LayerNorm + linear kernel with two workgroups per CU (same bits).  Mode: 0 by launch size, 1 never, 2 always.
int scp_lnlin2_mode();
int scp_lnlin2_launch(RcLnLinArgs a, bool kv, int ncu, hipStream_t stream);
