// LayerNorm + projection of the Swin blocks, the form with TWO independent workgroups per CU (gfx950 / CDNA4).
//
// Same per-row arithmetic as rc_ln_linear_kernel (rowchain.hip) - every output element is one accumulation chain that starts from b or
// b + W beta and runs k-steps 0 .. 15 with the three bf16x3 products in the order lo.hi, hi.lo, hi.hi; statistics, split and plane layouts
// come from rc_common.h - so it gives the same bits for every row.  What differs is how the work is scheduled.  rc_ln_linear_kernel is one wave
// per SIMD (465 registers, 160 KB of LDS) with every memory instruction hand-dealt into an MFMA gap; a lone wave issues in order, so whenever
// a store, an LDS-DMA piece or a row load is held at issue the matrix pipe behind it waits and the tile lasts the sum of its phases.  Here a
// workgroup fits half a CU (at most 256 registers, 72 KB of LDS, no scratch), two of them are resident, they share no barrier and drift
// apart: one's row fetch, LayerNorm and output epilogues fall under the other's MFMAs.  The fine scheduling is left to the compiler and to
// the second wave.
//
// Geometry: 256 threads, a 128-row tile, wave w owns rows 32 w .. 32 w + 31 as the B operand (A for the value heads) and keeps them in
// registers (Xh / Xl, 128) for the whole tile.  A STEP is 64 output channels (two 32-row blocks of the tiled weight planes, two alternating
// chains: a lone dependent chain of v_mfma_f32_32x32x16 issues every 45 - 52 cycles instead of 32); it runs as four QUARTERS of 4 k-steps
// (64 k) each.  LDS: a ring of three 16 KiB quarters - the one in use, the next, and the one being filled two quarters (1 536 matrix cycles)
// ahead; the 1 KiB blocks of scp_tile_weight_bf16 are fetched by LDS-DMA as they are, a quarter is [block 0, 1][hi, lo][row group 0, 1]
// [k-slab 0, 1] x 1 KiB, 4 pieces per wave.  Then the 4 x 4 KiB bounce buffers of the epilogues and b, b + W beta (8 KiB).
// A step's results leave right behind it (no second accumulator pair); its 8 stores are then the youngest memory operations of the wave,
// and the barriers of the next two quarters wait with a counted vmcnt for their weight pieces only, so the stores have two quarters to
// complete.  What rc_ln_linear_kernel has and this has not: the v[128] prefetch of the next tile's rows, the deferred epilogue, the
// gap-by-gap dealing.
//
// Weight fragments and biases are read with inline-asm LDS reads (the compiler's own would wait for the LDS-DMA in flight, which may alias
// them for all it knows).  Biases and the first k-step of a quarter: the reads and their wait are ONE statement with early-clobber outputs.
// Inside a quarter the four reads of k-step s + 1 go out in front of the MFMAs of k-step s and are waited for behind them, by a statement
// that names all four registers as read-write operands, so no consumer can be scheduled above it; that pins order, not register
// allocation, so tests/test_lnlin2_isa.py scans the generated code: nothing may touch a fragment register between its read and its wait.
//
// Measured (one MI355X, 256 CUs, against rc_ln_linear_kernel in interleaved fresh processes; profiles/lnlin2_ab.md): 590 848 rows, N = 768 /
// 512 / 256: 0.905 / 0.592 / 0.327 ms against 1.019 / 0.680 / 0.360; 51 200 rows: 0.077 / 0.067 / 0.040 against 0.100 / 0.084 / 0.048; 192
// tiles: 0.92 / 0.90 / 0.89 of the old kernel's time, 128 tiles (where that kernel shares a tile between two workgroups): 1.19 / 1.05 / 0.89 -
// hence the dispatch threshold in rowchain.hip.  512 one-tile workgroups last 1.63 x 256 of them: two are resident.  Held to one workgroup per
// CU (SCP_LNLIN_ONE=1) the largest launch takes 1.005 ms.  Probes (SCP_RC_PROBE, N = 768): stores dropped 0.754, no weight DMA 0.845, rows from
// cache 0.866, all three 0.637 (0.759 with one workgroup per CU) for 0.36 ms of products: what two workgroups do not hide is vector work -
// LayerNorm and the split, twelve epilogues per tile - not memory.
// Tried and dropped: a ring of two 32 KiB half-steps with the biases from global memory (64 more registers: spilled; behind the epilogue they
// would wait for its stores); a branch per quarter between value heads and the other steps (the compiler copied the accumulators at every
// merge: +2 %; two loops now); one fragment set without read-ahead (+1.5 %); the leftover tiles of the static split shared out by steps
// among the idle workgroups (-1.4 % at 590 848 rows, +5 ... 12 % at 87 040: the launch does not last a whole number of rounds).
#include <stdlib.h>
#include <type_traits>
#include "rc_common.h"

#define L2_Q 16384                                      // one quarter of a step's weights: 64 channels x 64 k, hi and lo
#define L2_OFF_BOUNCE (3 * L2_Q)
#define L2_OFF_BIAS (L2_OFF_BOUNCE + 4 * RC_BOUNCE)     // b[1024], (b + W beta)[1024]
#define L2_LDS (L2_OFF_BIAS + 8192)                     // 72 KiB: two workgroups per CU
static_assert(L2_LDS <= 80 * 1024, "two workgroups per CU: at most half of the 160 KiB");
#define L2_LDS_ONE (160 * 1024)                         // SCP_LNLIN_ONE=1: the same kernel held to one workgroup per CU (measurement)

// the 4 pieces this wave fetches of quarter qt of step j: piece i = [block i >> 1][plane i & 1], row group w >> 1, k-slab 2 qt + (w & 1)
// (buffer form: the per-lane offset 16 lane in one register for all pieces, the piece's offset in an SGPR)
__device__ __forceinline__ void l2_issue(const RcLane &L, __amdgpu_buffer_rsrc_t wr_hi, __amdgpu_buffer_rsrc_t wr_lo, int j, int qt, char *dst) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = i >> 1, plane = i & 1;
        const int soff = ((2 * j + b) * 16 + (L.w >> 1) * 8 + qt * 2 + (L.w & 1)) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(plane ? wr_lo : wr_hi, (rc_lds_ptr_t)(dst + (L.w + 4 * i) * 1024), 16, L.lane * 16, soff, 0, 0);
    }
}

// four 16-byte LDS reads and their wait
#define L2_READ4(d0, d1, d2, d3, addr, o0, o1, o2, o3)                                                                                  \
    asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\t"                      \
                 "ds_read_b128 %3, %4 offset:%8\n\ts_waitcnt lgkmcnt(0)"                                                                  \
                 : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3) : "v"(addr), "n"(o0), "n"(o1), "n"(o2), "n"(o3) : "memory")
// the same reads without the wait, and the wait that retires them (see the head of this file)
#define L2_READ4_AHEAD(d0, d1, d2, d3, addr, o0, o1, o2, o3)                                                                            \
    asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\t"                      \
                 "ds_read_b128 %3, %4 offset:%8"                                                                                         \
                 : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3) : "v"(addr), "n"(o0), "n"(o1), "n"(o2), "n"(o3) : "memory")
#define L2_WAIT4(d0, d1, d2, d3) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(d0), "+v"(d1), "+v"(d2), "+v"(d3) :: "memory")
// barrier in front of a quarter: this wave's pieces of it have landed (N younger memory operations may stay in flight), and every wave is
// done with the quarter before, whose ring slot is filled next
#define L2_TOP(N) asm volatile("s_waitcnt vmcnt(" #N ") lgkmcnt(0)\n\ts_barrier" ::: "memory")

// one quarter: k-steps 4 Q .. 4 Q + 3 of both chains; ad0 / ad1 = the lane's fragment address in the quarter's ring slot, k-chunk 0 / 1.
// Fragments: A[0] hi of block 0, A[1] lo of block 0, A[2] hi of block 1, A[3] lo of block 1.  SWAP (value heads): the operands change
// places, the accumulator holds C[row][channel] with lane = channel - the order V^T tiles are stored in; same products, same k order.
template <bool SWAP, int Q>
__device__ __forceinline__ void l2_quarter(unsigned ad0, unsigned ad1, rf32x16 &c0, rf32x16 &c1, const rbf16x8 (&Xh)[16], const rbf16x8 (&Xl)[16]) {
#define L2_MFMA(c, wf, xf) c = SWAP ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, wf, c, 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, xf, c, 0, 0, 0)
#define L2_FRAGS(M, A, ad, s) M(A[1], A[3], A[0], A[2], ad, 4096 + ((s) >> 1) * 1024, 12288 + ((s) >> 1) * 1024, ((s) >> 1) * 1024, 8192 + ((s) >> 1) * 1024)
    rbf16x8 A[2][4];
    L2_FRAGS(L2_READ4, A[0], ad0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k = 4 * Q + s, n = (s + 1) & 1;
        if (s < 3) {
            if (n) L2_FRAGS(L2_READ4_AHEAD, A[1], ad1, s + 1);
            else L2_FRAGS(L2_READ4_AHEAD, A[0], ad0, s + 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        L2_MFMA(c0, A[s & 1][1], Xh[k]);
        L2_MFMA(c1, A[s & 1][3], Xh[k]);
        L2_MFMA(c0, A[s & 1][0], Xl[k]);
        L2_MFMA(c1, A[s & 1][2], Xl[k]);
        L2_MFMA(c0, A[s & 1][0], Xh[k]);
        L2_MFMA(c1, A[s & 1][2], Xh[k]);
        __builtin_amdgcn_sched_barrier(0);
        if (s < 3) L2_WAIT4(A[n][0], A[n][1], A[n][2], A[n][3]);
    }
#undef L2_FRAGS
#undef L2_MFMA
}

__device__ __forceinline__ unsigned l2_split_pair(float x0, float x1, int plane) {
    const unsigned hh = rc_pack2(x0, x1);
    return plane ? rc_pack2(x0 - __builtin_bit_cast(float, hh << 16), x1 - __builtin_bit_cast(float, hh & 0xffff0000u)) : hh;
}

// a key head (accumulators: lane = row) as the K hi / lo planes of the plane-fed attention: rows of 256 bf16, 64 per head
__device__ __forceinline__ void l2_store_k(const RcLane &L, char *bounce, const rf32x16 &c0, const rf32x16 &c1, __amdgpu_buffer_rsrc_t prs, int kvoff,
                                           int pbytes, int head) {
    ri32x4 y[2][4];
    int col = L.col;
    asm volatile("" : "+v"(col));                                   // the bounce addresses are made here, not kept in registers across the steps
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const rf32x16 &c = b ? c1 : c0;
                *(ru32x2 *)(bounce + col * 128 + (((4 * b + q) ^ (col & 7)) << 4) + 8 * L.h) =
                    (ru32x2){l2_split_pair(c[4 * q], c[4 * q + 1], plane), l2_split_pair(c[4 * q + 2], c[4 * q + 3], plane)};
            }
#pragma unroll
        for (int it = 0; it < 4; ++it) y[plane][it] = *(const ri32x4 *)(bounce + it * 1024 + L.lane * 16);
    }
#pragma unroll
    for (int plane = 0; plane < 2; ++plane)
#pragma unroll
        for (int it = 0; it < 4; ++it)
            __builtin_amdgcn_raw_buffer_store_b128(y[plane][it], prs, kvoff, it * 8 * 512 + head * 128 + plane * pbytes, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// a value head (accumulators: lane = channel) as the V^T hi / lo planes: 4 KiB tiles of 32 tokens x 64 channels
__device__ __forceinline__ void l2_store_v(const RcLane &L, char *bounce, const rf32x16 &c0, const rf32x16 &c1, __amdgpu_buffer_rsrc_t prs, int vblk,
                                           int pbytes, int head) {
    ri32x4 y[2][4];
    int col = L.col;
    asm volatile("" : "+v"(col));                                   // (as in l2_store_k)
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const rf32x16 &c = b ? c1 : c0;
                const int d = col + 32 * b, R = d >> 1, sl = (d & 1) * 4 + 2 * cc + L.h;
                *(ru32x4 *)(bounce + R * 128 + ((sl ^ (R & 7)) << 4)) =
                    (ru32x4){l2_split_pair(c[8 * cc], c[8 * cc + 1], plane), l2_split_pair(c[8 * cc + 2], c[8 * cc + 3], plane),
                             l2_split_pair(c[8 * cc + 4], c[8 * cc + 5], plane), l2_split_pair(c[8 * cc + 6], c[8 * cc + 7], plane)};
            }
#pragma unroll
        for (int it = 0; it < 4; ++it) y[plane][it] = *(const ri32x4 *)(bounce + it * 1024 + L.lane * 16);
    }
#pragma unroll
    for (int plane = 0; plane < 2; ++plane)
#pragma unroll
        for (int it = 0; it < 4; ++it)
            __builtin_amdgcn_raw_buffer_store_b128(y[plane][it], prs, L.lane * 16, it * 1024 + (vblk + head) * 4096 + (2 + plane) * pbytes, 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// KV = false (scp_swin_ln_linear): every step leaves as fp32 rows.  KV = true (scp_swin_ln_qkv): the first nq steps are the query (fp32 rows),
// the next four the key heads, the last four the value heads (planes, see RcLnLinArgs).
template <bool KV>
__global__ __launch_bounds__(256, 2) void ln2_proj_kernel(const RcLnLinArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const RcLane L = rc_lane();
    const int ntiles = (a.M + RC_ROWS - 1) / RC_ROWS;
    const int nsteps = a.N >> 6;
    const int nq = KV ? a.nq : nsteps;
    char *bounce = smem + L2_OFF_BOUNCE + L.w * RC_BOUNCE;
    const unsigned ab = (unsigned)(uintptr_t)(rc_lds_ptr_t)smem + L.rg * 2048;
    const unsigned af0 = ab + L.frag, af1 = ab + (L.frag ^ 32);     // fragment address in ring slot 0, k-chunk 0 / 1
    const unsigned asb = (unsigned)(uintptr_t)(rc_lds_ptr_t)(smem + L2_OFF_BIAS);
    const int ldo_bytes = (int)(a.ldo * 4);
    const int voff = (32 * L.w + (L.lane >> 3)) * ldo_bytes + (L.lane & 7) * 16;
    const int pbytes = (int)a.plane_bytes;
    const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc((void *)a.planes, 0, (KV && !(a.probe & 1)) ? (int)(4 * a.plane_bytes) : 0, 0x00020000);
    const bool dma = !(a.probe & 2);                                // timing probes (SCP_RC_PROBE; RESULTS ARE WRONG): 1 stores dropped, 2 no LDS-DMA, 4 every tile reads the rows of the first (cache hits)

    const int wbytes = ((a.N + 255) & ~255) * 512;                  // one weight plane: [Npad][256] bf16
    const __amdgpu_buffer_rsrc_t wr_hi = __builtin_amdgcn_make_buffer_rsrc((void *)a.Whi, 0, wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wr_lo = __builtin_amdgcn_make_buffer_rsrc((void *)a.Wlo, 0, wbytes, 0x00020000);

    float *sb = (float *)(smem + L2_OFF_BIAS), *sbw = sb + 1024;    // b and b + W beta
    for (int i = threadIdx.x; i < a.N; i += 256) {
        const float b = a.bias ? a.bias[i] : 0.f;
        sb[i] = b; sbw[i] = b + (a.wbeta ? a.wbeta[i] : 0.f);
    }
    __syncthreads();
    // the ring: quarter g of the wave's sequence (4 per step, running on across tiles) lives in slot g % 3
    int slot = 0;                                                   // of the quarter about to run
    if (dma) { l2_issue(L, wr_hi, wr_lo, 0, 0, smem); l2_issue(L, wr_hi, wr_lo, 0, 1, smem + L2_Q); }
    for (int tile = blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
        const int m0 = tile * RC_ROWS;
        const int row = m0 + 32 * L.w + L.col;
        const int rowc = row < a.M ? row : a.M - 1;
        float keep = (row < a.M) ? 1.0f : 0.0f;
        if (a.valid) keep *= a.valid[rowc];
        rbf16x8 Xh[16], Xl[16];
        {
            // the rows (k = 16 s + 8 h + i of row `col`: natural k order), their statistics, and the split in place
            float v[128];
            const float *src = a.x + (int64_t)((a.probe & 4) ? (rowc & 127) % a.M : rowc) * a.ldx + 8 * L.h;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const rf32x4 q0 = *(const rf32x4 *)(src + 16 * s), q1 = *(const rf32x4 *)(src + 16 * s + 4);
#pragma unroll
                for (int u = 0; u < 4; ++u) { v[8 * s + u] = q0[u]; v[8 * s + 4 + u] = q1[u]; }
            }
            float mean, rstd;
            rc_ln_stats(v, a.eps, mean, rstd);
            const float sc = rstd * keep;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                float f[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] = (v[8 * s + i] - mean) * sc;
                rc_split8(f, Xh[s], Xl[s]);
            }
        }
        const bool kept = keep != 0.f;                              // rows the window pads after LayerNorm get b alone
        const int64_t rows_left = (int64_t)a.M - m0;
        const int64_t span = (rows_left < RC_ROWS ? rows_left : RC_ROWS) * a.ldo * 4;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + (int64_t)m0 * a.ldo, 0, (a.probe & 1) ? 0 : (int)span, 0x00020000);
        const unsigned kmask = (unsigned)__builtin_amdgcn_ballot_w64(kept);             // valid bits of the wave's 32 rows (lanes 0 - 31)
        const unsigned maskh = kmask >> (4 * L.h);
        const int kvoff = (m0 + 32 * L.w + (L.lane >> 3)) * 512 + (L.lane & 7) * 16;     // key planes: row 8 it + (lane >> 3), chunk lane & 7
        const int vblk = ((m0 >> 5) + L.w) * 4;                      // value planes: this wave's 32-token block, head 0

        // Biases of step j, the accumulators' start: lane = row (register r = channel 8 (r >> 2) + 4 h + (r & 3); rows the window pads
        // after LayerNorm get b alone) or, value heads, lane = channel (the row is the register: maskh)
        const unsigned atb = asb + (kept ? 4096 : 0) + 16 * L.h, atv = asb + 4 * L.col;
        rf32x16 c0, c1;
        auto bias_start = [&](int j) {
            if (KV && j >= nq + 4) {
                float bb[2], bwv[2];
                const unsigned ad = atv + 256 * j;
                asm volatile("ds_read_b32 %0, %4\n\tds_read_b32 %1, %4 offset:128\n\tds_read_b32 %2, %4 offset:4096\n\tds_read_b32 %3, %4 offset:4224\n\t"
                             "s_waitcnt lgkmcnt(0)" : "=&v"(bb[0]), "=&v"(bb[1]), "=&v"(bwv[0]), "=&v"(bwv[1]) : "v"(ad) : "memory");
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    rf32x16 &c = blk ? c1 : c0;
#pragma unroll
                    for (int r = 0; r < 16; ++r) c[r] = ((maskh >> (8 * (r >> 2) + (r & 3))) & 1u) ? bwv[blk] : bb[blk];
                }
            } else {
                const unsigned ad = atb + 256 * j;
                rf32x4 t[2][4];
                L2_READ4(t[0][0], t[0][1], t[0][2], t[0][3], ad, 0, 32, 64, 96);
                L2_READ4(t[1][0], t[1][1], t[1][2], t[1][3], ad, 128, 160, 192, 224);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int u = 0; u < 4; ++u) { c0[4 * q + u] = t[0][q][u]; c1[4 * q + u] = t[1][q][u]; }
            }
        };
        bias_start(0);
        SCP_WAIT_DMA(0);                                            // (nothing of this wave is in flight across a tile boundary)
        // steps [ja, jb) of one kind (SW: value heads) - two loops rather than a branch per quarter, behind which the compiler kept the
        // accumulators in different registers and copied them at every merge
        auto steps = [&](auto sw, int ja, int jb) {
        constexpr bool SW = decltype(sw)::value;
        for (int j = ja; j < jb; ++j) {
            const int jn = j + 1 < nsteps ? j + 1 : 0;              // the step behind this one (the next tile's first one at the end)
            // Quarter Q: its pieces were requested at the top of the quarter before last; younger than they are the 4 pieces of the next
            // quarter and, for quarters 0 and 1, the 8 stores of the step before - which therefore have two quarters to complete.
#define L2_QUARTER(Q, N)                                                                                                                \
            {                                                                                                                           \
                L2_TOP(N);                                                                                                              \
                const int sl2 = slot == 0 ? 2 : slot - 1;               /* (slot + 2) % 3: the quarter before this one, free now */     \
                if (dma) l2_issue(L, wr_hi, wr_lo, Q < 2 ? j : jn, (Q + 2) & 3, smem + sl2 * L2_Q);                                       \
                __builtin_amdgcn_sched_barrier(0);                                                                                      \
                const unsigned a0 = af0 + slot * L2_Q, a1 = af1 + slot * L2_Q;                                                          \
                l2_quarter<SW, Q>(a0, a1, c0, c1, Xh, Xl);                                                                              \
                slot = slot == 2 ? 0 : slot + 1;                                                                                        \
            }
            L2_QUARTER(0, 12)
            L2_QUARTER(1, 12)
            L2_QUARTER(2, 4)
            L2_QUARTER(3, 4)
#undef L2_QUARTER
            __builtin_amdgcn_sched_barrier(0);
            if (!SW && j < nq) {
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    rf32x4 o[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int u = 0; u < 4; ++u) o[q][u] = (blk ? c1 : c0)[4 * q + u];
                    rc_store_block(L, bounce, o, rs, ldo_bytes, voff, 64 * j + 32 * blk);
                }
            } else if (!SW) {
                l2_store_k(L, bounce, c0, c1, prs, kvoff, pbytes, j - nq);
            } else {
                l2_store_v(L, bounce, c0, c1, prs, vblk, pbytes, j - nq - 4);
            }
            if (j + 1 < nsteps) bias_start(jn);
        }
        };
        if (KV) { steps(std::false_type(), 0, nq + 4); steps(std::true_type(), nq + 4, nsteps); }
        else steps(std::false_type(), 0, nsteps);
    }
    SCP_WAIT_DMA(0);                                                // the quarters requested for a tile that does not exist
}

// which form scp_swin_ln_linear / scp_swin_ln_qkv launch: SCP_LNLIN=1 rc_ln_linear_kernel everywhere, 2 this file's kernel everywhere
// (A/B bracket, identical bits), anything else by launch size.  Read once.
int scp_lnlin2_mode() {
    static int mode = -1;
    if (mode < 0) { const char *e = getenv("SCP_LNLIN"); mode = e ? atoi(e) : 0; if (mode < 0 || mode > 2) mode = 0; }
    return mode;
}

int scp_lnlin2_launch(RcLnLinArgs a, bool kv, int ncu, hipStream_t stream) {
    static int one = -1, probe = -1;
    if (one < 0) { const char *e = getenv("SCP_LNLIN_ONE"); one = (e && e[0] == '1') ? 1 : 0; }
    if (probe < 0) { const char *e = getenv("SCP_RC_PROBE"); probe = e ? atoi(e) : 0; }
    static bool configured = false;
    if (!configured) {
        HIP_TRY(hipFuncSetAttribute((const void *)ln2_proj_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, one ? L2_LDS_ONE : L2_LDS));
        HIP_TRY(hipFuncSetAttribute((const void *)ln2_proj_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, one ? L2_LDS_ONE : L2_LDS));
        configured = true;
    }
    a.ngroups = 1; a.probe = probe; a.dbg = nullptr;
    const int ntiles = (a.M + RC_ROWS - 1) / RC_ROWS;
    const int wgs = (one ? 1 : 2) * ncu;
    const dim3 grid((unsigned)(ntiles < wgs ? ntiles : wgs));
    if (kv) hipLaunchKernelGGL(ln2_proj_kernel<true>, grid, dim3(256), one ? L2_LDS_ONE : L2_LDS, stream, a);
    else hipLaunchKernelGGL(ln2_proj_kernel<false>, grid, dim3(256), one ? L2_LDS_ONE : L2_LDS, stream, a);
    LAUNCH_CHECK();
    return SCP_OK;
}
