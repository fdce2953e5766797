// Ring LOD ("Ring LOD"): every range ring of a frame has its own octree truncation depth.  Two entry points (gfx950), both
// integer only - an encoder and a decoder that share them cannot disagree:
//
//   scp_ringlod_cells   j[r] = J(origin_r, s_r): the size exponent of the largest TERMINAL cell around an integer position.  A cell of size
//                       2^j has the origin o = (x >> j) << j per axis and the doubled radial centre c2 = 2 o[0] + 2^j - 1 (int64); its ring is
//                       the number of thresholds t_i with c2 >= 2 t_i, and it is terminal iff drops[ring] >= j.  J is the largest j in
//                       max(s, 1) .. max(drops) with a terminal cell, 0 without one.  One thread per row; the tables lie in LDS.  The same call
//                       snaps points (s = 0, with the snapped origins as a second output), marks the implied nodes of a tree (s = the node's
//                       own size exponent, from its level) and sizes the leaves a decoder ends with (s = 0).
//   scp_force_rows      the logits row of every masked row becomes (0, -1000, -1000, ...): one-hot on symbol 0 under every softmax the coders
//                       run.  A wavefront per row, lane l owns columns 4 l .. 4 l + 3 (as scp_scale_rows); unmasked rows and columns >= nsym
//                       keep their bits.  Optionally counts the masked rows whose coded symbol is not 0 (integer atomic add, one per
//                       wavefront that found any).
// No floating-point arithmetic and no floating-point atomics: the two constants of a forced row are stored, nothing is computed.
#include "scp_internal.h"

#define RL_THREADS 256
#define RL_ROWS_PER_BLOCK 4            // scp_force_rows: a wavefront per row

struct rl_table {                      // 288 bytes: 36 words of 8
    int64_t thr[SCP_RINGLOD_MAX_RINGS - 1];        // ascending; entries >= nring - 1 are never read
    uint8_t drops[SCP_RINGLOD_MAX_RINGS];
    int32_t nring;
    int32_t kmax;
};
static_assert(sizeof(rl_table) % 8 == 0, "rl_table is copied in 8-byte words");
static_assert(sizeof(scp_ringlod_seg) == 24, "scp_ringlod_seg layout");

static inline int64_t rl_tables_bytes(int32_t ntab) { return (int64_t)ntab * (int64_t)sizeof(rl_table); }

extern "C" int64_t scp_ringlod_workspace_bytes(int32_t ntab, int32_t nseg) {
    if (ntab < 1 || ntab > SCP_RINGLOD_MAX_TABLES || nseg < 0 || nseg > SCP_RINGLOD_MAX_TABLES) return SCP_EINVAL;
    return rl_tables_bytes(ntab) + (int64_t)nseg * (int64_t)sizeof(scp_ringlod_seg);
}

__global__ __launch_bounds__(RL_THREADS) void ringlod_cells_kernel(const int32_t *origins, int64_t n, int start, const uint8_t *__restrict__ level,
                                                                   const rl_table *__restrict__ d_tabs, int ntab,
                                                                   const scp_ringlod_seg *__restrict__ d_segs, int nseg,
                                                                   uint8_t *__restrict__ jout, int32_t *snapped) {
    __shared__ rl_table s_tab[SCP_RINGLOD_MAX_TABLES];
    __shared__ scp_ringlod_seg s_seg[SCP_RINGLOD_MAX_TABLES];
    {
        const int64_t *src = (const int64_t *)d_tabs;
        int64_t *dst = (int64_t *)s_tab;
        const int words = ntab * (int)(sizeof(rl_table) / 8);
        for (int i = threadIdx.x; i < words; i += RL_THREADS) dst[i] = src[i];
        const int64_t *ssrc = (const int64_t *)d_segs;
        int64_t *sdst = (int64_t *)s_seg;
        for (int i = threadIdx.x; i < nseg * 3; i += RL_THREADS) sdst[i] = ssrc[i];
    }
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * RL_THREADS + threadIdx.x;
    if (r >= n) return;
    const int32_t x0 = origins[3 * r], x1 = origins[3 * r + 1], x2 = origins[3 * r + 2];
    int tab = 0, s = start, held = 1;
    if (nseg > 0) {
        held = 0;
        for (int k = 0; k < nseg; ++k) {                   // (the segments are few and disjoint: a row lies in at most one)
            if (r >= s_seg[k].first && r - s_seg[k].first < s_seg[k].count) {
                held = 1;
                tab = s_seg[k].table;
                if (level) s = s_seg[k].depth - (int)level[r] + 1;
                break;
            }
        }
    }
    int best = 0;
    if (held) {
        const rl_table &t = s_tab[tab];
        const int nthr = t.nring - 1;
        for (int j = s < 1 ? 1 : s; j <= t.kmax; ++j) {
            const int64_t o = ((int64_t)x0 >> j) << j;
            const int64_t c2 = 2 * o + ((int64_t)1 << j) - 1;
            int ring = 0;
            for (int i = 0; i < nthr; ++i) ring += c2 >= 2 * t.thr[i] ? 1 : 0;
            if ((int)t.drops[ring] >= j) best = j;
        }
    }
    jout[r] = (uint8_t)best;
    if (snapped) {
        snapped[3 * r] = (x0 >> best) << best;
        snapped[3 * r + 1] = (x1 >> best) << best;
        snapped[3 * r + 2] = (x2 >> best) << best;
    }
}

extern "C" int scp_ringlod_cells(const int32_t *origins, int64_t n, int32_t start, const uint8_t *level, const scp_ringlod_seg *segs, int32_t nseg,
                                 const int64_t *thresholds, const uint8_t *drops, int32_t ntab, int32_t nring, uint8_t *j, int32_t *snapped,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    if (n < 0 || nseg < 0 || nseg > SCP_RINGLOD_MAX_TABLES || ntab < 1 || ntab > SCP_RINGLOD_MAX_TABLES) return SCP_EINVAL;
    if (nring < 1 || nring > SCP_RINGLOD_MAX_RINGS || !drops || (nring > 1 && !thresholds)) return SCP_EINVAL;
    if (start < 0 || start > SCP_MAX_DEPTH + 1 || (nseg > 0 && !segs) || (level && nseg == 0)) return SCP_EINVAL;
    if (n > 0 && (!origins || !j)) return SCP_EINVAL;
    if (!workspace || (((uintptr_t)workspace) & 7) || workspace_bytes < scp_ringlod_workspace_bytes(ntab, nseg)) return SCP_EINVAL;
    static thread_local rl_table host[SCP_RINGLOD_MAX_TABLES];
    for (int t = 0; t < ntab; ++t) {
        rl_table &h = host[t];
        h.nring = nring;
        h.kmax = 0;
        int64_t prev = 0;
        for (int i = 0; i < SCP_RINGLOD_MAX_RINGS - 1; ++i) {
            int64_t v = INT64_MAX;
            if (i < nring - 1) {
                v = thresholds[(int64_t)t * (nring - 1) + i];
                if (v < prev || v > (int64_t)INT32_MAX) return SCP_EINVAL;      // negative, descending or beyond the clamp
                prev = v;
            }
            h.thr[i] = v;
        }
        for (int i = 0; i < SCP_RINGLOD_MAX_RINGS; ++i) {
            const uint8_t d = i < nring ? drops[(int64_t)t * nring + i] : 0;
            if (d > SCP_RINGLOD_MAX) return SCP_EINVAL;
            h.drops[i] = d;
            h.kmax = d > h.kmax ? d : h.kmax;
        }
    }
    for (int s = 0; s < nseg; ++s) {
        if (segs[s].first < 0 || segs[s].count < 0 || segs[s].first > n || segs[s].count > n - segs[s].first) return SCP_EINVAL;
        if (segs[s].table < 0 || segs[s].table >= ntab || segs[s].depth < 0 || segs[s].depth > SCP_MAX_DEPTH) return SCP_EINVAL;
        for (int q = 0; q < s; ++q)                          // disjoint: a row has one table
            if (segs[s].count > 0 && segs[q].count > 0 && segs[s].first < segs[q].first + segs[q].count && segs[q].first < segs[s].first + segs[s].count)
                return SCP_EINVAL;
    }
    if (n == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    rl_table *d_tabs = (rl_table *)workspace;
    scp_ringlod_seg *d_segs = (scp_ringlod_seg *)((uint8_t *)workspace + rl_tables_bytes(ntab));
    HIP_TRY(hipMemcpyAsync(d_tabs, host, (size_t)rl_tables_bytes(ntab), hipMemcpyHostToDevice, st));
    if (nseg > 0) HIP_TRY(hipMemcpyAsync(d_segs, segs, (size_t)nseg * sizeof(scp_ringlod_seg), hipMemcpyHostToDevice, st));
    const int64_t nb = cdiv64(n, RL_THREADS);
    if (nb > 0x7fffffffll) return SCP_EINVAL;
    hipLaunchKernelGGL(ringlod_cells_kernel, dim3((unsigned)nb), dim3(RL_THREADS), 0, st, origins, n, (int)start, level, d_tabs, (int)ntab, d_segs,
                       (int)nseg, j, snapped);
    LAUNCH_CHECK();
    return SCP_OK;
}

#define RL_FORCED_FIRST 0.0f
#define RL_FORCED_REST -1000.0f

template <bool VEC>
__global__ __launch_bounds__(256) void force_rows_kernel(float *table, int64_t ld, int64_t n, int nsym, const uint8_t *__restrict__ mask,
                                                         const uint8_t *__restrict__ sym, unsigned long long *mismatch) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * RL_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * RL_ROWS_PER_BLOCK;
    unsigned long long bad = 0;                            // (the same in every lane of the wavefront)
    for (int64_t r = wave; r < n; r += nwave) {
        if (!mask[r]) continue;
        if (sym && sym[r] != 0) ++bad;
        float *dst = table + r * ld;
        const int c = 4 * lane;
        if (VEC && c + 3 < nsym) {                         // stride 256, 16-byte aligned base: four whole columns in one store
            *(float4 *)(dst + c) = make_float4(c == 0 ? RL_FORCED_FIRST : RL_FORCED_REST, RL_FORCED_REST, RL_FORCED_REST, RL_FORCED_REST);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < nsym) dst[c + k] = (c + k) == 0 ? RL_FORCED_FIRST : RL_FORCED_REST;
        }
    }
    if (mismatch && lane == 0 && bad) atomicAdd(mismatch, bad);
}

extern "C" int scp_force_rows(float *table, int64_t ld, int64_t n, int32_t nsym, const uint8_t *mask, const uint8_t *sym, int64_t *mismatch,
                              void *stream) {
    if (n < 0 || nsym < 2 || nsym > 256 || ld < nsym) return SCP_EINVAL;
    if ((sym == nullptr) != (mismatch == nullptr)) return SCP_EINVAL;          // the counter counts symbols: both or neither
    if (mismatch && (((uintptr_t)mismatch) & 7)) return SCP_EINVAL;
    if (n > 0 && (!table || !mask)) return SCP_EINVAL;
    if (n == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t want = cdiv64(n, RL_ROWS_PER_BLOCK);
    const unsigned nb = (unsigned)(want < 16384 ? want : 16384);
    if (ld == 256 && (((uintptr_t)table) & 15) == 0)
        hipLaunchKernelGGL(force_rows_kernel<true>, dim3(nb), dim3(256), 0, st, table, ld, n, (int)nsym, mask, sym, (unsigned long long *)mismatch);
    else
        hipLaunchKernelGGL(force_rows_kernel<false>, dim3(nb), dim3(256), 0, st, table, ld, n, (int)nsym, mask, sym, (unsigned long long *)mismatch);
    LAUNCH_CHECK();
    return SCP_OK;
}
