// The lifting engine of the attribute layers: the integer region-adaptive transform on the tree of attr_common.h, for C value
// planes at once.  The tree, the weights, the merge plan and the step of a pair do not depend on the channel: a thread owns a parent, holds
// its <= 8 children's C values in registers, decides and steps once per pair and takes C differences.  csrc/attr.hip instantiates it with
// one plane and 511 symbols, csrc/color.hip with three planes and 1021 symbols; a layer adds its level-1 epilogue (Store) and nothing else.
//
//   lift_forward   the tree, level 0 of the planes from the caller's values, then per level j = 1 .. D one parent launch: three lifting
//                  stages (axis 2, 1, 0), coefficients planar [C][U - 1] in coding order at (n_j - 1) + first[p] - p, one context array
//                  for the planes, a histogram row per (channel, level) - C LDS rows per workgroup.
//   lift_inverse   the tree with weights only, then levels D .. 1 downwards: each parent replays its merge plan from the weights and
//                  undoes it; level 1 hands the leaves' C values to Store.
//   lift_pairs     (c_low | c_high << 16) of the C n coefficients in payload order from the table of context channel * D + (level - 1).
//   lift_sweep     for a grid of steps at once: the histograms lift_forward would return and the error of what lift_inverse would return,
//                  from lift_forward at Q = 1 and one downward launch per level ("step sweep" below).
//
// The number of entries of a level is known on the device only; every launch is sized by the level's capacity in the workspace and reads
// the count itself, so no entry waits for the device.  Unsorted or repeated leaves give unspecified values, but no access leaves the
// buffers: counts are clamped at the scan (attr_common.h), a parent reads at most 8 children below the count of their level and writes
// inside its own coefficient range below U - 1.  Integer arithmetic and integer atomics (the histogram) only.
#pragma once
#include "attr_common.h"

namespace {

template <int C>
struct lift_planes {
    int32_t *v[C];
};

template <int C>
struct lift_vec {
    int32_t v[C];
};

// the C value planes of the workspace from entry `off` on: plane 0 is the layout's b_val, planes 1 .. C - 1 follow the layout
template <int C>
inline lift_planes<C> lift_values(uint8_t *ws, const at_layout &L, int64_t off) {
    lift_planes<C> p;
    p.v[0] = (int32_t *)(ws + L.b_val) + off;
    for (int ch = 1; ch < C; ++ch) p.v[ch] = (int32_t *)(ws + L.bytes) + (ch - 1) * L.total + off;
    return p;
}

template <int C>
inline int64_t lift_bytes(const at_layout &L) { return (L.bytes + 4 * (C - 1) * L.total + 7) & ~7ll; }

// level 0 of the planes from the caller's values: Src [C][U]
template <int C, typename Src>
__global__ __launch_bounds__(AT_THREADS) void level0_kernel(const Src *__restrict__ src, int64_t U, lift_planes<C> val) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= U) return;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) val.v[ch][i] = (int32_t)src[(int64_t)ch * U + i];
}

template <int C, int ALPHABET, int KMAX>
__global__ __launch_bounds__(AT_THREADS) void lift_kernel(int j, int D, uint32_t Q, const int64_t *__restrict__ counts, const uint32_t *__restrict__ first_j,
                                                          const uint64_t *__restrict__ key_c, const uint32_t *__restrict__ w_c, uint32_t *__restrict__ w_j,
                                                          lift_planes<C> val_c, lift_planes<C> val_j, int16_t *__restrict__ coef, uint8_t *__restrict__ ctx,
                                                          int32_t *__restrict__ hist, int64_t n_coef) {
    __shared__ int32_t s_hist[C * ALPHABET];
    for (int i = threadIdx.x; i < C * ALPHABET; i += AT_THREADS) s_hist[i] = 0;
    __syncthreads();
    const int64_t n_j = counts[j], n_prev = counts[j - 1];
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p < n_j) {
        at_children<C> c;
        at_load(c, p, n_j, n_prev, first_j, key_c, w_c, val_c.v);
        int32_t k[C][7];
        bool em[7];
#pragma unroll
        for (int t = 6; t >= 0; --t) {                  // stage 1 first: pairs 3 .. 6, then 1 .. 2, then 0
            const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
            em[t] = false;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) k[ch][t] = 0;
            if (c.w[hi]) {
                if (c.w[lo]) {                          // the decision, the weight and the step once; C differences
                    const uint32_t W = c.w[lo] + c.w[hi];
                    int32_t d[C];
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        d[ch] = c.v[ch][hi] - c.v[ch][lo];
                        c.v[ch][lo] += (int32_t)at_floordiv((int64_t)c.w[hi] * (int64_t)d[ch], (int64_t)W);
                    }
                    const uint32_t s = at_step(c.w[lo], c.w[hi], Q);
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        const uint32_t ad = (uint32_t)(d[ch] < 0 ? -d[ch] : d[ch]);
                        const int32_t q = (int32_t)((ad + (s >> 1)) / s);
                        k[ch][t] = d[ch] < 0 ? -q : q;
                    }
                    em[t] = true;
                    c.w[lo] = W;
                } else {
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) c.v[ch][lo] = c.v[ch][hi];
                    c.w[lo] = c.w[hi];
                }
                c.w[hi] = 0u;
            }
        }
        w_j[p] = c.w[0];
#pragma unroll
        for (int ch = 0; ch < C; ++ch) val_j.v[ch][p] = c.v[ch][0];
        int64_t pos = (n_j - 1) + c.b - p;
        const int64_t lim = pos + (c.n > 0 ? c.n - 1 : 0);      // this parent's own range
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            if (em[t] && pos < lim && pos < n_coef) {
                ctx[pos] = (uint8_t)(j - 1);
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    int32_t kk = k[ch][t];
                    kk = kk > KMAX ? KMAX : (kk < -KMAX ? -KMAX : kk);          // a weighted mean stays between its inputs: never taken
                    coef[(int64_t)ch * n_coef + pos] = (int16_t)kk;
                    atomicAdd(&s_hist[ch * ALPHABET + 2 * (kk < 0 ? -kk : kk) - (kk > 0 ? 1 : 0)], 1);
                }
                ++pos;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * ALPHABET; i += AT_THREADS) {
        const int ch = C == 1 ? 0 : i / ALPHABET, z = i - ch * ALPHABET;
        if (s_hist[i]) atomicAdd(&hist[((int64_t)ch * D + (j - 1)) * ALPHABET + z], s_hist[i]);
    }
}

__global__ __launch_bounds__(AT_THREADS) void weight_kernel(int j, const int64_t *__restrict__ counts, const uint32_t *__restrict__ first_j,
                                                            const uint32_t *__restrict__ w_c, uint32_t *__restrict__ w_j) {
    const int64_t n_j = counts[j], n_prev = counts[j - 1];
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p >= n_j) return;
    const int64_t b = (int64_t)first_j[p];
    int64_t end = p + 1 < n_j ? (int64_t)first_j[p + 1] : n_prev;
    if (end > n_prev) end = n_prev;
    if (end > b + 8) end = b + 8;
    uint32_t w = 0;
    for (int64_t e = b; e < end; ++e) w += w_c[e];
    w_j[p] = w;
}

template <int C>
__global__ __launch_bounds__(AT_THREADS) void root_kernel(lift_planes<C> val_D, int32_t *__restrict__ root) {
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
        if (blockIdx.x == 0 && (int)threadIdx.x == ch) root[ch] = val_D.v[ch][0];
}

// Store::leaf(out, i, x): what leaf i keeps of its C values x - the layer's clamp, after its inverse colour transform if it has one
template <int C, typename Store>
__global__ __launch_bounds__(AT_THREADS) void unlift_kernel(int j, int D, uint32_t Q, lift_vec<C> root, const int64_t *__restrict__ counts,
                                                            const uint32_t *__restrict__ first_j, const uint64_t *__restrict__ key_c,
                                                            const uint32_t *__restrict__ w_c, lift_planes<C> val_j, lift_planes<C> val_c,
                                                            const int16_t *__restrict__ coef, int64_t n_coef, uint8_t *__restrict__ out) {
    const int64_t n_j = counts[j], n_prev = counts[j - 1];
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p >= n_j) return;
    at_children<0> c;
    at_load(c, p, n_j, n_prev, first_j, key_c, w_c);
    // the merge plan, from the weights alone
    uint32_t wl[7], wh[7];
#pragma unroll
    for (int t = 6; t >= 0; --t) {
        const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
        wl[t] = c.w[lo];
        wh[t] = c.w[hi];
        if (c.w[hi]) {
            c.w[lo] += c.w[hi];
            c.w[hi] = 0u;
        }
    }
    int32_t v[C][8];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
#pragma unroll
        for (int s = 0; s < 8; ++s) v[ch][s] = 0;
        v[ch][0] = j == D ? root.v[ch] : val_j.v[ch][p];
    }
    int64_t pos = (n_j - 1) + c.b - p;
    const int64_t lim = pos + (c.n > 0 ? c.n - 1 : 0);
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
        if (wh[t]) {
            if (wl[t]) {
                const bool have = pos < lim && pos < n_coef;
                const uint32_t s = at_step(wl[t], wh[t], Q);
                const uint32_t W = wl[t] + wh[t];
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const int32_t kk = have ? (int32_t)coef[(int64_t)ch * n_coef + pos] : 0;
                    const int32_t dh = kk * (int32_t)s;
                    v[ch][lo] = v[ch][lo] - (int32_t)at_floordiv((int64_t)wh[t] * (int64_t)dh, (int64_t)W);
                    v[ch][hi] = v[ch][lo] + dh;
                }
                if (have) ++pos;
            } else {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) v[ch][hi] = v[ch][lo];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < c.n) {
            int32_t x[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                x[ch] = 0;
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    if (c.slot_of[i] == (uint32_t)s) x[ch] = v[ch][s];
            }
            if (j == 1) {
                Store::leaf(out, c.b + i, x);
            } else {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) val_c.v[ch][c.b + i] = x[ch];
            }
        }
    }
}

template <int C, int ALPHABET, int KMAX>
__global__ __launch_bounds__(AT_THREADS) void pairs_kernel(const int16_t *__restrict__ coef, const uint8_t *__restrict__ ctx, int64_t n,
                                                           const uint16_t *__restrict__ tables, int D, uint32_t *__restrict__ lohi) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= C * n) return;
    const int ch = C == 1 ? 0 : (int)(i / n);
    int32_t k = coef[i];
    k = k > KMAX ? KMAX : (k < -KMAX ? -KMAX : k);
    const int z = 2 * (k < 0 ? -k : k) - (k > 0 ? 1 : 0);
    int c = ctx[i - (int64_t)ch * n];
    c = c < D ? c : D - 1;
    const uint16_t *row = tables + ((int64_t)ch * D + c) * (ALPHABET + 1);
    lohi[i] = (uint32_t)row[z] | ((uint32_t)row[z + 1] << 16);
}

// src: Src [C][U]; k int16 [C][U - 1], root int32 [C], hist int32 [C D][ALPHABET]
template <int C, int ALPHABET, int KMAX, typename Src>
int lift_forward(const int32_t *leaves, const Src *src, int64_t U, int32_t D, int32_t Q, int16_t *k, uint8_t *ctx, int32_t *root, int32_t *hist,
                 int64_t *level_counts, void *workspace, int64_t workspace_bytes, void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || Q < 1 || Q > 255) return SCP_EINVAL;
    if (!hist || !level_counts || !root || (U > 0 && (!leaves || !src)) || (U > 1 && (!k || !ctx))) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, lift_bytes<C>(L))) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)C * D * ALPHABET * 4, st));
    HIP_TRY(hipMemsetAsync(root, 0, 4 * C, st));
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(level_counts, 0, (size_t)(D + 1) * 8, st));
        return SCP_OK;
    }
    uint8_t *ws = (uint8_t *)workspace;
    const int rc = at_build_tree(leaves, U, D, L, ws, st);
    if (rc) return rc;
    const int64_t *counts = (const int64_t *)(ws + L.b_counts);
    const uint64_t *key = (const uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w);
    hipLaunchKernelGGL((level0_kernel<C, Src>), dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, src, U, lift_values<C>(ws, L, 0));
    LAUNCH_CHECK();
    for (int j = 1; j <= D; ++j) {
        hipLaunchKernelGGL((lift_kernel<C, ALPHABET, KMAX>), dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, (int)D, (uint32_t)Q, counts,
                           first + L.off[j], key + L.off[j - 1], w + L.off[j - 1], w + L.off[j], lift_values<C>(ws, L, L.off[j - 1]),
                           lift_values<C>(ws, L, L.off[j]), k, ctx, hist, U - 1);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((root_kernel<C>), dim3(1), dim3(AT_THREADS), 0, st, lift_values<C>(ws, L, L.off[D]), root);
    LAUNCH_CHECK();
    HIP_TRY(at_copy_counts(level_counts, ws, L, D, st));
    return SCP_OK;
}

// the layer has checked the range of `root`; out is what Store::leaf writes, one item per leaf
template <int C, typename Store>
int lift_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, lift_vec<C> root, const int16_t *k, uint8_t *out, void *workspace,
                 int64_t workspace_bytes, void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || Q < 1 || Q > 255) return SCP_EINVAL;
    if ((U > 0 && (!leaves || !out)) || (U > 1 && !k)) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, lift_bytes<C>(L))) return SCP_EINVAL;
    if (U == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    const int rc = at_build_tree(leaves, U, D, L, ws, st);
    if (rc) return rc;
    const int64_t *counts = (const int64_t *)(ws + L.b_counts);
    const uint64_t *key = (const uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w);
    for (int j = 1; j <= D; ++j) {
        hipLaunchKernelGGL(weight_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, counts, first + L.off[j], w + L.off[j - 1],
                           w + L.off[j]);
        LAUNCH_CHECK();
    }
    for (int j = D; j >= 1; --j) {
        hipLaunchKernelGGL((unlift_kernel<C, Store>), dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, (int)D, (uint32_t)Q, root, counts,
                           first + L.off[j], key + L.off[j - 1], w + L.off[j - 1], lift_values<C>(ws, L, L.off[j]), lift_values<C>(ws, L, L.off[j - 1]), k,
                           U - 1, out);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

// ---------------------------------------------------------------------------------------------------------------- step sweep
// The transform is open-loop: lift_kernel lifts exact values, so the means and the differences d do not depend on Q, and at Q = 1 the
// coefficient planes are the d themselves.  lift_sweep runs lift_forward once at Q = 1 into the workspace and then one downward launch per
// level that serves a whole grid of steps: a thread owns a parent as in unlift_kernel, replays the merge plan from the weights once, holds
// the parent's <= 7 C differences in registers and, per step g, forms s, k and k s, counts the symbol and undoes the pairs - one step's
// v[C][8] live at a time.  The G x C reconstructed planes of a level live in the workspace, two buffers of cap[1] entries per plane that
// the levels use in turn (level j reads buffer j & 1 and writes the other); level D starts every step from the exact root, level 1 applies
// Store::rule in registers and takes the error against the values that were coded.
//
// Histogram: G x C x ALPHABET counters do not fit a workgroup's LDS (16 x 3 x 1021 x 4 = 196 KB against 160 KB per CU, and whole rows
// for fewer steps would leave one workgroup per CU), so the first ZL symbols of every (g, channel) row have LDS counters (dynamic, G C ZL x 4 bytes: 24 KB at G = 16, C = 3,
// ZL = 128, which leaves six workgroups per CU) and the tail goes to the global row with one atomic per symbol: exact either way.  Symbol
// 0, where every thread of a workgroup meets at a large step, is counted in a register first.  sse / linf: per wave by shuffles, per
// workgroup in LDS, then one global atomic per workgroup and output.
struct sweep_steps {
    int32_t q[SCP_SWEEP_MAX_STEPS];
};

template <int C, int ALPHABET, int ZL, typename Store>
inline size_t sweep_lds_bytes(int G) { return (size_t)G * (C * ZL + 2 * Store::OUT) * 4; }

// val_j / val_c: the step planes [G C][cap1] of level j (read; level D reads `top`, the exact level-D planes) and j - 1 (written; LEAF:
// level 0 goes to Store::rule and the error against cmp uint8 [U][OUT] instead)
template <int C, int ALPHABET, int KMAX, int ZL, bool LEAF, typename Store>
__global__ __launch_bounds__(AT_THREADS) void sweep_kernel(int j, int D, int G, sweep_steps steps, const int64_t *__restrict__ counts,
                                                           const uint32_t *__restrict__ first_j, const uint64_t *__restrict__ key_c,
                                                           const uint32_t *__restrict__ w_c, lift_planes<C> top, const int32_t *__restrict__ val_j,
                                                           int32_t *__restrict__ val_c, int64_t cap1, const int16_t *__restrict__ coef, int64_t n_coef,
                                                           const uint8_t *__restrict__ cmp, int32_t *__restrict__ hist,
                                                           unsigned long long *__restrict__ sse, uint32_t *__restrict__ linf) {
    constexpr int OUT = Store::OUT;
    extern __shared__ int32_t s_sweep[];
    int32_t *s_hist = s_sweep;                                  // [G][C][ZL]
    uint32_t *s_sse = (uint32_t *)(s_sweep + G * C * ZL);       // [G][OUT]: a workgroup adds at most 256 x 8 x 255^2 < 2^32
    uint32_t *s_max = s_sse + G * OUT;                          // [G][OUT]
    const int n_lds = G * (C * ZL + 2 * OUT);
    for (int i = threadIdx.x; i < n_lds; i += AT_THREADS) s_sweep[i] = 0;
    __syncthreads();
    const int64_t n_j = counts[j], n_prev = counts[j - 1];
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    const bool active = p < n_j;
    at_children<0> c;
    uint32_t wl[7], wh[7];
    int32_t d[C][7];
    bool have[7];
    c.n = 0;
    c.b = 0;
    if (active) {
        at_load(c, p, n_j, n_prev, first_j, key_c, w_c);
#pragma unroll
        for (int t = 6; t >= 0; --t) {                          // the merge plan, from the weights alone
            const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
            wl[t] = c.w[lo];
            wh[t] = c.w[hi];
            if (c.w[hi]) {
                c.w[lo] += c.w[hi];
                c.w[hi] = 0u;
            }
        }
        int64_t pos = (n_j - 1) + c.b - p;
        const int64_t lim = pos + (c.n > 0 ? c.n - 1 : 0);
#pragma unroll
        for (int t = 0; t < 7; ++t) {                           // the exact differences of this parent's pairs, in coding order
            have[t] = false;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) d[ch][t] = 0;
            if (wh[t] && wl[t] && pos < lim && pos < n_coef) {
                have[t] = true;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) d[ch][t] = (int32_t)coef[(int64_t)ch * n_coef + pos];
                ++pos;
            }
        }
    }
    for (int g = 0; g < G; ++g) {
        uint32_t e2[OUT], em[OUT];
#pragma unroll
        for (int o = 0; o < OUT; ++o) e2[o] = em[o] = 0u;
        if (active) {
            const uint32_t Q = (uint32_t)steps.q[g];
            int32_t v[C][8], zeros[C];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
#pragma unroll
                for (int s = 0; s < 8; ++s) v[ch][s] = 0;
                v[ch][0] = j == D ? top.v[ch][p] : val_j[((int64_t)g * C + ch) * cap1 + p];
                zeros[ch] = 0;
            }
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
                if (wh[t]) {
                    if (wl[t]) {
                        const uint32_t s = at_step(wl[t], wh[t], Q);
                        const uint32_t W = wl[t] + wh[t];
#pragma unroll
                        for (int ch = 0; ch < C; ++ch) {
                            const int32_t dd = d[ch][t];
                            const uint32_t ad = (uint32_t)(dd < 0 ? -dd : dd);
                            const int32_t q = (int32_t)((ad + (s >> 1)) / s);
                            int32_t kk = dd < 0 ? -q : q;
                            kk = kk > KMAX ? KMAX : (kk < -KMAX ? -KMAX : kk);
                            if (have[t]) {
                                const int z = 2 * (kk < 0 ? -kk : kk) - (kk > 0 ? 1 : 0);
                                if (z == 0) ++zeros[ch];
                                else if (z < ZL) atomicAdd(&s_hist[(g * C + ch) * ZL + z], 1);
                                else atomicAdd(&hist[(((int64_t)g * C + ch) * D + (j - 1)) * ALPHABET + z], 1);
                            }
                            const int32_t dh = kk * (int32_t)s;
                            v[ch][lo] = v[ch][lo] - (int32_t)at_floordiv((int64_t)wh[t] * (int64_t)dh, (int64_t)W);
                            v[ch][hi] = v[ch][lo] + dh;
                        }
                    } else {
#pragma unroll
                        for (int ch = 0; ch < C; ++ch) v[ch][hi] = v[ch][lo];
                    }
                }
            }
#pragma unroll
            for (int ch = 0; ch < C; ++ch)
                if (zeros[ch]) atomicAdd(&s_hist[(g * C + ch) * ZL], zeros[ch]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < c.n) {
                    int32_t x[C];
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) {
                        x[ch] = 0;
#pragma unroll
                        for (int s = 0; s < 8; ++s)
                            if (c.slot_of[i] == (uint32_t)s) x[ch] = v[ch][s];
                    }
                    if (LEAF) {
                        int32_t y[OUT];
                        Store::rule(x, y);
#pragma unroll
                        for (int o = 0; o < OUT; ++o) {
                            const int32_t e = y[o] - (int32_t)cmp[(c.b + i) * OUT + o];
                            const uint32_t ae = (uint32_t)(e < 0 ? -e : e);
                            e2[o] += ae * ae;
                            em[o] = ae > em[o] ? ae : em[o];
                        }
                    } else {
#pragma unroll
                        for (int ch = 0; ch < C; ++ch) val_c[((int64_t)g * C + ch) * cap1 + c.b + i] = x[ch];
                    }
                }
            }
        }
        if (LEAF) {
#pragma unroll
            for (int o = 0; o < OUT; ++o) {
                for (int off = warpSize >> 1; off > 0; off >>= 1) {
                    e2[o] += __shfl_down(e2[o], off);
                    const uint32_t m = __shfl_down(em[o], off);
                    em[o] = m > em[o] ? m : em[o];
                }
                if ((threadIdx.x & (warpSize - 1)) == 0) {
                    if (e2[o]) atomicAdd(&s_sse[g * OUT + o], e2[o]);
                    if (em[o]) atomicMax(&s_max[g * OUT + o], em[o]);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G * C * ZL; i += AT_THREADS) {
        if (s_hist[i]) {
            const int row = i / ZL, z = i - row * ZL;           // row = g C + ch
            atomicAdd(&hist[((int64_t)row * D + (j - 1)) * ALPHABET + z], s_hist[i]);
        }
    }
    if (LEAF) {
        for (int i = threadIdx.x; i < G * OUT; i += AT_THREADS) {
            if (s_sse[i]) atomicAdd(&sse[i], (unsigned long long)s_sse[i]);
            if (s_max[i]) atomicMax(&linf[i], s_max[i]);
        }
    }
}

// what follows lift_bytes<C>(L) in a sweep's workspace: the Q = 1 coefficients, contexts and histogram, then the step planes
template <int C, int ALPHABET>
struct sweep_layout {
    int64_t b_coef, b_ctx, b_hist, b_val, bytes, cap1;
    sweep_layout(const at_layout &L, int64_t U, int D, int G) {
        const int64_t n = U > 1 ? U - 1 : 0;
        cap1 = L.cap[1];                                        // the largest level that has step planes: cap[j] does not grow with j
        int64_t b = lift_bytes<C>(L);
        b_coef = b; b += (2 * C * n + 7) & ~7ll;
        b_ctx = b;  b += (n + 7) & ~7ll;
        b_hist = b; b += ((int64_t)4 * C * D * ALPHABET + 7) & ~7ll;
        b_val = b;  b += ((int64_t)4 * 2 * G * C * cap1 + 7) & ~7ll;
        bytes = b;
    }
};

inline bool sweep_steps_ok(const int32_t *steps, int G, sweep_steps &S) {
    if (!steps || G < 1 || G > SCP_SWEEP_MAX_STEPS) return false;
    for (int g = 0; g < SCP_SWEEP_MAX_STEPS; ++g) S.q[g] = 1;
    for (int g = 0; g < G; ++g) {
        if (steps[g] < 1 || steps[g] > 255 || (g > 0 && steps[g] <= steps[g - 1])) return false;
        S.q[g] = steps[g];
    }
    return true;
}

template <int C, int ALPHABET>
int64_t lift_sweep_bytes(int64_t U, int32_t D, int32_t G) {
    at_layout L;
    if (!at_make_layout(U, D, L) || G < 1 || G > SCP_SWEEP_MAX_STEPS) return SCP_EINVAL;
    return sweep_layout<C, ALPHABET>(L, U, D, G).bytes;
}

// src: Src [C][U], the values the layer lifts; cmp uint8 [U][Store::OUT], the values the layer's inverse entry is measured against;
// steps HOST int32 [G]; hist int32 [G][C D][ALPHABET], sse uint64 [G][OUT], linf uint32 [G][OUT], root int32 [C]
template <int C, int ALPHABET, int KMAX, int ZL, typename Store, typename Src>
int lift_sweep(const int32_t *leaves, const Src *src, const uint8_t *cmp, int64_t U, int32_t D, const int32_t *steps, int32_t G, int32_t *hist,
               uint64_t *sse, uint32_t *linf, int32_t *root, int64_t *level_counts, void *workspace, int64_t workspace_bytes, void *stream) {
    static_assert(ZL >= 1 && ZL <= ALPHABET, "the LDS rows hold a prefix of the alphabet");
    at_layout L;
    sweep_steps S;
    if (!at_make_layout(U, D, L) || !sweep_steps_ok(steps, G, S)) return SCP_EINVAL;
    if (!hist || !sse || !linf || !root || !level_counts || (U > 0 && (!leaves || !src || !cmp))) return SCP_EINVAL;
    const sweep_layout<C, ALPHABET> X(L, U, D, G);
    if (!at_ws_ok(workspace, workspace_bytes, X.bytes)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)G * C * D * ALPHABET * 4, st));
    HIP_TRY(hipMemsetAsync(sse, 0, (size_t)G * Store::OUT * 8, st));
    HIP_TRY(hipMemsetAsync(linf, 0, (size_t)G * Store::OUT * 4, st));
    // the tree, the weights, the exact values of every level, the root and the counts; at Q = 1 the coefficients are the differences
    const int rc = lift_forward<C, ALPHABET, KMAX>(leaves, src, U, D, 1, (int16_t *)(ws + X.b_coef), ws + X.b_ctx, root, (int32_t *)(ws + X.b_hist),
                                                   level_counts, workspace, workspace_bytes, stream);
    if (rc || U < 2) return rc;
    const int64_t *counts = (const int64_t *)(ws + L.b_counts);
    const uint64_t *key = (const uint64_t *)(ws + L.b_key);
    const uint32_t *first = (const uint32_t *)(ws + L.b_first), *w = (const uint32_t *)(ws + L.b_w);
    int32_t *planes = (int32_t *)(ws + X.b_val);
    const int64_t half = (int64_t)G * C * X.cap1;
    const size_t lds = sweep_lds_bytes<C, ALPHABET, ZL, Store>(G);
    for (int j = D; j >= 1; --j) {
        const int32_t *val_j = planes + (j & 1) * half;
        int32_t *val_c = planes + ((j - 1) & 1) * half;
        const dim3 grid(at_grid(L.cap[j], AT_THREADS)), block(AT_THREADS);
        if (j > 1)
            hipLaunchKernelGGL((sweep_kernel<C, ALPHABET, KMAX, ZL, false, Store>), grid, block, lds, st, j, (int)D, (int)G, S, counts, first + L.off[j],
                               key + L.off[j - 1], w + L.off[j - 1], lift_values<C>(ws, L, L.off[D]), val_j, val_c, X.cap1,
                               (const int16_t *)(ws + X.b_coef), U - 1, cmp, hist, (unsigned long long *)sse, linf);
        else
            hipLaunchKernelGGL((sweep_kernel<C, ALPHABET, KMAX, ZL, true, Store>), grid, block, lds, st, j, (int)D, (int)G, S, counts, first + L.off[j],
                               key + L.off[j - 1], w + L.off[j - 1], lift_values<C>(ws, L, L.off[D]), val_j, val_c, X.cap1,
                               (const int16_t *)(ws + X.b_coef), U - 1, cmp, hist, (unsigned long long *)sse, linf);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

// k int16 [C][n], tables uint16 [C D][ALPHABET + 1] -> lohi uint32 [C n]
template <int C, int ALPHABET, int KMAX>
int lift_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream) {
    if (n < 0 || n > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH || !tables) return SCP_EINVAL;
    if (n > 0 && (!k || !ctx || !lohi)) return SCP_EINVAL;
    if (n == 0) return SCP_OK;
    hipLaunchKernelGGL((pairs_kernel<C, ALPHABET, KMAX>), dim3(at_grid(C * n, AT_THREADS)), dim3(AT_THREADS), 0, (hipStream_t)stream, k, ctx, n, tables,
                       (int)D, lohi);
    LAUNCH_CHECK();
    return SCP_OK;
}

}  // namespace
