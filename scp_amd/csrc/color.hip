// Colour layer ("Colour"): the RGB of an object cloud on the octree of its shell - per-leaf means, a reversible YCoCg-R
// transform and the reflectance layer's integer lifting (csrc/attr.hip) on the three planes at once, in exact integer arithmetic (gfx950).
// The tree, the weights, the merge plan and the step of a pair do not depend on the channel: they are built and evaluated once
// (attr_common.h) and applied to Y, Co and Cg.
//
//   scp_color_leaf_values  one thread per point: binary search of the point's cell among the leaf keys, three 64-bit integer atomic adds
//                          and the count; then one thread per leaf: the rounded means and their YCoCg-R image (int16, planar).
//   scp_color_forward      the tree once, then per level one parent launch: a thread owns a parent with its <= 8 children's three values
//                          in registers; per pair one merge decision and one step, three differences.  Coefficients planar [3][U - 1] in
//                          the reflectance layer's coding order, one context array for the three planes, a histogram row per (channel,
//                          level) over 1021 symbols - three LDS rows per workgroup.
//   scp_color_inverse      weights once, then levels D .. 1 downwards for the three planes in one launch per level; level 1 undoes the colour
//                          transform and clamps R, G, B to 0 .. 255.
//   scp_color_pairs        (c_low | c_high << 16) of the 3 (U - 1) coefficients in payload order (Y block, Co block, Cg block) from the table
//                          of context channel * D + (level - 1).
//
// As in attr.hip every launch is sized by the host bound min(U, 8^(D-j)) and reads the level's count on the device; here the count is
// also clamped to that bound, so that unsorted or repeated leaves (unspecified values) cannot carry an index out of a level's range.
// Integer arithmetic only.
#include "attr_common.h"

#define CL_ALPHABET 1021
#define CL_KMAX 510

namespace {

struct cl_planes {
    int32_t *v[3];
};

// the three value planes of the workspace: plane 0 is the layout's own, planes 1 and 2 follow the layout
inline cl_planes cl_values(uint8_t *ws, const at_layout &L) {
    cl_planes p;
    p.v[0] = (int32_t *)(ws + L.b_val);
    p.v[1] = (int32_t *)(ws + L.bytes);
    p.v[2] = p.v[1] + L.total;
    return p;
}

inline int64_t cl_bytes(const at_layout &L) { return (L.bytes + 8 * L.total + 7) & ~7ll; }

__global__ __launch_bounds__(AT_THREADS) void color_level0_kernel(const int16_t *__restrict__ ycc, int64_t U, cl_planes val) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= U) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) val.v[ch][i] = (int32_t)ycc[(int64_t)ch * U + i];
}

__device__ __forceinline__ int64_t cl_min(int64_t a, int64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(AT_THREADS) void color_lift_kernel(int j, int D, uint32_t Q, const int64_t *__restrict__ counts, int64_t cap_j, int64_t cap_prev,
                                                                int64_t off_j, int64_t off_prev, const uint32_t *__restrict__ first, const uint64_t *__restrict__ key,
                                                                uint32_t *__restrict__ w, cl_planes val, int16_t *__restrict__ coef, uint8_t *__restrict__ ctx,
                                                                int32_t *__restrict__ hist, int64_t n_coef) {
    __shared__ int32_t s_hist[3 * CL_ALPHABET];
    for (int i = threadIdx.x; i < 3 * CL_ALPHABET; i += AT_THREADS) s_hist[i] = 0;
    __syncthreads();
    const int64_t n_j = cl_min(counts[j], cap_j), n_prev = cl_min(counts[j - 1], cap_prev);
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p < n_j) {
        at_children c;
        at_load<false>(c, p, n_j, n_prev, first + off_j, key + off_prev, w + off_prev, nullptr);
        int32_t v[3][8];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int s = 0; s < 8; ++s) v[ch][s] = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < c.n) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int32_t x = val.v[ch][off_prev + c.b + i];
#pragma unroll
                    for (int s = 0; s < 8; ++s)
                        if (c.slot_of[i] == (uint32_t)s) v[ch][s] = x;
                }
            }
        }
        int32_t k[3][7];
        bool em[7];
#pragma unroll
        for (int t = 6; t >= 0; --t) {                  // stage 1 first: pairs 3 .. 6, then 1 .. 2, then 0
            const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
            em[t] = false;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) k[ch][t] = 0;
            if (c.w[hi]) {
                if (c.w[lo]) {                          // the decision, the weight and the step once; three differences
                    const uint32_t W = c.w[lo] + c.w[hi];
                    const uint32_t s = at_step(c.w[lo], c.w[hi], Q);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const int32_t d = v[ch][hi] - v[ch][lo];
                        const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                        const int32_t q = (int32_t)((ad + (s >> 1)) / s);
                        k[ch][t] = d < 0 ? -q : q;
                        v[ch][lo] += (int32_t)at_floordiv((int64_t)c.w[hi] * (int64_t)d, (int64_t)W);
                    }
                    em[t] = true;
                    c.w[lo] = W;
                } else {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) v[ch][lo] = v[ch][hi];
                    c.w[lo] = c.w[hi];
                }
                c.w[hi] = 0u;
            }
        }
        w[off_j + p] = c.w[0];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) val.v[ch][off_j + p] = v[ch][0];
        int64_t pos = (n_j - 1) + c.b - p;
        const int64_t lim = pos + (c.n > 0 ? c.n - 1 : 0);      // this parent's own range
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            if (em[t] && pos < lim && pos < n_coef) {
                ctx[pos] = (uint8_t)(j - 1);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    int32_t kk = k[ch][t];
                    kk = kk > CL_KMAX ? CL_KMAX : (kk < -CL_KMAX ? -CL_KMAX : kk);      // a weighted mean stays between its inputs: never taken
                    coef[(int64_t)ch * n_coef + pos] = (int16_t)kk;
                    atomicAdd(&s_hist[ch * CL_ALPHABET + 2 * (kk < 0 ? -kk : kk) - (kk > 0 ? 1 : 0)], 1);
                }
                ++pos;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * CL_ALPHABET; i += AT_THREADS) {
        const int ch = i / CL_ALPHABET, z = i - ch * CL_ALPHABET;
        if (s_hist[i]) atomicAdd(&hist[((int64_t)ch * D + (j - 1)) * CL_ALPHABET + z], s_hist[i]);
    }
}

__global__ __launch_bounds__(AT_THREADS) void color_weight_kernel(int j, const int64_t *__restrict__ counts, int64_t cap_j, int64_t cap_prev,
                                                                  const uint32_t *__restrict__ first_j, const uint32_t *__restrict__ w_c, uint32_t *__restrict__ w_j) {
    const int64_t n_j = cl_min(counts[j], cap_j), n_prev = cl_min(counts[j - 1], cap_prev);
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

__global__ __launch_bounds__(AT_THREADS) void color_root_kernel(cl_planes val, int64_t off_D, int32_t *__restrict__ root) {
    if (blockIdx.x == 0 && threadIdx.x < 3) root[threadIdx.x] = val.v[threadIdx.x][off_D];
}

struct cl_root {
    int32_t v[3];
};

__global__ __launch_bounds__(AT_THREADS) void color_unlift_kernel(int j, int D, uint32_t Q, cl_root root, const int64_t *__restrict__ counts, int64_t cap_j,
                                                                  int64_t cap_prev, int64_t off_j, int64_t off_prev, const uint32_t *__restrict__ first,
                                                                  const uint64_t *__restrict__ key, const uint32_t *__restrict__ w, cl_planes val,
                                                                  const int16_t *__restrict__ coef, int64_t n_coef, uint8_t *__restrict__ rgb) {
    const int64_t n_j = cl_min(counts[j], cap_j), n_prev = cl_min(counts[j - 1], cap_prev);
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p >= n_j) return;
    at_children c;
    at_load<false>(c, p, n_j, n_prev, first + off_j, key + off_prev, w + off_prev, nullptr);
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
    int32_t v[3][8];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
        for (int s = 0; s < 8; ++s) v[ch][s] = 0;
        v[ch][0] = j == D ? root.v[ch] : val.v[ch][off_j + p];
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
                for (int ch = 0; ch < 3; ++ch) {
                    const int32_t kk = have ? (int32_t)coef[(int64_t)ch * n_coef + pos] : 0;
                    const int32_t dh = kk * (int32_t)s;
                    v[ch][lo] = v[ch][lo] - (int32_t)at_floordiv((int64_t)wh[t] * (int64_t)dh, (int64_t)W);
                    v[ch][hi] = v[ch][lo] + dh;
                }
                if (have) ++pos;
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][hi] = v[ch][lo];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < c.n) {
            int32_t x[3] = {0, 0, 0};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    if (c.slot_of[i] == (uint32_t)s) x[ch] = v[ch][s];
            if (j == 1) {                               // the leaves: YCoCg-R back to R, G, B, and the only clamp of the layer
                const int32_t t = x[0] - (x[2] >> 1), G = x[2] + t, B = t - (x[1] >> 1), R = B + x[1];
                uint8_t *o = rgb + 3 * (c.b + i);
                o[0] = (uint8_t)(R < 0 ? 0 : (R > 255 ? 255 : R));
                o[1] = (uint8_t)(G < 0 ? 0 : (G > 255 ? 255 : G));
                o[2] = (uint8_t)(B < 0 ? 0 : (B > 255 ? 255 : B));
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) val.v[ch][off_prev + c.b + i] = x[ch];
            }
        }
    }
}

__global__ __launch_bounds__(AT_THREADS) void color_pairs_kernel(const int16_t *__restrict__ coef, const uint8_t *__restrict__ ctx, int64_t n,
                                                                 const uint16_t *__restrict__ tables, int D, uint32_t *__restrict__ lohi) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= 3 * n) return;
    const int ch = (int)(i / n);
    int32_t k = coef[i];
    k = k > CL_KMAX ? CL_KMAX : (k < -CL_KMAX ? -CL_KMAX : k);
    const int z = 2 * (k < 0 ? -k : k) - (k > 0 ? 1 : 0);
    int c = ctx[i - (int64_t)ch * n];
    c = c < D ? c : D - 1;
    const uint16_t *row = tables + ((int64_t)ch * D + c) * (CL_ALPHABET + 1);
    lohi[i] = (uint32_t)row[z] | ((uint32_t)row[z + 1] << 16);
}

__global__ __launch_bounds__(AT_THREADS) void color_point_kernel(const int32_t *__restrict__ q, const uint8_t *__restrict__ rgb, int64_t P,
                                                                 const uint64_t *__restrict__ key, int64_t U, int D, unsigned long long *__restrict__ sum,
                                                                 int32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= P) return;
    const int32_t x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    if ((x | y | z) < 0 || (((int64_t)x | (int64_t)y | (int64_t)z) >> D) != 0) return;
    const uint64_t k = at_morton(x, y, z, D);
    int64_t lo = 0, hi = U;                         // first leaf with key >= k
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    if (lo >= U || key[lo] != k) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) atomicAdd(&sum[(int64_t)ch * U + lo], (unsigned long long)rgb[3 * i + ch]);
    atomicAdd(&cnt[lo], 1);
}

__global__ __launch_bounds__(AT_THREADS) void color_mean_kernel(const unsigned long long *__restrict__ sum, const int32_t *__restrict__ cnt, int64_t U,
                                                                uint8_t *__restrict__ rgb_mean, int16_t *__restrict__ ycc) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= U) return;
    const unsigned long long c = (unsigned long long)(cnt[i] > 0 ? cnt[i] : 0);
    int32_t m[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned long long v = c ? (2ull * sum[(int64_t)ch * U + i] + c) / (2ull * c) : 0ull;
        m[ch] = (int32_t)(v > 255ull ? 255ull : v);
        rgb_mean[3 * i + ch] = (uint8_t)m[ch];
    }
    const int32_t Co = m[0] - m[2], t = m[2] + (Co >> 1), Cg = m[1] - t, Y = t + (Cg >> 1);
    ycc[i] = (int16_t)Y;
    ycc[U + i] = (int16_t)Co;
    ycc[2 * U + i] = (int16_t)Cg;
}

}  // namespace

extern "C" int64_t scp_color_leaf_values_workspace_bytes(int64_t U) {
    if (U < 0 || U - 1 > (1ll << 31)) return SCP_EINVAL;
    return 32 * (U > 0 ? U : 1);
}

extern "C" int64_t scp_color_forward_workspace_bytes(int64_t U, int32_t D) {
    at_layout L;
    return at_make_layout(U, D, L) ? cl_bytes(L) : (int64_t)SCP_EINVAL;
}

extern "C" int64_t scp_color_inverse_workspace_bytes(int64_t U, int32_t D) { return scp_color_forward_workspace_bytes(U, D); }

extern "C" int scp_color_leaf_values(const int32_t *q, const uint8_t *rgb, int64_t P, const int32_t *leaves, int64_t U, int32_t D, uint8_t *rgb_mean,
                                     int16_t *ycc, int32_t *cnt, void *workspace, int64_t workspace_bytes, void *stream) {
    if (P < 0 || P > (1ll << 31) || U < 0 || U - 1 > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH) return SCP_EINVAL;
    if ((P > 0 && (!q || !rgb)) || (U > 0 && (!leaves || !rgb_mean || !ycc || !cnt))) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, scp_color_leaf_values_workspace_bytes(U))) return SCP_EINVAL;
    if (U == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    uint64_t *key = (uint64_t *)workspace;
    unsigned long long *sum = (unsigned long long *)workspace + U;
    HIP_TRY(hipMemsetAsync(sum, 0, (size_t)U * 24, st));
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)U * 4, st));
    hipLaunchKernelGGL(attr_keys_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, leaves, U, (int)D, key);
    LAUNCH_CHECK();
    if (P > 0) {
        hipLaunchKernelGGL(color_point_kernel, dim3(at_grid(P, AT_THREADS)), dim3(AT_THREADS), 0, st, q, rgb, P, key, U, (int)D, sum, cnt);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(color_mean_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, sum, cnt, U, rgb_mean, ycc);
    LAUNCH_CHECK();
    return SCP_OK;
}

extern "C" int scp_color_forward(const int32_t *leaves, const int16_t *ycc, int64_t U, int32_t D, int32_t Q, int16_t *k, uint8_t *ctx, int32_t *root,
                                 int32_t *hist, int64_t *level_counts, void *workspace, int64_t workspace_bytes, void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || Q < 1 || Q > 255) return SCP_EINVAL;
    if (!hist || !level_counts || !root || (U > 0 && (!leaves || !ycc)) || (U > 1 && (!k || !ctx))) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, cl_bytes(L))) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)3 * D * CL_ALPHABET * 4, st));
    HIP_TRY(hipMemsetAsync(root, 0, 12, st));
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(level_counts, 0, (size_t)(D + 1) * 8, st));
        return SCP_OK;
    }
    uint8_t *ws = (uint8_t *)workspace;
    const int rc = at_build_tree(leaves, nullptr, U, D, L, ws, st);
    if (rc) return rc;
    int64_t *counts = (int64_t *)(ws + L.b_counts);
    uint64_t *key = (uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w);
    const cl_planes val = cl_values(ws, L);
    hipLaunchKernelGGL(color_level0_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, ycc, U, val);
    LAUNCH_CHECK();
    for (int j = 1; j <= D; ++j) {
        hipLaunchKernelGGL(color_lift_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, (int)D, (uint32_t)Q, counts, L.cap[j],
                           L.cap[j - 1], L.off[j], L.off[j - 1], first, key, w, val, k, ctx, hist, U - 1);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(color_root_kernel, dim3(1), dim3(AT_THREADS), 0, st, val, L.off[D], root);
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(level_counts, counts, (size_t)(D + 1) * 8, hipMemcpyDeviceToDevice, st));
    return SCP_OK;
}

extern "C" int scp_color_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, const int32_t *root, const int16_t *k, uint8_t *rgb,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || Q < 1 || Q > 255 || !root) return SCP_EINVAL;
    if (root[0] < 0 || root[0] > 255 || root[1] < -255 || root[1] > 255 || root[2] < -255 || root[2] > 255) return SCP_EINVAL;
    if ((U > 0 && (!leaves || !rgb)) || (U > 1 && !k)) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, cl_bytes(L))) return SCP_EINVAL;
    if (U == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    const int rc = at_build_tree(leaves, nullptr, U, D, L, ws, st);
    if (rc) return rc;
    int64_t *counts = (int64_t *)(ws + L.b_counts);
    uint64_t *key = (uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w);
    const cl_planes val = cl_values(ws, L);
    cl_root r;
    for (int ch = 0; ch < 3; ++ch) r.v[ch] = root[ch];
    for (int j = 1; j <= D; ++j) {
        hipLaunchKernelGGL(color_weight_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, counts, L.cap[j], L.cap[j - 1],
                           first + L.off[j], w + L.off[j - 1], w + L.off[j]);
        LAUNCH_CHECK();
    }
    for (int j = D; j >= 1; --j) {
        hipLaunchKernelGGL(color_unlift_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, (int)D, (uint32_t)Q, r, counts, L.cap[j],
                           L.cap[j - 1], L.off[j], L.off[j - 1], first, key, w, val, k, U - 1, rgb);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

extern "C" int scp_color_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream) {
    if (n < 0 || n > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH || !tables) return SCP_EINVAL;
    if (n > 0 && (!k || !ctx || !lohi)) return SCP_EINVAL;
    if (n == 0) return SCP_OK;
    hipLaunchKernelGGL(color_pairs_kernel, dim3(at_grid(3 * n, AT_THREADS)), dim3(AT_THREADS), 0, (hipStream_t)stream, k, ctx, n, tables, (int)D, lohi);
    LAUNCH_CHECK();
    return SCP_OK;
}
