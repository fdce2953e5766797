// Reflectance layer ("Reflectance"): a region-adaptive hierarchical transform on the octree of a shell, in exact integer
// arithmetic (gfx950).  Encoder and decoder run the same integer steps on the same Morton-ordered leaf list, so they agree bit for bit.
//
//   scp_attr_leaf_values   one thread per point: 8-bit value of the reflectance, binary search of the point's cell among the leaf keys,
//                          integer atomic adds of (value, 1) on the leaf; then a = (2 sum + cnt) // (2 cnt) per leaf.
//   scp_attr_forward       keys once (one thread per leaf), then per level j = 1 .. D: head flags of the level-(j-1) entries (a head opens
//                          a new 3-bit prefix), a three-launch scan (block counts, one block over the counts, assignment), and the parent
//                          pass - one thread per parent, its <= 8 children in registers, three lifting stages (axis 2, 1, 0), coefficients
//                          written in coding order at (n_j - 1) + first[p] - p.
//   scp_attr_inverse       the same tree with weights only, then levels D .. 1 downwards: each parent replays its merge plan from the
//                          weights and undoes it.
//   scp_attr_level_counts  the tree alone: n_0 .. n_D, from which a decoder knows every coefficient's context before it has one.
//   scp_attr_pairs         (c_low | c_high << 16) of every coefficient from the chosen table of its context.
//
// The number of entries of a level is known on the device only (counts[j]); every launch is sized by the host bound min(U, 8^(D-j)) and
// reads the count itself, so no entry waits for the device.  Integer atomics only (leaf sums, histogram); no floating-point arithmetic
// except the one exact product r * scale of a point value.  Unsorted or repeated leaves give unspecified values, but no access leaves the
// buffers: a parent reads at most 8 children and writes inside its own coefficient range.
// The tree build, the child load, the step and the pair order are shared with the colour layer (csrc/color.hip): attr_common.h.
#include "attr_common.h"

#define AT_ALPHABET 511

namespace {

__global__ __launch_bounds__(AT_THREADS) void attr_lift_kernel(int j, uint32_t Q, const int64_t *__restrict__ counts, const uint32_t *__restrict__ first_j,
                                                               const uint64_t *__restrict__ key_c, const uint32_t *__restrict__ w_c, const int32_t *__restrict__ val_c,
                                                               uint32_t *__restrict__ w_j, int32_t *__restrict__ val_j, int16_t *__restrict__ coef,
                                                               uint8_t *__restrict__ ctx, int32_t *__restrict__ hist, int64_t n_coef) {
    __shared__ int32_t s_hist[AT_ALPHABET];
    for (int i = threadIdx.x; i < AT_ALPHABET; i += AT_THREADS) s_hist[i] = 0;
    __syncthreads();
    const int64_t n_j = counts[j], n_prev = counts[j - 1];
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p < n_j) {
        at_children c;
        at_load<true>(c, p, n_j, n_prev, first_j, key_c, w_c, val_c);
        int32_t k[7];
        bool em[7];
#pragma unroll
        for (int t = 6; t >= 0; --t) {                  // stage 1 first: pairs 3 .. 6, then 1 .. 2, then 0
            const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
            k[t] = 0;
            em[t] = false;
            if (c.w[hi]) {
                if (c.w[lo]) {
                    const int32_t d = c.v[hi] - c.v[lo];
                    const uint32_t W = c.w[lo] + c.w[hi];
                    const int32_t m = c.v[lo] + (int32_t)at_floordiv((int64_t)c.w[hi] * (int64_t)d, (int64_t)W);
                    const uint32_t s = at_step(c.w[lo], c.w[hi], Q);
                    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                    const int32_t q = (int32_t)((ad + (s >> 1)) / s);
                    k[t] = d < 0 ? -q : q;
                    em[t] = true;
                    c.v[lo] = m;
                    c.w[lo] = W;
                } else {
                    c.v[lo] = c.v[hi];
                    c.w[lo] = c.w[hi];
                }
                c.w[hi] = 0u;
            }
        }
        w_j[p] = c.w[0];
        val_j[p] = c.v[0];
        int64_t pos = (n_j - 1) + c.b - p;
        const int64_t lim = pos + (c.n > 0 ? c.n - 1 : 0);      // this parent's own range
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            if (em[t] && pos < lim && pos < n_coef) {
                int32_t kk = k[t];
                kk = kk > 255 ? 255 : (kk < -255 ? -255 : kk);          // |d| <= 255 on 8-bit leaves: never taken there
                coef[pos] = (int16_t)kk;
                ctx[pos] = (uint8_t)(j - 1);
                atomicAdd(&s_hist[2 * (kk < 0 ? -kk : kk) - (kk > 0 ? 1 : 0)], 1);
                ++pos;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < AT_ALPHABET; i += AT_THREADS)
        if (s_hist[i]) atomicAdd(&hist[(int64_t)(j - 1) * AT_ALPHABET + i], s_hist[i]);
}

__global__ __launch_bounds__(AT_THREADS) void attr_weight_kernel(int j, const int64_t *__restrict__ counts, const uint32_t *__restrict__ first_j,
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

__global__ __launch_bounds__(AT_THREADS) void attr_root_kernel(const int32_t *__restrict__ val_D, int32_t *__restrict__ root) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *root = val_D[0];
}

__global__ __launch_bounds__(AT_THREADS) void attr_unlift_kernel(int j, int D, uint32_t Q, int32_t root, const int64_t *__restrict__ counts,
                                                                 const uint32_t *__restrict__ first_j, const uint64_t *__restrict__ key_c,
                                                                 const uint32_t *__restrict__ w_c, const int32_t *__restrict__ val_j, int32_t *__restrict__ val_c,
                                                                 const int16_t *__restrict__ coef, int64_t n_coef, uint8_t *__restrict__ a) {
    const int64_t n_j = counts[j], n_prev = counts[j - 1];
    const int64_t p = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (p >= n_j) return;
    at_children c;
    at_load<false>(c, p, n_j, n_prev, first_j, key_c, w_c, nullptr);
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
    int32_t v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) v[s] = 0;
    v[0] = j == D ? root : val_j[p];
    int64_t pos = (n_j - 1) + c.b - p;
    const int64_t lim = pos + (c.n > 0 ? c.n - 1 : 0);
#pragma unroll
    for (int t = 0; t < 7; ++t) {
        const int lo = AT_PAIR_LO(t), hi = lo | AT_PAIR_BIT(t);
        if (wh[t]) {
            if (wl[t]) {
                int32_t kk = 0;
                if (pos < lim && pos < n_coef) kk = (int32_t)coef[pos++];
                const uint32_t s = at_step(wl[t], wh[t], Q);
                const int32_t dh = kk * (int32_t)s;
                const uint32_t W = wl[t] + wh[t];
                v[lo] = v[lo] - (int32_t)at_floordiv((int64_t)wh[t] * (int64_t)dh, (int64_t)W);
                v[hi] = v[lo] + dh;
            } else {
                v[hi] = v[lo];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < c.n) {
            int32_t x = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (c.slot_of[i] == (uint32_t)s) x = v[s];
            if (j == 1) a[c.b + i] = (uint8_t)(x < 0 ? 0 : (x > 255 ? 255 : x));
            else val_c[c.b + i] = x;
        }
    }
}

__global__ __launch_bounds__(AT_THREADS) void attr_pairs_kernel(const int16_t *__restrict__ coef, const uint8_t *__restrict__ ctx, int64_t n,
                                                                const uint16_t *__restrict__ tables, int D, uint32_t *__restrict__ lohi) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= n) return;
    int32_t k = coef[i];
    k = k > 255 ? 255 : (k < -255 ? -255 : k);
    const int z = 2 * (k < 0 ? -k : k) - (k > 0 ? 1 : 0);
    int c = ctx[i];
    c = c < D ? c : D - 1;
    const uint16_t *row = tables + (int64_t)c * (AT_ALPHABET + 1);
    lohi[i] = (uint32_t)row[z] | ((uint32_t)row[z + 1] << 16);
}

__global__ __launch_bounds__(AT_THREADS) void attr_point_kernel(const int32_t *__restrict__ q, const float *__restrict__ r, int64_t P,
                                                                const uint64_t *__restrict__ key, int64_t U, int D, double scale,
                                                                unsigned long long *__restrict__ sum, int32_t *__restrict__ cnt) {
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
    const float rf = r[i];
    unsigned long long v = 0;
    if (__builtin_isfinite(rf)) {
        const double t = __builtin_floor((double)rf * scale + 0.5);
        v = t > 0.0 ? (t < 255.0 ? (unsigned long long)t : 255ull) : 0ull;
    }
    atomicAdd(&sum[lo], v);
    atomicAdd(&cnt[lo], 1);
}

__global__ __launch_bounds__(AT_THREADS) void attr_mean_kernel(const unsigned long long *__restrict__ sum, const int32_t *__restrict__ cnt, int64_t U,
                                                               uint8_t *__restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= U) return;
    const unsigned long long c = (unsigned long long)(cnt[i] > 0 ? cnt[i] : 0);
    const unsigned long long m = c ? (2ull * sum[i] + c) / (2ull * c) : 0ull;
    a[i] = (uint8_t)(m > 255ull ? 255ull : m);
}

}  // namespace

extern "C" int64_t scp_attr_leaf_values_workspace_bytes(int64_t U) {
    if (U < 0 || U - 1 > (1ll << 31)) return SCP_EINVAL;
    return 16 * (U > 0 ? U : 1);
}

extern "C" int64_t scp_attr_forward_workspace_bytes(int64_t U, int32_t D) {
    at_layout L;
    return at_make_layout(U, D, L) ? L.bytes : (int64_t)SCP_EINVAL;
}

extern "C" int64_t scp_attr_inverse_workspace_bytes(int64_t U, int32_t D) { return scp_attr_forward_workspace_bytes(U, D); }

extern "C" int scp_attr_leaf_values(const int32_t *q, const float *r, int64_t P, const int32_t *leaves, int64_t U, int32_t D, int32_t scale,
                                    uint8_t *a, int32_t *cnt, void *workspace, int64_t workspace_bytes, void *stream) {
    if (P < 0 || P > (1ll << 31) || U < 0 || U - 1 > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH || scale < 1 || scale > (1 << 20)) return SCP_EINVAL;
    if ((P > 0 && (!q || !r)) || (U > 0 && (!leaves || !a || !cnt))) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, scp_attr_leaf_values_workspace_bytes(U))) return SCP_EINVAL;
    if (U == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    uint64_t *key = (uint64_t *)workspace;
    unsigned long long *sum = (unsigned long long *)workspace + U;
    HIP_TRY(hipMemsetAsync(sum, 0, (size_t)U * 8, st));
    HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)U * 4, st));
    hipLaunchKernelGGL(attr_keys_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, leaves, U, (int)D, key);
    LAUNCH_CHECK();
    if (P > 0) {
        hipLaunchKernelGGL(attr_point_kernel, dim3(at_grid(P, AT_THREADS)), dim3(AT_THREADS), 0, st, q, r, P, key, U, (int)D, (double)scale, sum, cnt);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(attr_mean_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, sum, cnt, U, a);
    LAUNCH_CHECK();
    return SCP_OK;
}

extern "C" int scp_attr_forward(const int32_t *leaves, const uint8_t *a, int64_t U, int32_t D, int32_t Q, int16_t *k, uint8_t *ctx, int32_t *root,
                                int32_t *hist, int64_t *level_counts, void *workspace, int64_t workspace_bytes, void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || Q < 1 || Q > 255) return SCP_EINVAL;
    if (!hist || !level_counts || !root || (U > 0 && (!leaves || !a)) || (U > 1 && (!k || !ctx))) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, L.bytes)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)D * AT_ALPHABET * 4, st));
    HIP_TRY(hipMemsetAsync(root, 0, 4, st));
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(level_counts, 0, (size_t)(D + 1) * 8, st));
        return SCP_OK;
    }
    uint8_t *ws = (uint8_t *)workspace;
    const int rc = at_build_tree(leaves, a, U, D, L, ws, st);
    if (rc) return rc;
    int64_t *counts = (int64_t *)(ws + L.b_counts);
    uint64_t *key = (uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w);
    int32_t *val = (int32_t *)(ws + L.b_val);
    for (int j = 1; j <= D; ++j) {
        hipLaunchKernelGGL(attr_lift_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, (uint32_t)Q, counts, first + L.off[j],
                           key + L.off[j - 1], w + L.off[j - 1], val + L.off[j - 1], w + L.off[j], val + L.off[j], k, ctx, hist, U - 1);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(attr_root_kernel, dim3(1), dim3(AT_THREADS), 0, st, val + L.off[D], root);
    LAUNCH_CHECK();
    HIP_TRY(hipMemcpyAsync(level_counts, counts, (size_t)(D + 1) * 8, hipMemcpyDeviceToDevice, st));
    return SCP_OK;
}

extern "C" int scp_attr_level_counts(const int32_t *leaves, int64_t U, int32_t D, int64_t *level_counts, void *workspace, int64_t workspace_bytes,
                                     void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || !level_counts || (U > 0 && !leaves)) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, L.bytes)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(level_counts, 0, (size_t)(D + 1) * 8, st));
        return SCP_OK;
    }
    const int rc = at_build_tree(leaves, nullptr, U, D, L, (uint8_t *)workspace, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(level_counts, (uint8_t *)workspace + L.b_counts, (size_t)(D + 1) * 8, hipMemcpyDeviceToDevice, st));
    return SCP_OK;
}

extern "C" int scp_attr_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, int32_t root, const int16_t *k, uint8_t *a, void *workspace,
                                int64_t workspace_bytes, void *stream) {
    at_layout L;
    if (!at_make_layout(U, D, L) || Q < 1 || Q > 255 || root < 0 || root > 255) return SCP_EINVAL;
    if ((U > 0 && (!leaves || !a)) || (U > 1 && !k)) return SCP_EINVAL;
    if (!at_ws_ok(workspace, workspace_bytes, L.bytes)) return SCP_EINVAL;
    if (U == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    const int rc = at_build_tree(leaves, nullptr, U, D, L, ws, st);
    if (rc) return rc;
    int64_t *counts = (int64_t *)(ws + L.b_counts);
    uint64_t *key = (uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w);
    int32_t *val = (int32_t *)(ws + L.b_val);
    for (int j = 1; j <= D; ++j) {
        hipLaunchKernelGGL(attr_weight_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, counts, first + L.off[j], w + L.off[j - 1],
                           w + L.off[j]);
        LAUNCH_CHECK();
    }
    for (int j = D; j >= 1; --j) {
        hipLaunchKernelGGL(attr_unlift_kernel, dim3(at_grid(L.cap[j], AT_THREADS)), dim3(AT_THREADS), 0, st, j, (int)D, (uint32_t)Q, root, counts,
                           first + L.off[j], key + L.off[j - 1], w + L.off[j - 1], val + L.off[j], val + L.off[j - 1], k, U - 1, a);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

extern "C" int scp_attr_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream) {
    if (n < 0 || n > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH || !tables) return SCP_EINVAL;
    if (n > 0 && (!k || !ctx || !lohi)) return SCP_EINVAL;
    if (n == 0) return SCP_OK;
    hipLaunchKernelGGL(attr_pairs_kernel, dim3(at_grid(n, AT_THREADS)), dim3(AT_THREADS), 0, (hipStream_t)stream, k, ctx, n, tables, (int)D, lohi);
    LAUNCH_CHECK();
    return SCP_OK;
}
