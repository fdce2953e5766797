// Reflectance layer ("Reflectance"): a region-adaptive hierarchical transform on the octree of a shell, in exact integer
// arithmetic (gfx950).  Encoder and decoder run the same integer steps on the same Morton-ordered leaf list, so they agree bit for bit.
// The tree is attr_common.h's, the transform lift.h's engine on one plane of 8-bit values with 511 symbols; here are the leaf values, the
// level-1 clamp and the entries.
//
//   scp_attr_leaf_values   one thread per point: 8-bit value of the reflectance, binary search of the point's cell among the leaf keys,
//                          integer atomic adds of (value, 1) on the leaf; then a = (2 sum + cnt) // (2 cnt) per leaf.
//   scp_attr_forward       lift_forward on a uint8 [U].
//   scp_attr_inverse       lift_inverse; a leaf keeps its value clamped to 0 .. 255.
//   scp_attr_level_counts  the tree alone: n_0 .. n_D, from which a decoder knows every coefficient's context before it has one.
//   scp_attr_pairs         lift_pairs: (c_low | c_high << 16) of every coefficient from the chosen table of its context.
//   scp_attr_sweep         lift_sweep: per step of a grid the histogram of scp_attr_forward and the error of scp_attr_inverse's values.
//
// Integer atomics only (leaf sums, histogram); no floating-point arithmetic except the one exact product r * scale of a point value.
// Unsorted or repeated leaves give unspecified values, but no access leaves the buffers: every level's count is clamped to the level's
// capacity where the scan produces it (attr_common.h), and the engine's indices all derive from those counts (lift.h).
#include "lift.h"

#define AT_ALPHABET 511
#define AT_KMAX 255
#define AT_SWEEP_LDS 256        // symbols of a sweep row with LDS counters (|k| <= 128): 16 KB at 16 steps

namespace {

struct attr_store {
    static constexpr int OUT = 1;
    static __device__ __forceinline__ void rule(const int32_t *x, int32_t *y) { y[0] = x[0] < 0 ? 0 : (x[0] > 255 ? 255 : x[0]); }
    static __device__ __forceinline__ void leaf(uint8_t *a, int64_t i, const int32_t *x) {
        int32_t y[OUT];
        rule(x, y);
        a[i] = (uint8_t)y[0];
    }
};

__global__ __launch_bounds__(AT_THREADS) void attr_point_kernel(const int32_t *__restrict__ q, const float *__restrict__ r, int64_t P,
                                                                const uint64_t *__restrict__ key, int64_t U, int D, double scale,
                                                                unsigned long long *__restrict__ sum, int32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= P) return;
    const int64_t leaf = at_find_leaf(key, U, q[3 * i], q[3 * i + 1], q[3 * i + 2], D);
    if (leaf < 0) return;
    const float rf = r[i];
    unsigned long long v = 0;
    if (__builtin_isfinite(rf)) {
        const double t = __builtin_floor((double)rf * scale + 0.5);
        v = t > 0.0 ? (t < 255.0 ? (unsigned long long)t : 255ull) : 0ull;
    }
    atomicAdd(&sum[leaf], v);
    atomicAdd(&cnt[leaf], 1);
}

__global__ __launch_bounds__(AT_THREADS) void attr_mean_kernel(const unsigned long long *__restrict__ sum, const int32_t *__restrict__ cnt, int64_t U,
                                                               uint8_t *__restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i < U) a[i] = (uint8_t)at_round_mean(sum[i], cnt[i]);
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
    hipLaunchKernelGGL(attr_keys_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, leaves, U, (int)D, key, (uint32_t *)nullptr, (int64_t *)nullptr);
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
    return lift_forward<1, AT_ALPHABET, AT_KMAX>(leaves, a, U, D, Q, k, ctx, root, hist, level_counts, workspace, workspace_bytes, stream);
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
    const int rc = at_build_tree(leaves, U, D, L, (uint8_t *)workspace, st);
    if (rc) return rc;
    HIP_TRY(at_copy_counts(level_counts, (const uint8_t *)workspace, L, D, st));
    return SCP_OK;
}

extern "C" int scp_attr_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, int32_t root, const int16_t *k, uint8_t *a, void *workspace,
                                int64_t workspace_bytes, void *stream) {
    if (root < 0 || root > 255) return SCP_EINVAL;
    return lift_inverse<1, attr_store>(leaves, U, D, Q, lift_vec<1>{{root}}, k, a, workspace, workspace_bytes, stream);
}

extern "C" int64_t scp_attr_sweep_workspace_bytes(int64_t U, int32_t D, int32_t G) { return lift_sweep_bytes<1, AT_ALPHABET>(U, D, G); }

extern "C" int scp_attr_sweep(const int32_t *leaves, const uint8_t *a, int64_t U, int32_t D, const int32_t *steps, int32_t G, int32_t *hist,
                              uint64_t *sse, uint32_t *linf, int32_t *root, int64_t *level_counts, void *workspace, int64_t workspace_bytes,
                              void *stream) {
    return lift_sweep<1, AT_ALPHABET, AT_KMAX, AT_SWEEP_LDS, attr_store>(leaves, a, a, U, D, steps, G, hist, sse, linf, root, level_counts, workspace,
                                                                         workspace_bytes, stream);
}

extern "C" int scp_attr_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream) {
    return lift_pairs<1, AT_ALPHABET, AT_KMAX>(k, ctx, n, tables, D, lohi, stream);
}
