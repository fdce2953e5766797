// Colour layer ("Colour"): the RGB of an object cloud on the octree of its shell - per-leaf means, a reversible YCoCg-R
// transform and lift.h's engine on the three planes Y, Co, Cg at once with 1021 symbols, in exact integer arithmetic (gfx950).  The tree,
// the weights, the merge plan and the step of a pair are the reflectance layer's (csrc/attr.hip): one engine, instantiated twice.
//
//   scp_color_leaf_values  one thread per point: binary search of the point's cell among the leaf keys, three 64-bit integer atomic adds
//                          and the count; then one thread per leaf: the rounded means and their YCoCg-R image (int16, planar).
//   scp_color_forward      lift_forward on ycc int16 [3][U]: coefficients planar [3][U - 1] in the reflectance layer's coding order, one
//                          context array for the three planes, a histogram row per (channel, level).
//   scp_color_inverse      lift_inverse; a leaf undoes the colour transform and clamps R, G, B to 0 .. 255 - the only clamp of the layer.
//   scp_color_pairs        lift_pairs: the 3 (U - 1) coefficients in payload order (Y block, Co block, Cg block), table of context
//                          channel * D + (level - 1).
//   scp_color_sweep        lift_sweep: per step of a grid the histograms of scp_color_forward and the R, G, B error of scp_color_inverse's
//                          colours against the leaf means.
//
// Integer arithmetic only.  Unsorted or repeated leaves give unspecified values, but no access leaves the buffers, for the reflectance
// layer's reason: counts are clamped at the scan (attr_common.h).
#include "lift.h"

#define CL_ALPHABET 1021
#define CL_KMAX 510
#define CL_SWEEP_LDS 128        // symbols of a sweep row with LDS counters (|k| <= 64): 24 KB at 16 steps and three planes

namespace {

struct color_store {       // YCoCg-R back to R, G, B
    static constexpr int OUT = 3;
    static __device__ __forceinline__ void rule(const int32_t *x, int32_t *y) {
        const int32_t t = x[0] - (x[2] >> 1), G = x[2] + t, B = t - (x[1] >> 1), R = B + x[1];
        y[0] = R < 0 ? 0 : (R > 255 ? 255 : R);
        y[1] = G < 0 ? 0 : (G > 255 ? 255 : G);
        y[2] = B < 0 ? 0 : (B > 255 ? 255 : B);
    }
    static __device__ __forceinline__ void leaf(uint8_t *rgb, int64_t i, const int32_t *x) {
        int32_t y[OUT];
        rule(x, y);
        uint8_t *o = rgb + 3 * i;
        o[0] = (uint8_t)y[0];
        o[1] = (uint8_t)y[1];
        o[2] = (uint8_t)y[2];
    }
};

__global__ __launch_bounds__(AT_THREADS) void color_point_kernel(const int32_t *__restrict__ q, const uint8_t *__restrict__ rgb, int64_t P,
                                                                 const uint64_t *__restrict__ key, int64_t U, int D, unsigned long long *__restrict__ sum,
                                                                 int32_t *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= P) return;
    const int64_t leaf = at_find_leaf(key, U, q[3 * i], q[3 * i + 1], q[3 * i + 2], D);
    if (leaf < 0) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) atomicAdd(&sum[(int64_t)ch * U + leaf], (unsigned long long)rgb[3 * i + ch]);
    atomicAdd(&cnt[leaf], 1);
}

__global__ __launch_bounds__(AT_THREADS) void color_mean_kernel(const unsigned long long *__restrict__ sum, const int32_t *__restrict__ cnt, int64_t U,
                                                                uint8_t *__restrict__ rgb_mean, int16_t *__restrict__ ycc) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= U) return;
    int32_t m[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        m[ch] = at_round_mean(sum[(int64_t)ch * U + i], cnt[i]);
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
    return at_make_layout(U, D, L) ? lift_bytes<3>(L) : (int64_t)SCP_EINVAL;
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
    hipLaunchKernelGGL(attr_keys_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, leaves, U, (int)D, key, (uint32_t *)nullptr, (int64_t *)nullptr);
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
    return lift_forward<3, CL_ALPHABET, CL_KMAX>(leaves, ycc, U, D, Q, k, ctx, root, hist, level_counts, workspace, workspace_bytes, stream);
}

extern "C" int scp_color_inverse(const int32_t *leaves, int64_t U, int32_t D, int32_t Q, const int32_t *root, const int16_t *k, uint8_t *rgb,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    if (!root || root[0] < 0 || root[0] > 255 || root[1] < -255 || root[1] > 255 || root[2] < -255 || root[2] > 255) return SCP_EINVAL;
    return lift_inverse<3, color_store>(leaves, U, D, Q, lift_vec<3>{{root[0], root[1], root[2]}}, k, rgb, workspace, workspace_bytes, stream);
}

extern "C" int64_t scp_color_sweep_workspace_bytes(int64_t U, int32_t D, int32_t G) { return lift_sweep_bytes<3, CL_ALPHABET>(U, D, G); }

extern "C" int scp_color_sweep(const int32_t *leaves, const int16_t *ycc, const uint8_t *rgb_mean, int64_t U, int32_t D, const int32_t *steps,
                               int32_t G, int32_t *hist, uint64_t *sse, uint32_t *linf, int32_t *root, int64_t *level_counts, void *workspace,
                               int64_t workspace_bytes, void *stream) {
    return lift_sweep<3, CL_ALPHABET, CL_KMAX, CL_SWEEP_LDS, color_store>(leaves, ycc, rgb_mean, U, D, steps, G, hist, sse, linf, root, level_counts,
                                                                          workspace, workspace_bytes, stream);
}

extern "C" int scp_color_pairs(const int16_t *k, const uint8_t *ctx, int64_t n, const uint16_t *tables, int32_t D, uint32_t *lohi, void *stream) {
    return lift_pairs<3, CL_ALPHABET, CL_KMAX>(k, ctx, n, tables, D, lohi, stream);
}
