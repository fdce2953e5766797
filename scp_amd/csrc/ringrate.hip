// Rate per range ring and depth report: every leaf's share of its ancestors' bits - all of them, or those of the first D - k levels -
// summed per (rho shell, range ring) bin (gfx950, float64).
//
// The rate report (rate.hip) says where the bits go per octree level, the distortion report (distreport.hip) where the error goes per
// range ring and shell.  A level is not a place: this file attributes the bits of every node to the points below it, so that the two
// reports meet on the same bins.  For one tree (one segment of a build; nodes in BFS order with occ / level / parent, depth D):
//   leaves(i) = popcount(occ_i) for a node of level D, the sum over the node's children otherwise        (integers)
//   share(i)  = bits(i) / double(leaves(i))                                                              (one IEEE float64 division)
//   cost(p)   = ((share(a_1) + share(a_2)) + ..) + share(a_D), a_l = the ancestor of leaf p at level l   (root first, float64, no fma)
//   leaf p    = in the order of scp_geom_emit_leaves: level-D node j owns the popcount(occ_j) consecutive leaves that start at the
//               exclusive prefix sum of the popcounts of the level-D nodes before it
//   bin       = group * n_rings + ring, ring = the largest r with rho2 >= edges_sq[r], rho2 = (x*x + y*y) + z*z of (point - view):
//               ring_bin of rate_common.h, which dr_split_kernel (distreport.hip) calls too.
//
// The depth report asks the same of a stream cut short: the symbols of levels 1 .. D - k describe the cloud at cell size 2^k, and
//   cost_k(p) = ((share(a_1) + share(a_2)) + ..) + share(a_{D-k})    for 0 <= k < D: the operations of cost(p), the chain cut short
//   cost_k(p) = +0.0                                                 for k >= D
// so cost_0 is cost, and cost_k(p) is the finished sum of p's ancestor at level D - k.  Plane k of the outputs holds cost_k.
//
// Order contract ("Rate per ring" and "Depth report"):
//   leaves:   integer atomics into the parent, one launch per level from the deepest up - exact, hence order-free;
//   cost:     one launch per level from the root down; a node adds its own share to its parent's finished sum - the order of the sum is
//             the order of the levels, no thread waits for another inside a launch.  The level-D launch writes plane 0;
//   planes:   for max_drop >= 1, ONE more launch in which every level-D node climbs up to max_drop parents and writes plane k of the
//             leaves it owns from the sum of the ancestor it stands on;
//   bin:      thread t of the (bin, plane)'s one workgroup adds rows t, t + 1024, .. of the bin in that order, then a fixed binary tree
//             over the 1024 partial sums (rate_common.h: the contract of rate.hip / distreport.hip).
// No floating-point atomics anywhere.  The number of launches (2 * deepest tree + 1, one more with max_drop >= 1) never depends on node
// or segment counts: all segments of a build go through the same launches (blockIdx.y = segment).
//
// The node table is the caller's, so nothing in it is trusted: a validation launch checks every node before any index is followed
// (rr_validate_kernel states what a well-formed table is) and the entry point returns SCP_EINVAL when it objects.
#include "rate_common.h"

#define RR_THREADS 256

struct rr_seg { int64_t node_base, n_nodes, depth, leaf_base, n_leaves; };

// A well-formed segment: the first node is the root (level 1, parent -1) and the only node of level 1; levels lie in 1 .. D and never
// fall along the table (BFS order); a node's parent lies inside the segment in front of the node, one level up; parents never fall
// along a level (siblings are neighbours); no occupancy byte is 0.  status[0] counts the nodes that break a rule, status[1 + s] is the
// popcount total of segment s's level-D nodes (the host compares it with the segment's leaf count).  With these rules the prefix
// offsets of rr_cost_kernel are exact, every leaf index it forms lies inside the segment's leaves, and a level-D node that climbs D - 1
// parents arrives at its root.
__global__ __launch_bounds__(RR_THREADS) void rr_validate_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                                 const int32_t *__restrict__ parent, const rr_seg *__restrict__ segs,
                                                                 unsigned long long *__restrict__ status) {
    __shared__ unsigned s_bad, s_pop;
    if (threadIdx.x == 0) { s_bad = 0u; s_pop = 0u; }
    __syncthreads();
    const rr_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (j < sg.n_nodes) {
        const int64_t i = sg.node_base + j;
        const int lv = level[i];
        const int64_t p = parent[i];
        const int o = occ[i];
        bool bad = lv < 1 || lv > sg.depth || o == 0;
        if (j == 0) {
            bad = bad || lv != 1 || p != -1;
        } else {
            bad = bad || lv < 2 || p < sg.node_base || p >= i;
            if (!bad) {
                const int lq = level[i - 1];
                bad = (int)level[p] != lv - 1 || lq > lv || (lq == lv && (int64_t)parent[i - 1] > p);
            }
        }
        if (bad) atomicAdd(&s_bad, 1u);
        else if (lv == sg.depth) atomicAdd(&s_pop, (unsigned)__popc(o));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad) atomicAdd(&status[0], (unsigned long long)s_bad);
        if (s_pop) atomicAdd(&status[1 + blockIdx.y], (unsigned long long)s_pop);
    }
}

// launch k: the nodes k levels above their tree's last level.  Their own count is final (the launch before added every child's): it goes
// to the parent.  The table was zeroed before launch 0, in which the last level stores its popcounts.
__global__ __launch_bounds__(RR_THREADS) void rr_leaves_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                               const int32_t *__restrict__ parent, const rr_seg *__restrict__ segs, int k,
                                                               int64_t *__restrict__ leaves) {
    const rr_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (j >= sg.n_nodes) return;
    const int64_t i = sg.node_base + j;
    if ((int64_t)level[i] != sg.depth - k) return;
    int64_t v;
    if (k == 0) {
        v = __popc((int)occ[i]);
        leaves[i] = v;
    } else {
        v = leaves[i];
    }
    if (j > 0) atomicAdd((unsigned long long *)(leaves + parent[i]), (unsigned long long)v);
}

// launch l: the nodes of level l.  off = the leaves in front of the node on its level = the parent's offset plus the earlier siblings'
// leaves (siblings are neighbours: at most seven nodes back); acc = the parent's sum plus the node's own share, so that the sum runs
// root first.  A node of the last level writes the sum to the leaves it owns.
__global__ __launch_bounds__(RR_THREADS) void rr_cost_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                             const int32_t *__restrict__ parent, const rr_seg *__restrict__ segs, int l,
                                                             const int64_t *__restrict__ leaves, const double *__restrict__ bits_ideal,
                                                             const double *__restrict__ bits_table, int64_t *__restrict__ off,
                                                             double *__restrict__ acc_ideal, double *__restrict__ acc_table,
                                                             double *__restrict__ cost_ideal, double *__restrict__ cost_table) {
    const rr_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (j >= sg.n_nodes) return;
    const int64_t i = sg.node_base + j;
    if ((int)level[i] != l) return;
    const double n = (double)leaves[i];
    double ai = bits_ideal[i] / n, at = bits_table[i] / n;
    int64_t o = 0;
    if (j > 0) {
        const int32_t p = parent[i];
        o = off[p];
        for (int64_t q = i - 1; q > sg.node_base && i - q <= 7 && parent[q] == p; --q) o += leaves[q];
        ai = acc_ideal[p] + ai;
        at = acc_table[p] + at;
    }
    off[i] = o;
    acc_ideal[i] = ai;
    acc_table[i] = at;
    if ((int64_t)l == sg.depth) {
        const int cnt = __popc((int)occ[i]);
        if (o >= 0 && o + cnt <= sg.n_leaves) {        // (holds for every table the validation launch lets through)
            for (int c = 0; c < cnt; ++c) {
                cost_ideal[sg.leaf_base + o + c] = ai;
                cost_table[sg.leaf_base + o + c] = at;
            }
        }
    }
}

// one launch after the last level, for max_drop >= 1: a level-D node stands on its ancestor of level D - k after k steps up and writes
// that node's sum to plane k of its leaves; past the root (k >= D) the plane holds +0.0.  Plane 0 is rr_cost_kernel's.
__global__ __launch_bounds__(RR_THREADS) void rr_planes_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                               const int32_t *__restrict__ parent, const rr_seg *__restrict__ segs,
                                                               int max_drop, int64_t total_leaves, const int64_t *__restrict__ off,
                                                               const double *__restrict__ acc_ideal, const double *__restrict__ acc_table,
                                                               double *__restrict__ cost_ideal, double *__restrict__ cost_table) {
    const rr_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (j >= sg.n_nodes) return;
    const int64_t i = sg.node_base + j;
    if ((int64_t)level[i] != sg.depth) return;
    const int cnt = __popc((int)occ[i]);
    const int64_t o = off[i];
    if (o < 0 || o + cnt > sg.n_leaves) return;            // (never for a table the validation launch lets through)
    int64_t a = i;
    for (int k = 1; k <= max_drop; ++k) {
        a = a > sg.node_base ? (int64_t)parent[a] : -1;    // the root is the segment's first node: the climb ends there
        double vi = 0.0, vt = 0.0;
        if (a >= sg.node_base) {
            vi = acc_ideal[a];
            vt = acc_table[a];
        }
        double *pi = cost_ideal + (int64_t)k * total_leaves + sg.leaf_base + o;
        double *pt = cost_table + (int64_t)k * total_leaves + sg.leaf_base + o;
        for (int c = 0; c < cnt; ++c) {
            pi[c] = vi;
            pt[c] = vt;
        }
    }
}

// one thread per point
__global__ __launch_bounds__(RR_THREADS) void rr_bins_kernel(const double *__restrict__ a, int64_t n, double vx, double vy, double vz,
                                                             ring_edges edges, int n_rings, const int *__restrict__ group, int n_groups,
                                                             int *__restrict__ bin, uint8_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (i >= n) return;
    double s2, rho2;
    int f = 0;
    bin[i] = ring_bin(a[3 * i] - vx, a[3 * i + 1] - vy, a[3 * i + 2] - vz, edges, n_rings, group ? group[i] : 0, n_groups, s2, rho2, f);
    if (flag) flag[i] = (uint8_t)f;
}

// one workgroup per (bin, plane): plane blockIdx.y of the costs starts at blockIdx.y * plane_stride
__global__ __launch_bounds__(RATE_SEG_THREADS) void rr_segments_kernel(const double *__restrict__ cost_ideal, const double *__restrict__ cost_table,
                                                                       const int64_t *__restrict__ order, int64_t n,
                                                                       const int64_t *__restrict__ seg_off, int64_t plane_stride,
                                                                       scp_share_seg *__restrict__ out) {
    __shared__ double s_ideal[RATE_SEG_THREADS], s_table[RATE_SEG_THREADS];
    __shared__ rate_max s_mx[RATE_SEG_THREADS];
    __shared__ int s_rows[RATE_SEG_THREADS];
    const int t = threadIdx.x;
    const double *ci = cost_ideal + (int64_t)blockIdx.y * plane_stride, *ct = cost_table + (int64_t)blockIdx.y * plane_stride;
    // the order lives in device memory like the offsets, so nobody has checked it: a row outside the table is skipped
    int64_t lo, hi;
    rate_seg_bounds(seg_off, blockIdx.x, n, lo, hi);
    double ideal = 0.0, table = 0.0, mx = 0.0;
    int rows = 0;
    for (int64_t p = lo + t; p < hi; p += RATE_SEG_THREADS) {
        const int64_t i = order ? order[p] : p;
        if (i < 0 || i >= n) continue;
        const double c = ci[i];
        ++rows;
        ideal += c;
        table += ct[i];
        mx = c > mx ? c : mx;
    }
    s_ideal[t] = ideal; s_table[t] = table; s_mx[t].v = mx; s_rows[t] = rows;
    rate_block_tree(t, s_ideal, s_table, s_mx, s_rows);
    if (t == 0) {
        scp_share_seg o;
        o.leaves = s_rows[0];
        o.ideal_bits = s_ideal[0];
        o.table_bits = s_table[0];
        o.max_ideal_bits = s_mx[0].v;
        out[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = o;
    }
}

static inline int64_t rr_align(int64_t b) { return (b + 255) / 256 * 256; }
static inline int64_t rr_head_bytes(int32_t nseg) { return rr_align((int64_t)nseg * (int64_t)sizeof(rr_seg) + (1 + (int64_t)nseg) * 8); }

extern "C" SCP_API int64_t scp_rate_leaf_share_workspace_bytes(int64_t total_nodes, int32_t nseg) {
    if (total_nodes < 1 || total_nodes > SCP_SHARE_MAX_NODES || nseg < 1 || nseg > SCP_MAX_SEGMENTS) return SCP_EINVAL;
    return rr_head_bytes(nseg) + 3 * rr_align(8 * total_nodes);      // segment table + status | off | acc_ideal | acc_table
}

extern "C" SCP_API int64_t scp_rate_depth_share_workspace_bytes(int64_t total_nodes, int32_t nseg) {
    return scp_rate_leaf_share_workspace_bytes(total_nodes, nseg);
}

// the tree pass of both entry points: planes 0 .. max_drop of cost_ideal / cost_table, total_leaves apart
static int rr_tree_pass(const uint8_t *occ, const uint8_t *level, const int32_t *parent, int64_t total_nodes, const double *bits_ideal,
                        const double *bits_table, const int64_t *segs, int32_t nseg, int64_t total_leaves, int32_t max_drop, int64_t *leaves,
                        double *cost_ideal, double *cost_table, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!occ || !level || !parent || !bits_ideal || !bits_table || !segs || !leaves || !cost_ideal || !cost_table || !workspace) return SCP_EINVAL;
    if (total_nodes < 1 || total_nodes > SCP_SHARE_MAX_NODES || total_leaves < 1 || total_leaves > SCP_SHARE_MAX_NODES) return SCP_EINVAL;
    if (nseg < 1 || nseg > SCP_MAX_SEGMENTS || (((uintptr_t)workspace) & 7) || max_drop < 0 || max_drop > SCP_MAX_DEPTH) return SCP_EINVAL;
    if (workspace_bytes < scp_rate_leaf_share_workspace_bytes(total_nodes, nseg)) return SCP_EINVAL;
    // the segments tile the node table and the leaf table, in this order, each with at least one node and one leaf
    rr_seg host[SCP_MAX_SEGMENTS];
    int64_t node = 0, leaf = 0, max_nodes = 0;
    int max_depth = 0;
    for (int s = 0; s < nseg; ++s) {
        const int64_t *row = segs + 4 * s;
        const int64_t next_leaf = s + 1 < nseg ? segs[4 * (s + 1) + 3] : total_leaves;
        if (row[0] != node || row[1] < 1 || row[1] > total_nodes - node || row[2] < 1 || row[2] > SCP_MAX_DEPTH) return SCP_EINVAL;
        if (row[3] != leaf || next_leaf <= leaf || next_leaf > total_leaves) return SCP_EINVAL;
        host[s].node_base = row[0]; host[s].n_nodes = row[1]; host[s].depth = row[2]; host[s].leaf_base = row[3]; host[s].n_leaves = next_leaf - leaf;
        node += row[1];
        leaf = next_leaf;
        max_nodes = row[1] > max_nodes ? row[1] : max_nodes;
        max_depth = (int)row[2] > max_depth ? (int)row[2] : max_depth;
    }
    if (node != total_nodes || leaf != total_leaves) return SCP_EINVAL;

    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace;
    rr_seg *d_segs = (rr_seg *)ws;
    unsigned long long *d_status = (unsigned long long *)(ws + (size_t)nseg * sizeof(rr_seg));
    int64_t *off = (int64_t *)(ws + rr_head_bytes(nseg));
    double *acc_ideal = (double *)(ws + rr_head_bytes(nseg) + rr_align(8 * total_nodes));
    double *acc_table = (double *)(ws + rr_head_bytes(nseg) + 2 * rr_align(8 * total_nodes));
    HIP_TRY(hipMemcpyAsync(d_segs, host, (size_t)nseg * sizeof(rr_seg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)(1 + nseg) * 8, st));
    const dim3 grid((unsigned)cdiv64(max_nodes, RR_THREADS), (unsigned)nseg);
    hipLaunchKernelGGL(rr_validate_kernel, grid, dim3(RR_THREADS), 0, st, occ, level, parent, d_segs, d_status);
    LAUNCH_CHECK();
    unsigned long long status[1 + SCP_MAX_SEGMENTS];
    HIP_TRY(hipMemcpyAsync(status, d_status, (size_t)(1 + nseg) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status[0] != 0ull) return SCP_EINVAL;
    for (int s = 0; s < nseg; ++s)
        if (status[1 + s] != (unsigned long long)host[s].n_leaves) return SCP_EINVAL;

    HIP_TRY(hipMemsetAsync(leaves, 0, (size_t)total_nodes * 8, st));
    for (int k = 0; k < max_depth; ++k) {
        hipLaunchKernelGGL(rr_leaves_kernel, grid, dim3(RR_THREADS), 0, st, occ, level, parent, d_segs, k, leaves);
        LAUNCH_CHECK();
    }
    for (int l = 1; l <= max_depth; ++l) {
        hipLaunchKernelGGL(rr_cost_kernel, grid, dim3(RR_THREADS), 0, st, occ, level, parent, d_segs, l, leaves, bits_ideal, bits_table, off,
                           acc_ideal, acc_table, cost_ideal, cost_table);
        LAUNCH_CHECK();
    }
    if (max_drop >= 1) {
        hipLaunchKernelGGL(rr_planes_kernel, grid, dim3(RR_THREADS), 0, st, occ, level, parent, d_segs, (int)max_drop, total_leaves, off, acc_ideal,
                           acc_table, cost_ideal, cost_table);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

/* leaves per node and every leaf's share of its ancestors' bits: see include/scp.h */
extern "C" SCP_API int scp_rate_leaf_share(const uint8_t *occ, const uint8_t *level, const int32_t *parent, int64_t total_nodes,
                                           const double *bits_ideal, const double *bits_table, const int64_t *segs, int32_t nseg,
                                           int64_t total_leaves, int64_t *leaves, double *cost_ideal, double *cost_table, void *workspace,
                                           int64_t workspace_bytes, void *stream) {
    return rr_tree_pass(occ, level, parent, total_nodes, bits_ideal, bits_table, segs, nseg, total_leaves, 0, leaves, cost_ideal, cost_table,
                        workspace, workspace_bytes, stream);
}

/* every leaf's share of the bits of levels 1 .. D - k, k = 0 .. max_drop: see include/scp.h */
extern "C" SCP_API int scp_rate_depth_share(const uint8_t *occ, const uint8_t *level, const int32_t *parent, int64_t total_nodes,
                                            const double *bits_ideal, const double *bits_table, const int64_t *segs, int32_t nseg,
                                            int64_t total_leaves, int32_t max_drop, int64_t *leaves, double *cost_ideal, double *cost_table,
                                            void *workspace, int64_t workspace_bytes, void *stream) {
    return rr_tree_pass(occ, level, parent, total_nodes, bits_ideal, bits_table, segs, nseg, total_leaves, max_drop, leaves, cost_ideal,
                        cost_table, workspace, workspace_bytes, stream);
}

/* (group, ring) bin per point: see include/scp.h */
extern "C" SCP_API int scp_ring_bins_f64(const double *xyz, int64_t n, const double *view, const double *edges_sq, int32_t n_rings,
                                         const int32_t *group, int32_t n_groups, int32_t *bin_out, uint8_t *flag_out, void *stream) {
    if (!xyz || !view || !bin_out || n <= 0 || n > SCP_DIST_MAX_POINTS || n_groups < 1) return SCP_EINVAL;
    if (!ring_edges_ok(edges_sq, n_rings) || (int64_t)n_groups * n_rings > SCP_DIST_MAX_BINS || !ring_view_ok(view)) return SCP_EINVAL;
    hipLaunchKernelGGL(rr_bins_kernel, dim3((unsigned)cdiv64(n, RR_THREADS)), dim3(RR_THREADS), 0, (hipStream_t)stream, xyz, n, view[0], view[1], view[2],
                       ring_edges_arg(edges_sq, n_rings), (int)n_rings, group, (int)n_groups, bin_out, flag_out);
    LAUNCH_CHECK();
    return SCP_OK;
}

/* per-(depth, bin) records of bin-ordered leaf cost planes: see include/scp.h */
extern "C" SCP_API int scp_share_segments_depth_f64(const double *cost_ideal, const double *cost_table, const int64_t *order, int64_t n,
                                                    const int64_t *seg_off, int32_t n_bins, int32_t n_depths, int64_t plane_stride,
                                                    scp_share_seg *out, void *stream) {
    if (!cost_ideal || !cost_table || !seg_off || !out || n <= 0 || n > SCP_DIST_MAX_POINTS || n_bins < 1 || n_bins > SCP_DIST_MAX_BINS) return SCP_EINVAL;
    if (n_depths < 1 || n_depths > SCP_MAX_DEPTH + 1 || plane_stride < n || plane_stride > SCP_SHARE_MAX_NODES) return SCP_EINVAL;
    hipLaunchKernelGGL(rr_segments_kernel, dim3((unsigned)n_bins, (unsigned)n_depths), dim3(RATE_SEG_THREADS), 0, (hipStream_t)stream, cost_ideal,
                       cost_table, order, n, seg_off, plane_stride, out);
    LAUNCH_CHECK();
    return SCP_OK;
}

/* per-bin records of bin-ordered leaf costs, the one-plane launch: see include/scp.h */
extern "C" SCP_API int scp_share_segments_f64(const double *cost_ideal, const double *cost_table, const int64_t *order, int64_t n,
                                              const int64_t *seg_off, int32_t n_bins, scp_share_seg *out, void *stream) {
    return scp_share_segments_depth_f64(cost_ideal, cost_table, order, n, seg_off, n_bins, 1, n, out, stream);
}
