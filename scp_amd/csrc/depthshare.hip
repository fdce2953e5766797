// Depth report: what the first D - k levels of every tree cost, per leaf and per (rho shell, range ring) bin, for k = 0 .. max_drop
// (gfx950, float64).
//
// An octree stream is progressive: the symbols of levels 1 .. D - k describe the cloud at cell size 2^k.  ringrate.hip hands every node's
// bits to the leaves below it and adds a leaf's ancestors root first; cut that chain short and the sum is what the leaf pays for the
// first D - k levels.  With leaves(i), share(i) and the leaf order of ringrate.hip (one tree = one segment of a build, depth D):
//   cost_k(p) = ((share(a_1) + share(a_2)) + ..) + share(a_{D-k})    for 0 <= k < D: the operations of cost(p), the chain cut short
//   cost_k(p) = +0.0                                                 for k >= D
// so cost_0 is scp_rate_leaf_share's cost bit for bit, and cost_k(p) is the finished sum of p's ancestor at level D - k.
//
// Order contract ("Depth report"): leaves and the per-node sums exactly as in ringrate.hip (integer atomics bottom-up, one
// launch per level; sums top-down, one launch per level, a node adding its share to its parent's finished sum); then ONE launch in which
// every level-D node climbs up to max_drop parents and writes plane k of the leaves it owns from the sum of the ancestor it stands on.
// The number of launches (2 * deepest tree + 2) depends on the depths alone: not on node counts, segment counts or max_drop.  No
// floating-point atomics.  The bins' sums follow the contract of rr_segments_kernel, one workgroup per (bin, depth).
//
// The node table is the caller's: it is validated on the device, by the rules of ringrate.hip, before any index in it is followed.
#include "scp_internal.h"

#define DS_THREADS 256
#define DS_SEG_THREADS 1024

struct ds_seg { int64_t node_base, n_nodes, depth, leaf_base, n_leaves; };

// The rules of rr_validate_kernel (ringrate.hip): the first node is the root (level 1, parent -1) and the only node of level 1; levels
// lie in 1 .. D and never fall along the table; a parent lies inside the segment in front of its child, one level up; parents never fall
// along a level; no occupancy byte is 0.  status[0] counts the nodes that break a rule, status[1 + s] is the popcount total of segment
// s's level-D nodes.  A table that passes lets a level-D node climb D - 1 parents and arrive at its root.
__global__ __launch_bounds__(DS_THREADS) void ds_validate_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                                 const int32_t *__restrict__ parent, const ds_seg *__restrict__ segs,
                                                                 unsigned long long *__restrict__ status) {
    __shared__ unsigned s_bad, s_pop;
    if (threadIdx.x == 0) { s_bad = 0u; s_pop = 0u; }
    __syncthreads();
    const ds_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
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

// launch k: the nodes k levels above their tree's last level hand their finished count to the parent (rr_leaves_kernel)
__global__ __launch_bounds__(DS_THREADS) void ds_leaves_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                               const int32_t *__restrict__ parent, const ds_seg *__restrict__ segs, int k,
                                                               int64_t *__restrict__ leaves) {
    const ds_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
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

// launch l: the nodes of level l.  off = the leaves in front of the node on its level, acc = the parent's finished sum plus the node's
// own share (rr_cost_kernel's expressions on the same operands: acc of a level-D node is cost(p) of the leaves it owns).
__global__ __launch_bounds__(DS_THREADS) void ds_acc_kernel(const uint8_t *__restrict__ level, const int32_t *__restrict__ parent,
                                                            const ds_seg *__restrict__ segs, int l, const int64_t *__restrict__ leaves,
                                                            const double *__restrict__ bits_ideal, const double *__restrict__ bits_table,
                                                            int64_t *__restrict__ off, double *__restrict__ acc_ideal,
                                                            double *__restrict__ acc_table) {
    const ds_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
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
}

// one launch after the last level: a level-D node stands on its ancestor of level D - k after k steps up and writes that node's sum to
// plane k of its leaves; past the root (k >= D) the plane holds +0.0
__global__ __launch_bounds__(DS_THREADS) void ds_planes_kernel(const uint8_t *__restrict__ occ, const uint8_t *__restrict__ level,
                                                               const int32_t *__restrict__ parent, const ds_seg *__restrict__ segs,
                                                               int max_drop, int64_t total_leaves, const int64_t *__restrict__ off,
                                                               const double *__restrict__ acc_ideal, const double *__restrict__ acc_table,
                                                               double *__restrict__ cost_ideal, double *__restrict__ cost_table) {
    const ds_seg sg = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * DS_THREADS + threadIdx.x;
    if (j >= sg.n_nodes) return;
    const int64_t i = sg.node_base + j;
    if ((int64_t)level[i] != sg.depth) return;
    const int cnt = __popc((int)occ[i]);
    const int64_t o = off[i];
    if (o < 0 || o + cnt > sg.n_leaves) return;            // (never for a table the validation launch lets through)
    int64_t a = i;
    for (int k = 0; k <= max_drop; ++k) {
        double vi = 0.0, vt = 0.0;
        if (a >= sg.node_base) {
            vi = acc_ideal[a];
            vt = acc_table[a];
            a = a > sg.node_base ? (int64_t)parent[a] : -1;       // the root is the segment's first node: the climb ends there
        }
        double *pi = cost_ideal + (int64_t)k * total_leaves + sg.leaf_base + o;
        double *pt = cost_table + (int64_t)k * total_leaves + sg.leaf_base + o;
        for (int c = 0; c < cnt; ++c) {
            pi[c] = vi;
            pt[c] = vt;
        }
    }
}

// one workgroup per (bin, depth): rr_segments_kernel on plane blockIdx.y
__global__ __launch_bounds__(DS_SEG_THREADS) void ds_segments_kernel(const double *__restrict__ cost_ideal, const double *__restrict__ cost_table,
                                                                     const int64_t *__restrict__ order, int64_t n,
                                                                     const int64_t *__restrict__ seg_off, int64_t plane_stride,
                                                                     scp_share_seg *__restrict__ out) {
    __shared__ double s_ideal[DS_SEG_THREADS], s_table[DS_SEG_THREADS], s_mx[DS_SEG_THREADS];
    __shared__ int s_rows[DS_SEG_THREADS];
    const int t = threadIdx.x;
    const double *ci = cost_ideal + (int64_t)blockIdx.y * plane_stride, *ct = cost_table + (int64_t)blockIdx.y * plane_stride;
    // the offsets and the order live in device memory, so nobody has checked them: clamped to the table, a row outside it is skipped
    int64_t lo = seg_off[blockIdx.x], hi = seg_off[blockIdx.x + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    double ideal = 0.0, table = 0.0, mx = 0.0;
    int rows = 0;
    for (int64_t p = lo + t; p < hi; p += DS_SEG_THREADS) {
        const int64_t i = order ? order[p] : p;
        if (i < 0 || i >= n) continue;
        const double c = ci[i];
        ++rows;
        ideal += c;
        table += ct[i];
        mx = c > mx ? c : mx;
    }
    s_ideal[t] = ideal; s_table[t] = table; s_mx[t] = mx; s_rows[t] = rows;
    __syncthreads();
    for (int h = DS_SEG_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) {
            s_ideal[t] += s_ideal[t + h];
            s_table[t] += s_table[t + h];
            s_mx[t] = s_mx[t + h] > s_mx[t] ? s_mx[t + h] : s_mx[t];
            s_rows[t] += s_rows[t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        scp_share_seg o;
        o.leaves = s_rows[0];
        o.ideal_bits = s_ideal[0];
        o.table_bits = s_table[0];
        o.max_ideal_bits = s_mx[0];
        out[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = o;
    }
}

static inline int64_t ds_align(int64_t b) { return (b + 255) / 256 * 256; }
static inline int64_t ds_head_bytes(int32_t nseg) { return ds_align((int64_t)nseg * (int64_t)sizeof(ds_seg) + (1 + (int64_t)nseg) * 8); }

extern "C" SCP_API int64_t scp_rate_depth_share_workspace_bytes(int64_t total_nodes, int32_t nseg) {
    if (total_nodes < 1 || total_nodes > SCP_SHARE_MAX_NODES || nseg < 1 || nseg > SCP_MAX_SEGMENTS) return SCP_EINVAL;
    return ds_head_bytes(nseg) + 3 * ds_align(8 * total_nodes);      // segment table + status | off | acc_ideal | acc_table
}

/* every leaf's share of the bits of levels 1 .. D - k, k = 0 .. max_drop: see include/scp.h */
extern "C" SCP_API int scp_rate_depth_share(const uint8_t *occ, const uint8_t *level, const int32_t *parent, int64_t total_nodes,
                                            const double *bits_ideal, const double *bits_table, const int64_t *segs, int32_t nseg,
                                            int64_t total_leaves, int32_t max_drop, int64_t *leaves, double *cost_ideal, double *cost_table,
                                            void *workspace, int64_t workspace_bytes, void *stream) {
    if (!occ || !level || !parent || !bits_ideal || !bits_table || !segs || !leaves || !cost_ideal || !cost_table || !workspace) return SCP_EINVAL;
    if (total_nodes < 1 || total_nodes > SCP_SHARE_MAX_NODES || total_leaves < 1 || total_leaves > SCP_SHARE_MAX_NODES) return SCP_EINVAL;
    if (nseg < 1 || nseg > SCP_MAX_SEGMENTS || (((uintptr_t)workspace) & 7) || max_drop < 0 || max_drop > SCP_MAX_DEPTH) return SCP_EINVAL;
    if (workspace_bytes < scp_rate_depth_share_workspace_bytes(total_nodes, nseg)) return SCP_EINVAL;
    // the segments tile the node table and the leaf table, in this order, each with at least one node and one leaf
    ds_seg host[SCP_MAX_SEGMENTS];
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
    ds_seg *d_segs = (ds_seg *)ws;
    unsigned long long *d_status = (unsigned long long *)(ws + (size_t)nseg * sizeof(ds_seg));
    int64_t *off = (int64_t *)(ws + ds_head_bytes(nseg));
    double *acc_ideal = (double *)(ws + ds_head_bytes(nseg) + ds_align(8 * total_nodes));
    double *acc_table = (double *)(ws + ds_head_bytes(nseg) + 2 * ds_align(8 * total_nodes));
    HIP_TRY(hipMemcpyAsync(d_segs, host, (size_t)nseg * sizeof(ds_seg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_status, 0, (size_t)(1 + nseg) * 8, st));
    const dim3 grid((unsigned)cdiv64(max_nodes, DS_THREADS), (unsigned)nseg);
    hipLaunchKernelGGL(ds_validate_kernel, grid, dim3(DS_THREADS), 0, st, occ, level, parent, d_segs, d_status);
    LAUNCH_CHECK();
    unsigned long long status[1 + SCP_MAX_SEGMENTS];
    HIP_TRY(hipMemcpyAsync(status, d_status, (size_t)(1 + nseg) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (status[0] != 0ull) return SCP_EINVAL;
    for (int s = 0; s < nseg; ++s)
        if (status[1 + s] != (unsigned long long)host[s].n_leaves) return SCP_EINVAL;

    HIP_TRY(hipMemsetAsync(leaves, 0, (size_t)total_nodes * 8, st));
    for (int k = 0; k < max_depth; ++k) {
        hipLaunchKernelGGL(ds_leaves_kernel, grid, dim3(DS_THREADS), 0, st, occ, level, parent, d_segs, k, leaves);
        LAUNCH_CHECK();
    }
    for (int l = 1; l <= max_depth; ++l) {
        hipLaunchKernelGGL(ds_acc_kernel, grid, dim3(DS_THREADS), 0, st, level, parent, d_segs, l, leaves, bits_ideal, bits_table, off, acc_ideal,
                           acc_table);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ds_planes_kernel, grid, dim3(DS_THREADS), 0, st, occ, level, parent, d_segs, (int)max_drop, total_leaves, off, acc_ideal,
                       acc_table, cost_ideal, cost_table);
    LAUNCH_CHECK();
    return SCP_OK;
}

/* per-(depth, bin) records of bin-ordered leaf cost planes: see include/scp.h */
extern "C" SCP_API int scp_share_segments_depth_f64(const double *cost_ideal, const double *cost_table, const int64_t *order, int64_t n,
                                                    const int64_t *seg_off, int32_t n_bins, int32_t n_depths, int64_t plane_stride,
                                                    scp_share_seg *out, void *stream) {
    if (!cost_ideal || !cost_table || !seg_off || !out || n <= 0 || n > SCP_DIST_MAX_POINTS || n_bins < 1 || n_bins > SCP_DIST_MAX_BINS) return SCP_EINVAL;
    if (n_depths < 1 || n_depths > SCP_MAX_DEPTH + 1 || plane_stride < n || plane_stride > SCP_SHARE_MAX_NODES) return SCP_EINVAL;
    hipLaunchKernelGGL(ds_segments_kernel, dim3((unsigned)n_bins, (unsigned)n_depths), dim3(DS_SEG_THREADS), 0, (hipStream_t)stream, cost_ideal,
                       cost_table, order, n, seg_off, plane_stride, out);
    LAUNCH_CHECK();
    return SCP_OK;
}
