// Distortion report: where a frame's error goes - per range ring and shell, split along the sensor's spherical axes (gfx950, float64).
//
// The rate report (rate.hip) says where the bits go; the three scalars of --metrics (chamfer, D1, D2) say nothing about where the error
// goes, although the codec quantises (rho, phi, theta) and gives the far shells finer steps in order to shape error over range.  For
// every query point a_i against a searched cloud B this file finds
//   j*(i)  = the LOWEST j with d2(i, j) == min_j d2(i, j) bit for bit,  d2 = (dx*dx + dy*dy) + dz*dz,  dx = a_i.x - b_j.x ... - the
//            expression of metrics.hip (both files are compiled with -ffp-contract=off), so the minimum scp_nn_sqdist_f64 stores is
//            reproduced exactly;
//   e      = b_j* - a_i in the local frame of a_i as seen from `view`: with (x, y, z) = a_i - view, s2 = x*x + y*y, s = sqrt(s2),
//            rho2 = s2 + z*z, rho = sqrt(rho2):  r^ = (x, y, z) / rho,  phi^ = (-y, x, 0) / s,  theta^ = (x z, y z, -s2) / (rho s)
//            (the direction of growing polar angle arccos(z / rho));  e_r = e . r^, e_phi = e . phi^, e_theta = e . theta^.
//            A query with s == 0 (on the sensor's axis, or at the sensor) has no such frame: an AXIS point, components 0, flagged;
//   bin    = group[i] * n_rings + ring(i),  ring(i) = the largest r with rho2 >= E_r * E_r  (decided on rho2: no sqrt takes part).
// The segment kernel then reduces rows brought into bin order into one scp_dist_seg record per bin.
//
// Order contract ("Distortion report"), as in rate.hip:
//   neighbour: the minimum is an integer atomicMin over the non-negative doubles' bit patterns (scp_nn_sqdist_f64), the index an integer
//              atomicMin among the pairs that reproduce that minimum - both exact and order-free, so j* does not depend on how the launch
//              splits B over workgroups or on the order in which tiles are visited;
//   bin:       thread t of the bin's one workgroup adds rows t, t + 1024, .. of the bin in that order, then a fixed binary tree over the
//              1024 partial sums - a function of the bin's rows in index order and of nothing else.
// No floating-point atomics anywhere.  rows, axis_rows, max_sq and hist are exact by nature (the histogram uses integer LDS atomics).
#include "rate_common.h"

#define DR_TILE 1024
#define DR_NO_INDEX 0x7FFFFFFF

__global__ __launch_bounds__(256) void dr_init_kernel(int *__restrict__ idx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) idx[i] = DR_NO_INDEX;
}

// the layout of nn_sqdist_f64_kernel: 256 queries per workgroup, B streamed through LDS in tiles of 1024, blockIdx.y splits B.  j runs
// upwards inside a slice, so the first pair that reproduces the minimum is the slice's lowest; the slices meet in an integer atomicMin.
__global__ __launch_bounds__(256) void dr_nn_index_kernel(const double *__restrict__ a, int64_t na, const double *__restrict__ b, int64_t nb,
                                                          const double *__restrict__ dmin, int *__restrict__ idx) {
    __shared__ double sb[DR_TILE * 3];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t ic = i < na ? i : na - 1;
    const double ax = a[3 * ic], ay = a[3 * ic + 1], az = a[3 * ic + 2];
    const double mine = dmin[ic];
    const int64_t per = ((nb + gridDim.y - 1) / gridDim.y + DR_TILE - 1) / DR_TILE * DR_TILE;
    const int64_t b0 = (int64_t)blockIdx.y * per, b1 = (b0 + per < nb) ? b0 + per : nb;
    int best = DR_NO_INDEX;
    for (int64_t t0 = b0; t0 < b1; t0 += DR_TILE) {
        const int cnt = (int)((b1 - t0) < DR_TILE ? (b1 - t0) : DR_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 3; e += 256) sb[e] = b[3 * t0 + e];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const double dx = ax - sb[3 * j], dy = ay - sb[3 * j + 1], dz = az - sb[3 * j + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            const int cand = (int)t0 + j;
            best = (d == mine && cand < best) ? cand : best;
        }
    }
    if (i < na && best != DR_NO_INDEX) atomicMin(idx + i, best);
}

// one thread per query: the error vector in the local frame, the bin, the flags
__global__ __launch_bounds__(256) void dr_split_kernel(const double *__restrict__ a, int64_t na, const double *__restrict__ b, int64_t nb,
                                                       double vx, double vy, double vz, ring_edges edges, int n_rings,
                                                       const int *__restrict__ group, int n_groups, int *__restrict__ idx,
                                                       double *__restrict__ d2, double *__restrict__ comp, int *__restrict__ bin,
                                                       uint8_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= na) return;
    const double ax = a[3 * i], ay = a[3 * i + 1], az = a[3 * i + 2];
    int f = 0;
    int j = idx[i];
    double ex = 0.0, ey = 0.0, ez = 0.0;
    if (j < 0 || (int64_t)j >= nb) {
        // no pair reproduced the minimum: only a non-finite coordinate does that.  Nothing is read through the index.
        f |= SCP_DIST_FLAG_NO_NEIGHBOUR;
        idx[i] = -1;
        d2[i] = 0.0;
    } else {
        ex = b[3 * (int64_t)j] - ax; ey = b[3 * (int64_t)j + 1] - ay; ez = b[3 * (int64_t)j + 2] - az;
    }
    const double x = ax - vx, y = ay - vy, z = az - vz;
    double s2, rho2;
    // (the Python binding refuses a group out of range before the launch)
    const int bn = ring_bin(x, y, z, edges, n_rings, group ? group[i] : 0, n_groups, s2, rho2, f);
    const double s = sqrt(s2);
    double er = 0.0, ephi = 0.0, eth = 0.0;
    if (s == 0.0) {
        f |= SCP_DIST_FLAG_AXIS;
    } else if (!(f & SCP_DIST_FLAG_NO_NEIGHBOUR)) {
        const double rho = sqrt(rho2);
        const double ux = x / s, uy = y / s;          // the horizontal unit vector; (sin, cos) of the polar angle below
        const double st = s / rho, ct = z / rho;
        const double eh = ex * ux + ey * uy;          // e along the horizontal direction of a_i
        er = eh * st + ez * ct;
        ephi = ey * ux - ex * uy;
        eth = eh * ct - ez * st;
    }
    comp[3 * i] = er; comp[3 * i + 1] = ephi; comp[3 * i + 2] = eth;
    bin[i] = bn;
    flag[i] = (uint8_t)f;
}

__device__ __forceinline__ int dr_bucket(double d) {
    if (d == 0.0) return 0;
    const int e = (int)(((unsigned long long)__double_as_longlong(d) >> 52) & 0x7FF) - 1023 + 41;       // floor(log2 d) + 41 from the exponent bits
    return e < 1 ? 1 : (e > 63 ? 63 : e);
}

// one workgroup per bin
__global__ __launch_bounds__(RATE_SEG_THREADS) void dr_segments_kernel(const double *__restrict__ d2, const double *__restrict__ comp,
                                                                       const uint8_t *__restrict__ flag, const int64_t *__restrict__ order,
                                                                       int64_t n, const int64_t *__restrict__ seg_off, scp_dist_seg *__restrict__ out) {
    __shared__ double s_sq[RATE_SEG_THREADS], s_r2[RATE_SEG_THREADS], s_p2[RATE_SEG_THREADS], s_t2[RATE_SEG_THREADS], s_r[RATE_SEG_THREADS];
    __shared__ rate_max s_mx[RATE_SEG_THREADS];
    __shared__ int s_axis[RATE_SEG_THREADS], s_rows[RATE_SEG_THREADS];
    __shared__ unsigned s_hist[64];
    const int t = threadIdx.x;
    if (t < 64) s_hist[t] = 0u;
    __syncthreads();
    // the order lives in device memory like the offsets, so nobody has checked it: a row outside the table is skipped
    int64_t lo, hi;
    rate_seg_bounds(seg_off, blockIdx.x, n, lo, hi);
    double sq = 0.0, r2 = 0.0, p2 = 0.0, t2 = 0.0, sr = 0.0, mx = 0.0;
    int axis = 0, rows = 0;
    for (int64_t p = lo + t; p < hi; p += RATE_SEG_THREADS) {
        const int64_t i = order ? order[p] : p;
        if (i < 0 || i >= n) continue;
        const double d = d2[i];
        const int f = flag[i];
        ++rows;
        sq += d;
        mx = d > mx ? d : mx;
        atomicAdd(&s_hist[dr_bucket(d)], 1u);
        if (f & SCP_DIST_FLAG_AXIS) {
            ++axis;
        } else {
            const double er = comp[3 * i], ep = comp[3 * i + 1], et = comp[3 * i + 2];
            r2 += er * er; p2 += ep * ep; t2 += et * et; sr += er;
        }
    }
    s_sq[t] = sq; s_r2[t] = r2; s_p2[t] = p2; s_t2[t] = t2; s_r[t] = sr; s_mx[t].v = mx; s_axis[t] = axis; s_rows[t] = rows;
    rate_block_tree(t, s_sq, s_r2, s_p2, s_t2, s_r, s_mx, s_axis, s_rows);
    scp_dist_seg *o = out + blockIdx.x;
    if (t == 0) {
        o->rows = s_rows[0]; o->axis_rows = s_axis[0];
        o->sum_sq = s_sq[0]; o->sum_r2 = s_r2[0]; o->sum_phi2 = s_p2[0]; o->sum_theta2 = s_t2[0]; o->sum_r = s_r[0]; o->max_sq = s_mx[0].v;
    }
    if (t < 64) o->hist[t] = (int64_t)s_hist[t];
}

/* nearest neighbour's identity, error split and bin per query: see include/scp.h */
extern "C" SCP_API int scp_nn_error_split_f64(const double *a, int64_t na, const double *b, int64_t nb, const double *view, const double *edges_sq,
                                              int32_t n_rings, const int32_t *group, int32_t n_groups, int32_t *idx_out, double *d2_out,
                                              double *comp_out, int32_t *bin_out, uint8_t *flag_out, void *stream) {
    if (!a || !b || !view || !idx_out || !d2_out || !comp_out || !bin_out || !flag_out) return SCP_EINVAL;
    if (na <= 0 || nb <= 0 || na > SCP_DIST_MAX_POINTS || nb > SCP_DIST_MAX_POINTS || n_groups < 1) return SCP_EINVAL;
    if (!ring_edges_ok(edges_sq, n_rings) || (int64_t)n_groups * n_rings > SCP_DIST_MAX_BINS || !ring_view_ok(view)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int rc = scp_nn_sqdist_f64(a, na, b, nb, d2_out, stream);       // the minimum: exact and order-free
    if (rc != SCP_OK) return rc;
    const unsigned gx = (unsigned)cdiv64(na, 256);
    hipLaunchKernelGGL(dr_init_kernel, dim3(gx), dim3(256), 0, st, idx_out, na);
    LAUNCH_CHECK();
    unsigned gy = gx >= 1024 ? 1 : (1024 + gx - 1) / gx;                  // enough workgroups for 256 CUs
    const unsigned max_y = (unsigned)cdiv64(nb, DR_TILE);
    if (gy > max_y) gy = max_y;
    hipLaunchKernelGGL(dr_nn_index_kernel, dim3(gx, gy), dim3(256), 0, st, a, na, b, nb, d2_out, idx_out);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(dr_split_kernel, dim3(gx), dim3(256), 0, st, a, na, b, nb, view[0], view[1], view[2],
                       ring_edges_arg(edges_sq, n_rings), (int)n_rings, group, (int)n_groups, idx_out, d2_out, comp_out, bin_out, flag_out);
    LAUNCH_CHECK();
    return SCP_OK;
}

/* per-bin records of bin-ordered rows: see include/scp.h */
extern "C" SCP_API int scp_dist_segments_f64(const double *d2, const double *comp, const uint8_t *flag, const int64_t *order, int64_t n,
                                             const int64_t *seg_off, int32_t n_bins, scp_dist_seg *out, void *stream) {
    if (!d2 || !comp || !flag || !seg_off || !out || n <= 0 || n > SCP_DIST_MAX_POINTS || n_bins < 1 || n_bins > SCP_DIST_MAX_BINS) return SCP_EINVAL;
    hipLaunchKernelGGL(dr_segments_kernel, dim3((unsigned)n_bins), dim3(RATE_SEG_THREADS), 0, (hipStream_t)stream, d2, comp, flag, order, n, seg_off, out);
    LAUNCH_CHECK();
    return SCP_OK;
}
