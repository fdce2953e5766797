// D2 (point-to-plane) distortion on the device (gfx950), float64 throughout: per-point normals of a cloud, and the tie-set reductions
// of the MPEG `pc_error` tool's p2plane metric.
//
// Replaces data_preproc/gene_normals.py (open3d estimate_normals with KDTreeSearchParamHybrid(radius, max_nn) +
// orient_normals_towards_camera_location) and the p2plane half of the pc_error run behind pt.py:13-85 / utils.get_psnr.
// Exhaustive search like metrics.hip, and the same distance expression: |a - b|^2 = (dx*dx + dy*dy) + dz*dz with separate roundings
// (this file is compiled with -ffp-contract=off), so a distance recomputed here equals the minimum scp_nn_sqdist_f64 stored bit for
// bit, and numpy reproduces every number.
//   every kernel: one thread per output element, the other cloud streams through LDS in tiles, sums run in index order.  No
//   floating-point atomics and no split of the streamed cloud: the results do not depend on the launch.
#include "scp_internal.h"

#define NRM_THREADS 128
#define NRM_TILE 1024
#define NRM_MAX_NN 32
#define NRM_SWEEPS 8       // cyclic Jacobi on a 3x3 matrix converges quadratically: 5 sweeps reach float64 precision, 8 leave a margin

#define TIE_THREADS 128
#define TIE_TILE 512

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix (Golub & Van Loan 8.5: t is the smaller root, |t| <= 1); r is the
// third index.  Updates the matrix entries and the columns p, q of the eigenvector matrix V.
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq,
                                              double &v0p, double &v0q, double &v1p, double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));     // theta^2 = inf -> t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    double a, b;
    a = c * v0p - s * v0q; b = s * v0p + c * v0q; v0p = a; v0q = b;
    a = c * v1p - s * v1q; b = s * v1p + c * v1q; v1p = a; v1q = b;
    a = c * v2p - s * v2q; b = s * v2p + c * v2q; v2p = a; v2q = b;
}

// Neighbour lists live in LDS, [slot][thread] so that the threads of a wave touch consecutive addresses (a per-thread array with a
// run-time subscript would go to scratch).  NRM_THREADS * 32 * 12 B = 48 KiB + the 24 KiB tile: two workgroups per CU.
__global__ __launch_bounds__(NRM_THREADS) void estimate_normals_f64_kernel(const double *__restrict__ xyz, int n, double r2, int max_nn,
                                                                           double vx, double vy, double vz, double *__restrict__ normals,
                                                                           int *__restrict__ count, int *__restrict__ idx_out) {
    __shared__ double sb[NRM_TILE * 3];
    __shared__ double ld[NRM_MAX_NN * NRM_THREADS];
    __shared__ int li[NRM_MAX_NN * NRM_THREADS];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * NRM_THREADS + tid;
    const int ic = i < n ? i : n - 1;
    const double px = xyz[3 * (int64_t)ic], py = xyz[3 * (int64_t)ic + 1], pz = xyz[3 * (int64_t)ic + 2];
    int cnt = 0;
    double lim = r2;                 // min(radius^2, current worst of a full list): nearly every candidate fails d <= lim
    for (int t0 = 0; t0 < n; t0 += NRM_TILE) {
        const int tc = (n - t0) < NRM_TILE ? (n - t0) : NRM_TILE;
        __syncthreads();
        for (int e = tid; e < tc * 3; e += NRM_THREADS) sb[e] = xyz[3 * (int64_t)t0 + e];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < tc; ++j) {
            const double dx = px - sb[3 * j], dy = py - sb[3 * j + 1], dz = pz - sb[3 * j + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d <= lim) {
                // candidates arrive in index order, so among equal distances the earlier one stays in front: (d2, index) ascending
                const bool full = cnt == max_nn;
                if (!(full && d >= ld[(max_nn - 1) * NRM_THREADS + tid])) {
                    int p = full ? max_nn - 1 : cnt;
                    while (p > 0 && ld[(p - 1) * NRM_THREADS + tid] > d) {
                        ld[p * NRM_THREADS + tid] = ld[(p - 1) * NRM_THREADS + tid];
                        li[p * NRM_THREADS + tid] = li[(p - 1) * NRM_THREADS + tid];
                        --p;
                    }
                    ld[p * NRM_THREADS + tid] = d;
                    li[p * NRM_THREADS + tid] = t0 + j;
                    if (!full) ++cnt;
                    if (cnt == max_nn) {
                        const double w = ld[(max_nn - 1) * NRM_THREADS + tid];
                        lim = w < r2 ? w : r2;
                    }
                }
            }
        }
    }
    if (i >= n) return;
    count[i] = cnt;
    if (idx_out)
        for (int k = 0; k < max_nn; ++k) idx_out[(int64_t)i * max_nn + k] = k < cnt ? li[k * NRM_THREADS + tid] : -1;
    double nx = 0.0, ny = 0.0, nz = 1.0;          // fewer than 3 neighbours: open3d's default normal
    if (cnt >= 3) {
        // centred two-pass covariance, summed in list order
        double mx = 0.0, my = 0.0, mz = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const int64_t j = li[k * NRM_THREADS + tid];
            mx += xyz[3 * j]; my += xyz[3 * j + 1]; mz += xyz[3 * j + 2];
        }
        const double inv = (double)cnt;
        mx = mx / inv; my = my / inv; mz = mz / inv;
        double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const int64_t j = li[k * NRM_THREADS + tid];
            const double x = xyz[3 * j] - mx, y = xyz[3 * j + 1] - my, z = xyz[3 * j + 2] - mz;
            a00 += x * x; a01 += x * y; a02 += x * z; a11 += y * y; a12 += y * z; a22 += z * z;
        }
        a00 = a00 / inv; a01 = a01 / inv; a02 = a02 / inv; a11 = a11 / inv; a12 = a12 / inv; a22 = a22 / inv;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int s = 0; s < NRM_SWEEPS; ++s) {
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0,1), r = 2
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0,2), r = 1
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1,2), r = 0
        }
        // eigenvector of the smallest eigenvalue (first of equals), renormalised
        const bool u1 = a11 < a00;
        const bool u2 = a22 < (u1 ? a11 : a00);
        nx = u2 ? v02 : (u1 ? v01 : v00);
        ny = u2 ? v12 : (u1 ? v11 : v10);
        nz = u2 ? v22 : (u1 ? v21 : v20);
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        nx = nx / len; ny = ny / len; nz = nz / len;
    }
    // orient towards the sensor
    const double dot = (nx * (vx - px) + ny * (vy - py)) + nz * (vz - pz);
    if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    normals[3 * (int64_t)i] = nx; normals[3 * (int64_t)i + 1] = ny; normals[3 * (int64_t)i + 2] = nz;
}

// Tie-set reductions.  A pair (q_i, p_j) belongs to a tie set iff its distance, recomputed by the expression above, equals the stored
// nearest-neighbour minimum bit for bit.
//   MODE 0 (SCP_TIE_MEAN_NORMAL): dmin [np] and nrm [np][3] belong to the STREAMED cloud p; out [nq][3] = mean of nrm[j] over
//          {j : q_i is a nearest neighbour of p_j} (0 when that set is empty) - the normals pc_error hands to the cloud without any.
//   MODE 1 (SCP_TIE_PLANE_ERROR): dmin [nq] belongs to the queries, nrm [np][3] to the streamed cloud; out [nq] = mean over the
//          nearest neighbours p_j of q_i of ((q_i - p_j) . nrm[j])^2.  Normals of points outside every tie set are never read into a sum.
template <int MODE>
__global__ __launch_bounds__(TIE_THREADS) void nn_tieset_f64_kernel(const double *__restrict__ q, int64_t nq, const double *__restrict__ p, int64_t np,
                                                                    const double *__restrict__ dmin, const double *__restrict__ nrm,
                                                                    double *__restrict__ out) {
    __shared__ double sp[TIE_TILE * 3];
    __shared__ double sn[TIE_TILE * 3];
    __shared__ double sd[MODE == 0 ? TIE_TILE : 1];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * TIE_THREADS + tid;
    const int64_t ic = i < nq ? i : nq - 1;
    const double qx = q[3 * ic], qy = q[3 * ic + 1], qz = q[3 * ic + 2];
    const double mine = MODE == 1 ? dmin[ic] : 0.0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int64_t cnt = 0;
    for (int64_t t0 = 0; t0 < np; t0 += TIE_TILE) {
        const int tc = (int)((np - t0) < TIE_TILE ? (np - t0) : TIE_TILE);
        __syncthreads();
        for (int e = tid; e < tc * 3; e += TIE_THREADS) { sp[e] = p[3 * t0 + e]; sn[e] = nrm[3 * t0 + e]; }
        if (MODE == 0)
            for (int e = tid; e < tc; e += TIE_THREADS) sd[e] = dmin[t0 + e];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < tc; ++j) {
            const double dx = qx - sp[3 * j], dy = qy - sp[3 * j + 1], dz = qz - sp[3 * j + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d == (MODE == 0 ? sd[j] : mine)) {
                if (MODE == 0) {
                    s0 += sn[3 * j]; s1 += sn[3 * j + 1]; s2 += sn[3 * j + 2];
                } else {
                    const double pr = (dx * sn[3 * j] + dy * sn[3 * j + 1]) + dz * sn[3 * j + 2];
                    s0 += pr * pr;
                }
                ++cnt;
            }
        }
    }
    if (i >= nq) return;
    const double c = (double)cnt;
    if (MODE == 0) {
        out[3 * i] = cnt ? s0 / c : 0.0; out[3 * i + 1] = cnt ? s1 / c : 0.0; out[3 * i + 2] = cnt ? s2 / c : 0.0;
    } else {
        out[i] = cnt ? s0 / c : 0.0;
    }
}

/* normals of a cloud: see include/scp.h */
extern "C" SCP_API int scp_estimate_normals_f64(const double *xyz, int64_t n, double radius, int32_t max_nn, const double *view, double *normals,
                                                int32_t *count, int32_t *idx, void *stream) {
    if (!xyz || !view || !normals || !count || n <= 0 || n > (1ll << 30) || max_nn < 1 || max_nn > NRM_MAX_NN || !(radius > 0.0)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(estimate_normals_f64_kernel, dim3((unsigned)cdiv64(n, NRM_THREADS)), dim3(NRM_THREADS), 0, st, xyz, (int)n, radius * radius,
                       (int)max_nn, view[0], view[1], view[2], normals, count, idx);
    LAUNCH_CHECK();
    return SCP_OK;
}

/* tie-set reductions of the p2plane metric: see include/scp.h */
extern "C" SCP_API int scp_nn_tieset_f64(int32_t mode, const double *q, int64_t nq, const double *p, int64_t np, const double *dmin, const double *nrm,
                                         double *out, void *stream) {
    if (!q || !p || !dmin || !nrm || !out || nq <= 0 || np <= 0 || (mode != SCP_TIE_MEAN_NORMAL && mode != SCP_TIE_PLANE_ERROR)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv64(nq, TIE_THREADS));
    if (mode == SCP_TIE_MEAN_NORMAL)
        hipLaunchKernelGGL(nn_tieset_f64_kernel<0>, grid, dim3(TIE_THREADS), 0, st, q, nq, p, np, dmin, nrm, out);
    else
        hipLaunchKernelGGL(nn_tieset_f64_kernel<1>, grid, dim3(TIE_THREADS), 0, st, q, nq, p, np, dmin, nrm, out);
    LAUNCH_CHECK();
    return SCP_OK;
}
