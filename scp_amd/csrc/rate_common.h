// The row and segment contracts of the rate report (csrc/rate.hip) as device functions, shared with the temperature sweep
// (csrc/temper.hip), the distortion report (csrc/distreport.hip) and the rate per ring (csrc/ringrate.hip): whoever evaluates a row's
// cross-entropy, adds rows up or bins a point through these gets the same bits.
//   row:     lane l of the row's wavefront owns columns 4 l .. 4 l + 3 and adds their exponentials in column order, then a fixed xor butterfly
//            (32, 16, .. 1) across the wavefront;
//   segment: thread t of the workgroup adds rows t, t + 1024, .. in that order, then a fixed binary tree over the 1024 partial sums;
//   ring:    one expression for rho2 and one ascending scan of the edges (ring_bin).
// Every including file is built with -ffp-contract=off.
#pragma once
#include "scp_internal.h"

#define RATE_ROWS_PER_BLOCK 4          // a wavefront per row
#define RATE_SEG_THREADS 1024
#define RATE_LN2 0.693147180559945309417232121458
#define RATE_DBL_MAX 1.79769313486231570815e308

__device__ __forceinline__ double rate_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);      // a + b == b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ float rate_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// the four columns 4 lane .. 4 lane + 3 of one row; columns >= nsym come back as -inf (they take no part in the maximum and are skipped in the sum)
template <bool VEC>
__device__ __forceinline__ float4 rate_load(const float *__restrict__ row, int lane, int nsym) {
    const int c = 4 * lane;
    float4 v;
    if (VEC) {
        v = *(const float4 *)(row + c);              // ld == 256, 16-byte aligned rows: all 256 floats of the row are the caller's
        if (c + 1 >= nsym) v.y = -INFINITY;
        if (c + 2 >= nsym) v.z = -INFINITY;
        if (c + 3 >= nsym) v.w = -INFINITY;
        if (c >= nsym) v.x = -INFINITY;
    } else {
        v.x = c < nsym ? row[c] : -INFINITY;
        v.y = c + 1 < nsym ? row[c + 1] : -INFINITY;
        v.z = c + 2 < nsym ? row[c + 2] : -INFINITY;
        v.w = c + 3 < nsym ? row[c + 3] : -INFINITY;
    }
    return v;
}

// the row's maximum, the same float in every lane
__device__ __forceinline__ float rate_row_max(const float4 v) { return rate_wave_max(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w))); }

// sum_j exp(x[j] - m) of the row, the same float64 in every lane
__device__ __forceinline__ double rate_row_expsum(const float4 v, double md, int lane, int nsym) {
    const int c = 4 * lane;
    double acc = 0.0;                             // column order inside the lane; a column >= nsym adds nothing
    if (c < nsym) acc = exp((double)v.x - md);
    if (c + 1 < nsym) acc += exp((double)v.y - md);
    if (c + 2 < nsym) acc += exp((double)v.z - md);
    if (c + 3 < nsym) acc += exp((double)v.w - md);
    return rate_wave_sum(acc);
}

// the row's cross-entropy in bits from its maximum, the symbol's logit and the sum above
__device__ __forceinline__ double rate_row_ideal(double md, float xs, double sum) { return (md - (double)xs + log(sum)) / RATE_LN2; }

__device__ __forceinline__ bool rate_finite(double v) { return fabs(v) <= RATE_DBL_MAX; }

// the offsets live in device memory, so nobody has checked them: clamp to the table
__device__ __forceinline__ void rate_seg_bounds(const int64_t *__restrict__ seg_off, int s, int64_t n, int64_t &a, int64_t &b) {
    a = seg_off[s];
    b = seg_off[s + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < a ? a : (b > n ? n : b);
}

// the fixed binary tree over RATE_SEG_THREADS partials per array (shared memory, written by every thread before the call): s[0] holds the
// result.  An array of rate_max carries a maximum through the same loop and the same barriers; every other array a sum.
struct rate_max { double v; };
template <typename T>
__device__ __forceinline__ void rate_join(T &a, const T &b) { a += b; }
__device__ __forceinline__ void rate_join(rate_max &a, const rate_max &b) { a.v = b.v > a.v ? b.v : a.v; }

template <typename... T>
__device__ __forceinline__ void rate_block_tree(int t, T *...s) {
    __syncthreads();
    for (int h = RATE_SEG_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) (rate_join(s[t], s[t + h]), ...);
        __syncthreads();
    }
}

// The ring rule of the distortion report and of the rate per ring: ring = the largest r with rho2 >= edges.sq[r], decided on
// rho2 = (x*x + y*y) + z*z of (point - view) - no sqrt takes part; bin = group * n_rings + ring.
struct ring_edges { double sq[SCP_DIST_MAX_RINGS]; };

// (x, y, z) = point - view, g = the point's group.  -> the bin; s2 and rho2 for a caller that goes on with them; a group outside
// [0, n_groups) never gives an out-of-range bin: it is clamped and SCP_DIST_FLAG_GROUP_CLAMPED is set in f.
__device__ __forceinline__ int ring_bin(double x, double y, double z, const ring_edges &edges, int n_rings, int g, int n_groups, double &s2,
                                        double &rho2, int &f) {
    s2 = x * x + y * y;
    rho2 = s2 + z * z;
    int ring = 0;
    for (int r = 1; r < n_rings; ++r) ring = rho2 >= edges.sq[r] ? r : ring;      // edges ascend: the last hit is the largest r
    if (g < 0 || g >= n_groups) {
        f |= SCP_DIST_FLAG_GROUP_CLAMPED;
        g = g < 0 ? 0 : n_groups - 1;
    }
    return g * n_rings + ring;
}

// host: squared edges 0 = e_0 < e_1 < .. finite, at most SCP_DIST_MAX_RINGS; a finite view
static inline bool ring_edges_ok(const double *edges_sq, int32_t n_rings) {
    if (!edges_sq || n_rings < 1 || n_rings > SCP_DIST_MAX_RINGS || edges_sq[0] != 0.0) return false;
    for (int r = 1; r < n_rings; ++r)
        if (!(edges_sq[r] > edges_sq[r - 1]) || !(edges_sq[r] <= RATE_DBL_MAX)) return false;
    return true;
}

static inline bool ring_view_ok(const double *view) {
    return fabs(view[0]) <= RATE_DBL_MAX && fabs(view[1]) <= RATE_DBL_MAX && fabs(view[2]) <= RATE_DBL_MAX;
}

static inline ring_edges ring_edges_arg(const double *edges_sq, int32_t n_rings) {
    ring_edges e;
    for (int r = 0; r < SCP_DIST_MAX_RINGS; ++r) e.sq[r] = r < n_rings ? edges_sq[r] : 0.0;
    return e;
}
