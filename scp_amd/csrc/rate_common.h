// The row and segment contracts of the rate report (csrc/rate.hip) as device functions, shared with the temperature sweep
// (csrc/temper.hip): whoever evaluates a row's cross-entropy or adds rows up through these gets the same bits.
//   row:     lane l of the row's wavefront owns columns 4 l .. 4 l + 3 and adds their exponentials in column order, then a fixed xor butterfly
//            (32, 16, .. 1) across the wavefront;
//   segment: thread t of the workgroup adds rows t, t + 1024, .. in that order, then a fixed binary tree over the 1024 partial sums.
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

// the fixed binary tree over RATE_SEG_THREADS partial sums per array (shared memory, written by every thread before the call): s[0] holds the sum
template <typename... T>
__device__ __forceinline__ void rate_block_tree(int t, T *...s) {
    __syncthreads();
    for (int h = RATE_SEG_THREADS / 2; h >= 1; h >>= 1) {
        if (t < h) ((s[t] += s[t + h]), ...);
        __syncthreads();
    }
}
