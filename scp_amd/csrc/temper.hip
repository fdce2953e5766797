// Per-level temperature ("Temperature"): what the coding-order logits table would cost in ideal bits had every row been
// multiplied by an inverse temperature beta - for a whole grid of betas in one pass -, the choice of one beta per group of segments, and
// the row scaling both the encoder and the decoder then apply in front of scp_softmax_cdf (gfx950).
//
// A scaled logit is y = fl32(beta * x): ONE float32 multiply (this file is built with -ffp-contract=off, and the product is converted to
// float64 before anything is added to it, so no fused operation can take its place).  That product is all the arithmetic the two sides of
// a tempered stream share: the encoder scales its table with scp_scale_rows, the decoder its rounds' rows, and both hand the result to the
// same CDF kernel.
//
//   scp_temper_sweep    entry (s, j) = what scp_rate_segments writes as ideal_bits / bad_rows for segment s of the table scaled by beta_j, bit for
//                       bit: the row and segment contracts are those of csrc/rate.hip, through the same device functions (rate_common.h).  One
//                       wavefront per row; the row is loaded once (the next one in flight, as in rate_rows_kernel) and the beta loop runs over
//                       registers: memory traffic of one rate pass whatever nt is, nt * nsym float64 exponentials per row.
//   scp_temper_choose   per group of segments the grid index with the smallest sum, under the side-information rule.
//   scp_scale_rows      out[r][c] = fl32(seg_beta[seg(r)] * in[r][c]).
// No floating-point atomics, no data-dependent order of additions: the same bits in every run.
#include "rate_common.h"

#define TEMPER_MAX_NT 32

struct temper_grid {
    float beta[TEMPER_MAX_NT];
};

template <bool VEC>
__global__ __launch_bounds__(256) void temper_rows_kernel(const float *__restrict__ logits, int64_t ld, int64_t n, int nsym,
                                                          const uint8_t *__restrict__ sym, const temper_grid grid, int nt,
                                                          double *__restrict__ ws_bits, uint32_t *__restrict__ ws_bad,
                                                          double *__restrict__ row_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * RATE_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * RATE_ROWS_PER_BLOCK;
    if (wave >= n) return;
    float4 next = rate_load<VEC>(logits + wave * ld, lane, nsym);
    for (int64_t r = wave; r < n; r += nwave) {
        const float4 v = next;
        if (r + nwave < n) next = rate_load<VEC>(logits + (r + nwave) * ld, lane, nsym);      // the next row is in flight under this row's exponentials
        const int s = (int)sym[r];
        const bool sym_ok = s < nsym;                 // (a symbol outside the alphabet has no logit to read: bad at every beta)
        const float xs = sym_ok ? logits[r * ld + s] : 0.0f;
        double mine = 0.0;                            // lane j keeps the row's bits at beta_j
        bool mine_bad = false;
        for (int j = 0; j < nt; ++j) {
            const float b = grid.beta[j];
            float4 y;                                 // beta > 0: a column >= nsym stays -inf
            y.x = b * v.x; y.y = b * v.y; y.z = b * v.z; y.w = b * v.w;
            const float m = rate_row_max(y);
            const double md = (double)m;
            const double sum = rate_row_expsum(y, md, lane, nsym);
            if (lane == j) {                          // md and sum are the same in every lane: the logarithm is lane j's alone
                const double ideal = sym_ok ? rate_row_ideal(md, b * xs, sum) : 0.0;
                mine_bad = !sym_ok || !rate_finite(ideal);
                mine = mine_bad ? 0.0 : ideal;
            }
        }
        const uint32_t bad = (uint32_t)__ballot(mine_bad);      // bit j: the row is bad at beta_j (lanes >= nt never set theirs)
        if (lane < nt) {
            ws_bits[r * nt + lane] = mine;
            if (row_bits) row_bits[r * nt + lane] = mine;
        }
        if (lane == 0) ws_bad[r] = bad;
    }
}

// one workgroup per (segment, beta)
__global__ __launch_bounds__(RATE_SEG_THREADS) void temper_segments_kernel(const double *__restrict__ ws_bits, const uint32_t *__restrict__ ws_bad,
                                                                           const int64_t *__restrict__ seg_off, int64_t n, int nt,
                                                                           double *__restrict__ seg_bits, int32_t *__restrict__ seg_bad) {
    __shared__ double s_bits[RATE_SEG_THREADS];
    __shared__ int s_bad[RATE_SEG_THREADS];
    const int t = threadIdx.x, j = blockIdx.y;
    int64_t a, b;
    rate_seg_bounds(seg_off, blockIdx.x, n, a, b);
    double bits = 0.0;
    int bad = 0;
    for (int64_t i = a + t; i < b; i += RATE_SEG_THREADS) {
        bits += ws_bits[i * nt + j];
        bad += (int)((ws_bad[i] >> j) & 1u);
    }
    s_bits[t] = bits; s_bad[t] = bad;
    rate_block_tree(t, s_bits, s_bad);
    if (t == 0) {
        seg_bits[(int64_t)blockIdx.x * nt + j] = s_bits[0];
        seg_bad[(int64_t)blockIdx.x * nt + j] = s_bad[0];
    }
}

__device__ __forceinline__ int temper_group(const int32_t *__restrict__ group, int s, int ngroup) {
    const int g = group[s];                           // device memory nobody has checked: clamped, never followed out of range
    return g < 0 ? 0 : (g >= ngroup ? ngroup - 1 : g);
}

// one workgroup per group, thread j adds the group's segments at beta_j in segment-index order
__global__ __launch_bounds__(64) void temper_choose_kernel(const double *__restrict__ seg_bits, const int32_t *__restrict__ seg_bad,
                                                           const int64_t *__restrict__ seg_off, int64_t n, const int32_t *__restrict__ group,
                                                           int nseg, int ngroup, const temper_grid grid, int nt, int unit, double min_gain,
                                                           int32_t *__restrict__ choice, double *__restrict__ group_bits,
                                                           float *__restrict__ seg_beta) {
    __shared__ double s_sum[TEMPER_MAX_NT];
    __shared__ int s_bad[TEMPER_MAX_NT];
    __shared__ int s_pick;
    const int g = blockIdx.x, j = threadIdx.x;
    if (j < nt) {
        double sum = 0.0;
        int bad = 0;
        for (int s = 0; s < nseg; ++s) {
            if (temper_group(group, s, ngroup) != g) continue;
            sum += seg_bits[(int64_t)s * nt + j];
            bad |= seg_bad[(int64_t)s * nt + j] != 0;
        }
        s_sum[j] = sum;
        s_bad[j] = bad;
    }
    __syncthreads();
    if (j == 0) {
        int64_t rows = 0;
        for (int s = 0; s < nseg; ++s) {
            if (temper_group(group, s, ngroup) != g) continue;
            int64_t a, b;
            rate_seg_bounds(seg_off, s, n, a, b);
            rows += b - a;
        }
        int best = unit, bad = 0;
        for (int k = 0; k < nt; ++k) {
            bad |= s_bad[k];
            const int dk = k < unit ? unit - k : k - unit, db = best < unit ? unit - best : best - unit;
            if (s_sum[k] < s_sum[best] || (s_sum[k] == s_sum[best] && (dk < db || (dk == db && k < best)))) best = k;
        }
        // the side-information rule: a group moves only when that saves more than its index costs
        if (bad || rows == 0 || !(s_sum[unit] - s_sum[best] > min_gain)) best = unit;
        choice[g] = best;
        group_bits[2 * g] = s_sum[unit];
        group_bits[2 * g + 1] = s_sum[best];
        s_pick = best;
    }
    __syncthreads();
    const float beta = grid.beta[s_pick];
    for (int s = j; s < nseg; s += 64)
        if (temper_group(group, s, ngroup) == g) seg_beta[s] = beta;
}

// a wavefront per row; the row's segment by bisection of the offsets
template <bool VEC>
__global__ __launch_bounds__(256) void scale_rows_kernel(const float *in, int64_t ld_in, float *out, int64_t ld_out, int64_t n, int nsym,
                                                         int ncopy, const int64_t *__restrict__ seg_off,
                                                         const float *__restrict__ seg_beta, int nseg) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * RATE_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * RATE_ROWS_PER_BLOCK;
    for (int64_t r = wave; r < n; r += nwave) {
        // the last segment whose (clamped) start is <= r; a row no segment holds keeps its bits (beta 1)
        int lo = 0, hi = nseg;                        // the answer lies in [lo, hi)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg_off[mid] <= r) lo = mid; else hi = mid;
        }
        float beta = 1.0f;
        if (nseg > 0 && seg_off[lo] <= r && r < seg_off[lo + 1]) beta = seg_beta[lo];
        const float *src = in + r * ld_in;
        float *dst = out + r * ld_out;
        const int c = 4 * lane;
        if (VEC) {                                    // both strides 256, 16-byte aligned bases: a row is 64 float4
            float4 v = *(const float4 *)(src + c);
            if (c + 3 < nsym) {
                v.x = beta * v.x; v.y = beta * v.y; v.z = beta * v.z; v.w = beta * v.w;
                *(float4 *)(dst + c) = v;
            } else {
                if (c < nsym) dst[c] = beta * v.x; else if (c < ncopy) dst[c] = v.x;
                if (c + 1 < nsym) dst[c + 1] = beta * v.y; else if (c + 1 < ncopy) dst[c + 1] = v.y;
                if (c + 2 < nsym) dst[c + 2] = beta * v.z; else if (c + 2 < ncopy) dst[c + 2] = v.z;
                if (c + 3 < nsym) dst[c + 3] = beta * v.w; else if (c + 3 < ncopy) dst[c + 3] = v.w;
            }
        } else {
            for (int k = lane; k < ncopy; k += 64) {
                const float x = src[k];
                dst[k] = k < nsym ? beta * x : x;
            }
        }
    }
}

static inline int64_t temper_bad_offset(int64_t n, int32_t nt) { return 8 * n * nt; }

extern "C" int64_t scp_temper_workspace_bytes(int64_t n, int32_t nseg, int32_t nt) {
    if (n < 0 || nseg < 0 || nt < 1 || nt > TEMPER_MAX_NT) return SCP_EINVAL;
    return n == 0 ? 0 : (((8 * (int64_t)nt + 4) * n + 255) / 256) * 256;       // nt float64 + one 32-bit mask per row
}

static int temper_grid_ok(const float *betas, int32_t nt, temper_grid *g) {
    if (nt < 1 || nt > TEMPER_MAX_NT || !betas) return 0;
    for (int j = 0; j < TEMPER_MAX_NT; ++j) g->beta[j] = 1.0f;
    for (int j = 0; j < nt; ++j) {
        if (!(betas[j] > 0.0f) || !(betas[j] <= 3.40282346638528859812e38f)) return 0;      // not finite or not positive
        g->beta[j] = betas[j];
    }
    return 1;
}

extern "C" int scp_temper_sweep(const float *logits, int64_t ld, int64_t n, int32_t nsym, const uint8_t *sym, const int64_t *seg_off,
                                int32_t nseg, const float *betas, int32_t nt, double *seg_bits, int32_t *seg_bad, double *row_bits,
                                void *workspace, int64_t workspace_bytes, void *stream) {
    temper_grid grid;
    if (n < 0 || nseg < 0 || nsym < 2 || nsym > 256 || ld < nsym) return SCP_EINVAL;
    if (!temper_grid_ok(betas, nt, &grid)) return SCP_EINVAL;
    if (nseg > 0 && (!seg_off || !seg_bits || !seg_bad)) return SCP_EINVAL;
    if (n > 0 && (!logits || !sym || !workspace || workspace_bytes < scp_temper_workspace_bytes(n, nseg, nt))) return SCP_EINVAL;
    if (n > 0 && (((uintptr_t)workspace) & 7)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (nseg > 0) {
            HIP_TRY(hipMemsetAsync(seg_bits, 0, (size_t)nseg * nt * sizeof(double), st));
            HIP_TRY(hipMemsetAsync(seg_bad, 0, (size_t)nseg * nt * sizeof(int32_t), st));
        }
        return SCP_OK;
    }
    double *ws_bits = (double *)workspace;
    uint32_t *ws_bad = (uint32_t *)((uint8_t *)workspace + temper_bad_offset(n, nt));
    const int64_t want = cdiv64(n, RATE_ROWS_PER_BLOCK);
    const unsigned nb = (unsigned)(want < 16384 ? want : 16384);
    // (booked under the rate report's tag, which has no sibling for the sweep: with launch profiling on, a tempered frame's "rate" bucket
    // holds the sweep as well; bytes: the table once, nt float64 and a mask word per row out and back in)
    SCP_PROF(SCP_PROF_RATE, st, (double)n * (4.0 * nsym + 1.0 + 2.0 * (8.0 * nt + 4.0)));
    if (ld == 256 && (((uintptr_t)logits) & 15) == 0)
        hipLaunchKernelGGL(temper_rows_kernel<true>, dim3(nb), dim3(256), 0, st, logits, ld, n, nsym, sym, grid, nt, ws_bits, ws_bad, row_bits);
    else
        hipLaunchKernelGGL(temper_rows_kernel<false>, dim3(nb), dim3(256), 0, st, logits, ld, n, nsym, sym, grid, nt, ws_bits, ws_bad, row_bits);
    LAUNCH_CHECK();
    if (nseg > 0) {
        hipLaunchKernelGGL(temper_segments_kernel, dim3((unsigned)nseg, (unsigned)nt), dim3(RATE_SEG_THREADS), 0, st, ws_bits, ws_bad, seg_off, n,
                           nt, seg_bits, seg_bad);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

extern "C" int scp_temper_choose(const double *seg_bits, const int32_t *seg_bad, const int64_t *seg_off, int64_t n, const int32_t *group,
                                 int32_t nseg, int32_t ngroup, const float *betas, int32_t nt, int32_t unit, double min_gain_bits,
                                 int32_t *choice, double *group_bits, float *seg_beta, void *stream) {
    temper_grid grid;
    if (n < 0 || nseg < 0 || ngroup < 1 || !temper_grid_ok(betas, nt, &grid)) return SCP_EINVAL;
    if (unit < 0 || unit >= nt || betas[unit] != 1.0f) return SCP_EINVAL;
    if (!(min_gain_bits >= 0.0) || !(min_gain_bits <= RATE_DBL_MAX)) return SCP_EINVAL;
    if (!choice || !group_bits) return SCP_EINVAL;
    if (nseg > 0 && (!seg_bits || !seg_bad || !seg_off || !group || !seg_beta)) return SCP_EINVAL;
    hipLaunchKernelGGL(temper_choose_kernel, dim3((unsigned)ngroup), dim3(64), 0, (hipStream_t)stream, seg_bits, seg_bad, seg_off, n, group, nseg,
                       ngroup, grid, nt, unit, min_gain_bits, choice, group_bits, seg_beta);
    LAUNCH_CHECK();
    return SCP_OK;
}

extern "C" int scp_scale_rows(const float *in, int64_t ld_in, float *out, int64_t ld_out, int64_t n, int32_t nsym, const int64_t *seg_off,
                              const float *seg_beta, int32_t nseg, void *stream) {
    if (n < 0 || nseg < 0 || nsym < 2 || nsym > 256 || ld_in < nsym || ld_out < nsym) return SCP_EINVAL;
    if (n > 0 && (!in || !out)) return SCP_EINVAL;
    if (n > 0 && in == out && ld_in != ld_out) return SCP_EINVAL;      // in place means the same rows
    if (nseg > 0 && (!seg_off || !seg_beta)) return SCP_EINVAL;
    if (n == 0) return SCP_OK;
    hipStream_t st = (hipStream_t)stream;
    // in place: columns >= nsym are left alone; out of place: those both rows have are copied
    const int64_t common = ld_in < ld_out ? ld_in : ld_out;
    const int ncopy = (in == out && ld_in == ld_out) ? nsym : (int)(common < (int64_t)1 << 30 ? common : (int64_t)1 << 30);
    const int64_t want = cdiv64(n, RATE_ROWS_PER_BLOCK);
    const unsigned nb = (unsigned)(want < 16384 ? want : 16384);
    if (ld_in == 256 && ld_out == 256 && ((((uintptr_t)in) | ((uintptr_t)out)) & 15) == 0)
        hipLaunchKernelGGL(scale_rows_kernel<true>, dim3(nb), dim3(256), 0, st, in, ld_in, out, ld_out, n, nsym, ncopy, seg_off, seg_beta, nseg);
    else
        hipLaunchKernelGGL(scale_rows_kernel<false>, dim3(nb), dim3(256), 0, st, in, ld_in, out, ld_out, n, nsym, ncopy, seg_off, seg_beta, nseg);
    LAUNCH_CHECK();
    return SCP_OK;
}
