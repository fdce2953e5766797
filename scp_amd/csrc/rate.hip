// Rate report: ideal (cross-entropy) and coded-table bits per row of the coding-order logits table, summed per segment (gfx950).
//
// What the encoder's rate figure hides: `8 * len(stream) / n_points` says nothing about where the bits go.  Per coded row this file computes
//   ideal_bits = (m - x[sym] + log(sum_j exp(x[j] - m))) / ln 2     the model's cross-entropy in bits (models/ehem.py:198-210: train_loss is its
//                                                                   mean per node), m = the row maximum, every term float64 from the float32 logits
//   table_bits = 16 - log2(c_high - c_low)                          what numpyAc's 16-bit table charges for the symbol (the pair scp_softmax_cdf wrote)
//   top1       = (x[sym] == m)                                      a tie with the maximum is a hit
// and sums them over caller-given segments of consecutive rows (octree levels, EHEM phases).
//
// Summation order is part of the contract ("Rate report"):
//   row:     lane l of the row's wavefront owns columns 4 l .. 4 l + 3 and adds their exponentials in column order, then a fixed xor butterfly
//            (32, 16, .. 1) across the wavefront - a function of nsym alone, the same for any row stride;
//   segment: thread t of the segment's one workgroup adds rows t, t + 1024, .. of the segment in that order, then a fixed binary tree over the
//            1024 partial sums - a function of the segment's length alone, wherever the segment lies in the table.
// No floating-point atomics anywhere: a segment's sums are the same bits in every run, for either row stride, alone or inside a batch.
// The row kernel leaves two float64 and one flag byte per row in the caller's workspace; the segment kernel reads them back.
#include "rate_common.h"        // the row and segment contracts as device functions (shared with csrc/temper.hip)

#define RATE_FLAG_TOP1 1
#define RATE_FLAG_BAD 2

template <bool VEC>
__global__ __launch_bounds__(256) void rate_rows_kernel(const float *__restrict__ logits, int64_t ld, int64_t n, int nsym,
                                                        const uint8_t *__restrict__ sym, const uint32_t *__restrict__ lohi,
                                                        double *__restrict__ ws_bits, uint8_t *__restrict__ ws_flag,
                                                        double *__restrict__ row_ideal, double *__restrict__ row_table) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * RATE_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * RATE_ROWS_PER_BLOCK;
    if (wave >= n) return;
    float4 next = rate_load<VEC>(logits + wave * ld, lane, nsym);
    for (int64_t r = wave; r < n; r += nwave) {
        const float4 v = next;
        if (r + nwave < n) next = rate_load<VEC>(logits + (r + nwave) * ld, lane, nsym);      // the next row is in flight under this row's exponentials
        const int s = (int)sym[r];
        const uint32_t p = lohi[r];
        const float m = rate_row_max(v);
        const double md = (double)m;
        const double sum = rate_row_expsum(v, md, lane, nsym);
        if (lane == 0) {
            const int w = (int)((p >> 16) ? (p >> 16) : 65536u) - (int)(p & 0xFFFFu);
            double ideal = 0.0, table = 0.0;
            int flag = 0;
            if (s < nsym) {                           // (a symbol outside the alphabet has no logit to read)
                const float xs = logits[r * ld + s];
                ideal = rate_row_ideal(md, xs, sum);
                if (xs == m) flag |= RATE_FLAG_TOP1;
            }
            const bool pair_ok = w >= 1 && s < nsym;
            // Bad rows are counted and nothing non-finite is written.  Two kinds: a pair no table of this library has (width below one, or a
            // symbol outside the alphabet) stays out of both sums; a non-finite cross-entropy (the symbol's logit is -inf) adds 0 ideal bits,
            // but its pair is a real table entry of width 1 or more - the coder spends those bits, so the table bits keep them.
            if (!pair_ok || !rate_finite(ideal)) {
                flag |= RATE_FLAG_BAD;
                ideal = 0.0;
            }
            if (pair_ok) table = 16.0 - log2((double)w);
            ws_bits[2 * r] = ideal;
            ws_bits[2 * r + 1] = table;
            ws_flag[r] = (uint8_t)flag;
            if (row_ideal) row_ideal[r] = ideal;
            if (row_table) row_table[r] = table;
        }
    }
}

// one workgroup per segment
__global__ __launch_bounds__(RATE_SEG_THREADS) void rate_segments_kernel(const double *__restrict__ ws_bits, const uint8_t *__restrict__ ws_flag,
                                                                         const int64_t *__restrict__ seg_off, int64_t n,
                                                                         scp_rate_seg *__restrict__ out) {
    __shared__ double s_ideal[RATE_SEG_THREADS], s_table[RATE_SEG_THREADS];
    __shared__ int s_top1[RATE_SEG_THREADS], s_bad[RATE_SEG_THREADS];
    const int t = threadIdx.x;
    int64_t a, b;
    rate_seg_bounds(seg_off, blockIdx.x, n, a, b);
    double ideal = 0.0, table = 0.0;
    int top1 = 0, bad = 0;
    for (int64_t i = a + t; i < b; i += RATE_SEG_THREADS) {
        ideal += ws_bits[2 * i];
        table += ws_bits[2 * i + 1];
        const int f = ws_flag[i];
        top1 += f & RATE_FLAG_TOP1;
        bad += (f & RATE_FLAG_BAD) >> 1;
    }
    s_ideal[t] = ideal; s_table[t] = table; s_top1[t] = top1; s_bad[t] = bad;
    rate_block_tree(t, s_ideal, s_table, s_top1, s_bad);
    if (t == 0) {
        scp_rate_seg o;
        o.rows = b - a;
        o.ideal_bits = s_ideal[0];
        o.table_bits = s_table[0];
        o.top1 = s_top1[0];
        o.bad_rows = s_bad[0];
        out[blockIdx.x] = o;
    }
}

static inline int64_t rate_flag_offset(int64_t n) { return 16 * n; }

extern "C" int64_t scp_rate_workspace_bytes(int64_t n, int32_t nseg) {
    if (n < 0 || nseg < 0) return SCP_EINVAL;
    return n == 0 ? 0 : ((17 * n + 255) / 256) * 256;       // two float64 + one flag byte per row
}

extern "C" int scp_rate_segments(const float *logits, int64_t ld, int64_t n, int32_t nsym, const uint8_t *sym, const uint32_t *lohi,
                                 const int64_t *seg_off, int32_t nseg, scp_rate_seg *out, double *row_ideal, double *row_table,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    if (n < 0 || nseg < 0 || nsym < 2 || nsym > 256 || ld < nsym) return SCP_EINVAL;
    if (nseg > 0 && (!seg_off || !out)) return SCP_EINVAL;
    if (n > 0 && (!logits || !sym || !lohi || !workspace || workspace_bytes < scp_rate_workspace_bytes(n, nseg))) return SCP_EINVAL;
    if (n > 0 && (((uintptr_t)workspace) & 7)) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (nseg > 0) HIP_TRY(hipMemsetAsync(out, 0, (size_t)nseg * sizeof(scp_rate_seg), st));
        return SCP_OK;
    }
    double *ws_bits = (double *)workspace;
    uint8_t *ws_flag = (uint8_t *)workspace + rate_flag_offset(n);
    // enough wavefronts to fill the chip several times over; the rest of the rows by stride (the loop keeps the next row in flight)
    const int64_t want = cdiv64(n, RATE_ROWS_PER_BLOCK);
    const unsigned nb = (unsigned)(want < 16384 ? want : 16384);
    SCP_PROF(SCP_PROF_RATE, st, (double)n * (4.0 * nsym + 5.0));
    if (ld == 256 && (((uintptr_t)logits) & 15) == 0)
        hipLaunchKernelGGL(rate_rows_kernel<true>, dim3(nb), dim3(256), 0, st, logits, ld, n, nsym, sym, lohi, ws_bits, ws_flag, row_ideal, row_table);
    else
        hipLaunchKernelGGL(rate_rows_kernel<false>, dim3(nb), dim3(256), 0, st, logits, ld, n, nsym, sym, lohi, ws_bits, ws_flag, row_ideal, row_table);
    LAUNCH_CHECK();
    if (nseg > 0) {
        hipLaunchKernelGGL(rate_segments_kernel, dim3((unsigned)nseg), dim3(RATE_SEG_THREADS), 0, st, ws_bits, ws_flag, seg_off, n, out);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}
