// OctAttention dual-stream causal attention, row-invariant form (the decodable profile, gfx950).
//
// Same mathematics as csrc/octattn.hip (models/attention_model.py:58-95): for query row t of a window
//   known stream   : softmax_{j <= t}(q_u[t].k[j] / sqrt(hd)) . v
//   unknown stream : the same row with the diagonal score replaced by q_u[t].k_u[t] / sqrt(hd), and v[t] by v_u[t]
// but every output row is ONE fixed arithmetic sequence that reads nothing outside rows 0..t of its own window:
//   - key tiles of KT keys in ascending order from key 0 (tile boundaries are multiples of KT whatever the launch), each
//     folded into the row's flash state (M, L, A) by the same update: M' = max(M, max_j s_j), alpha = exp(M - M'),
//     L' = L alpha + sum_j p_j (j ascending), A' = A alpha then A' = fma(p_j, v_j, A') for j ascending; a tile with no
//     key below t is skipped for that row (no alpha = exp(-inf + inf) and no x * 1 + 0 rewrites);
//   - scores are fp32 FMA chains over the head's channels in ascending order; V is read as fp32 (no scale at all: no f16
//     planes, hence no launch-global max |v| - the f16x3 kernel's V scale is what made a row depend on other windows);
//   - the two diagonal terms close the state last: out = (A a2 + p2 v[t]) / (L a2 + p2) with m2 = max(M, s_diag).
// So a row comes out bit-identical whether the launch covers one window or a hundred, all rows of its window or only
// [q0, q1): the encoder runs it over every row of every window, the decoder over the one row it is decoding (K / V as a
// per-layer cache with a row stride).  Workgroup = QT query rows of one (window, head); 256 threads.
#include "scp_internal.h"

#define RI_QT 32          // query rows per workgroup
#define RI_KT 32          // keys per tile
#define RI_MAXHD 152      // head width limit (LDS: Q, K tiles padded to 153 floats per row, V 152: 62.9 KB)
#define RI_LDQ (RI_MAXHD + 1)
#define RI_NDL ((RI_MAXHD + 31) / 32)
#define RI_NLD ((RI_KT * RI_MAXHD + 255) / 256)   // tile elements per thread

struct RowInvArgs {
    const float *q, *k, *v, *ku, *vu;
    float *out, *out_u;
    int64_t qw, qr, kw, kr, uw, ur, ow, orr;   // window / row strides (floats) of q, k = v (cache), k_u = v_u, out = out_u
    int32_t q0, q1, qoff, H, hd;               // query rows [q0, q1) of every window; row r of q / k_u / v_u / out sits at r - qoff
    float scale;
};

__global__ __launch_bounds__(256) void octattn_rowinv_kernel(const RowInvArgs a) {
    __shared__ float sQ[RI_QT * RI_LDQ];
    __shared__ float sK[RI_KT * RI_LDQ];
    __shared__ float sV[RI_KT * RI_MAXHD];
    __shared__ float sS[RI_QT * (RI_KT + 1)];
    __shared__ float sAlpha[RI_QT], sM[RI_QT], sL[RI_QT], sDiag[2][RI_QT];
    __shared__ int sNk[RI_QT];
    const int tid = threadIdx.x, hd = a.hd, h = blockIdx.y, w = blockIdx.z;
    const int r0 = a.q0 + blockIdx.x * RI_QT;
    const int nq = min(RI_QT, a.q1 - r0);
    const float *kb = a.k + (int64_t)w * a.kw + (int64_t)h * hd;
    const float *vb = a.v + (int64_t)w * a.kw + (int64_t)h * hd;

    for (int i = tid; i < RI_QT * hd; i += 256) {
        const int q = i / hd, d = i - q * hd;
        sQ[q * RI_LDQ + d] = q < nq ? a.q[(int64_t)w * a.qw + (int64_t)(r0 + q - a.qoff) * a.qr + h * hd + d] : 0.f;
    }
    if (tid < RI_QT) { sM[tid] = -INFINITY; sL[tid] = 0.f; }

    // PV ownership: queries qg * 4 .. qg * 4 + 3, channels dl + 32 i
    const int qg = tid >> 5, dl = tid & 31;
    float acc[4][RI_NDL];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < RI_NDL; ++e) acc[i][e] = 0.f;

    const int tmax = r0 + nq - 1;                 // the block's last row attends keys < tmax in the flash pass
    const int ntile = (tmax + RI_KT - 1) / RI_KT;
    for (int kt = 0; kt < ntile; ++kt) {
        const int k0 = kt * RI_KT;
        const int nkt = min(RI_KT, tmax - k0);
        // the tile's K / V rows into registers first: every load in flight at once (and overlapping the previous tile's PV step),
        // instead of one global round trip per element
        float kx[RI_NLD], vx[RI_NLD];
#pragma unroll
        for (int e = 0; e < RI_NLD; ++e) {
            const int i = tid + 256 * e, j = i / hd, d = i - j * hd;
            kx[e] = 0.f;
            vx[e] = 0.f;
            if (i < RI_KT * hd && j < nkt) {
                kx[e] = kb[(int64_t)(k0 + j) * a.kr + d];
                vx[e] = vb[(int64_t)(k0 + j) * a.kr + d];
            }
        }
        __syncthreads();                          // previous tile's sK / sV / sS consumed (and sQ / sM written, first time)
#pragma unroll
        for (int e = 0; e < RI_NLD; ++e) {
            const int i = tid + 256 * e, j = i / hd, d = i - j * hd;
            if (i < RI_KT * hd) {
                sK[j * RI_LDQ + d] = kx[e];
                sV[j * RI_MAXHD + d] = vx[e];
            }
        }
        __syncthreads();
        {   // scores: key j = lane & 31, queries (tid >> 5) + 8 i
            const int j = tid & 31, qs = tid >> 5;
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for (int d = 0; d < hd; ++d) {
                const float kx = sK[j * RI_LDQ + d];
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = fmaf(sQ[(qs + 8 * i) * RI_LDQ + d], kx, s[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) sS[(qs + 8 * i) * (RI_KT + 1) + j] = s[i] * a.scale;
        }
        __syncthreads();
        if (tid < RI_QT) {   // the row's softmax update over this tile's keys j < t
            const int q = tid, t = r0 + q;
            const int nk = (q < nq) ? min(RI_KT, t - k0) : 0;
            if (nk > 0) {
                float sv[RI_KT];                  // the row's scores in registers (one LDS round trip, not 2 nk dependent ones)
#pragma unroll
                for (int j = 0; j < RI_KT; ++j) sv[j] = sS[q * (RI_KT + 1) + j];
                float mt = sv[0];
#pragma unroll
                for (int j = 1; j < RI_KT; ++j)
                    if (j < nk) mt = fmaxf(mt, sv[j]);
                const float M = sM[q], mn = fmaxf(M, mt);
                const float alpha = __expf(M - mn);
                float ps = 0.f;
#pragma unroll
                for (int j = 0; j < RI_KT; ++j) {
                    if (j < nk) {
                        const float p = __expf(sv[j] - mn);
                        sS[q * (RI_KT + 1) + j] = p;
                        ps += p;
                    }
                }
                sL[q] = sL[q] * alpha + ps;
                sM[q] = mn;
                sAlpha[q] = alpha;
            }
            sNk[q] = nk > 0 ? nk : 0;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = qg * 4 + i;
            const int nk = sNk[q];
            if (nk <= 0) continue;
            const float alpha = sAlpha[q];
#pragma unroll
            for (int e = 0; e < RI_NDL; ++e) acc[i][e] *= alpha;
            for (int j = 0; j < nk; ++j) {
                const float p = sS[q * (RI_KT + 1) + j];
#pragma unroll
                for (int e = 0; e < RI_NDL; ++e) {
                    const int d = dl + 32 * e;
                    if (d < hd) acc[i][e] = fmaf(p, sV[j * RI_MAXHD + d], acc[i][e]);
                }
            }
        }
    }
    __syncthreads();
    // the two diagonal scores: q_u[t].k[t] (known stream, only when `out` is wanted) and q_u[t].k_u[t]
    if (tid < 2 * RI_QT) {
        const int q = tid & (RI_QT - 1), which = tid >> 5;
        const bool want = which == 0 ? a.out != nullptr : a.out_u != nullptr;
        float s = 0.f;
        if (q < nq && want) {
            const int t = r0 + q;
            const float *kr = which == 0 ? kb + (int64_t)t * a.kr
                                         : a.ku + (int64_t)w * a.uw + (int64_t)(t - a.qoff) * a.ur + (int64_t)h * hd;
            for (int d = 0; d < hd; ++d) s = fmaf(sQ[q * RI_LDQ + d], kr[d], s);
        }
        sDiag[which][q] = s * a.scale;
    }
    __syncthreads();
    for (int which = 0; which < 2; ++which) {
        float *ob = which == 0 ? a.out : a.out_u;
        if (!ob) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = qg * 4 + i;
            if (q >= nq) continue;
            const int t = r0 + q;
            const float M = sM[q], sd = sDiag[which][q];
            const float m2 = fmaxf(M, sd);
            const float a2 = __expf(M - m2), p2 = __expf(sd - m2);
            const float L2 = sL[q] * a2 + p2;
            const float *vr = which == 0 ? vb + (int64_t)t * a.kr
                                         : a.vu + (int64_t)w * a.uw + (int64_t)(t - a.qoff) * a.ur + (int64_t)h * hd;
            float *orow = ob + (int64_t)w * a.ow + (int64_t)(t - a.qoff) * a.orr + (int64_t)h * hd;
#pragma unroll
            for (int e = 0; e < RI_NDL; ++e) {
                const int d = dl + 32 * e;
                if (d < hd) orow[d] = (acc[i][e] * a2 + p2 * vr[d]) / L2;
            }
        }
    }
}

// B windows; rows [q0, q1) of each.  k / v: [B] x [>= q1 rows] with strides (kw, kr) - the known stream's keys and values of
// rows 0 .. q1 - 1 (a decoder's per-layer cache); q_u, k_u, v_u, out, out_u: row r at index r - qoff.  out or out_u may be NULL
// (that stream is not written; with out == NULL row t of k / v is not read either).  Float strides; unit channel stride.
extern "C" SCP_API int scp_octattn_attention_rowinv(const float *q_u, int64_t qw, int64_t qr, const float *k, const float *v, int64_t kw, int64_t kr,
                                                    const float *k_u, const float *v_u, int64_t uw, int64_t ur, float *out, float *out_u, int64_t ow,
                                                    int64_t orr, int32_t B, int32_t q0, int32_t q1, int32_t qoff, int32_t H, int32_t hd, void *stream) {
    if (!q_u || !k || !v || (!out && !out_u) || (out_u && (!k_u || !v_u)) || B <= 0 || H <= 0 || hd <= 0 || hd > RI_MAXHD || q0 < 0 ||
        q1 <= q0 || qoff < 0 || qoff > q0 || qw < 0 || qr < (int64_t)H * hd || kw < 0 || kr < (int64_t)H * hd || uw < 0 || ur < 0 ||
        ow < 0 || orr < (int64_t)H * hd || (B > 1 && (kw == 0 || ow == 0)))
        return SCP_EINVAL;
    RowInvArgs a;
    a.q = q_u; a.k = k; a.v = v; a.ku = k_u; a.vu = v_u; a.out = out; a.out_u = out_u;
    a.qw = qw; a.qr = qr; a.kw = kw; a.kr = kr; a.uw = uw; a.ur = ur; a.ow = ow; a.orr = orr;
    a.q0 = q0; a.q1 = q1; a.qoff = qoff; a.H = H; a.hd = hd;
    a.scale = 1.0f / sqrtf((float)hd);
    const dim3 grid((unsigned)((q1 - q0 + RI_QT - 1) / RI_QT), (unsigned)H, (unsigned)B);
    hipLaunchKernelGGL(octattn_rowinv_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    LAUNCH_CHECK();
    return SCP_OK;
}

// ------------------------------------------------------------------------------------------------ one query row per stream
// The decoder's lockstep step: launch row s is the current node of one stream; it sits at row t[slot[s]] of the window whose known
// stream's keys / values are cache slot slot[s].  Both arrays live on the device, so nothing about a stream's position is a launch
// argument.  Row s comes out bit-identical to octattn_rowinv_kernel launched with q0 = t, q1 = t + 1 on that cache - the same
// arithmetic sequence (header comment), laid out for ONE query row instead of 32:
//   1. scores: every key j < t is an independent fp32 FMA chain over the head's channels, one key per thread, K staged through LDS
//      in tiles of RS_KT rows (coalesced row reads, conflict-free column reads); the two diagonal scores ride along on idle waves;
//   2. the (M, alpha) recurrence over the <= 32 flash tiles of 32 keys: tile maxima in parallel, the chain on one thread;
//      p_j = exp(s_j - M_tile) by all threads; tile sums in parallel, the L chain by register shuffles inside the idle fourth wave;
//   3. PV: one chain per channel (thread d) over the keys, alpha applied at each tile boundary, the next tile's V rows in flight
//      while the current one is folded in;
//   4. the diagonal term closes the state (m2 / a2 / p2) exactly as above.
// Workgroup = one (stream, head); 256 threads.  Cache rows >= t (> t when `out` is wanted) and slots not listed are never read.
#define RS_KT 128                 // keys per LDS tile of the score pass (128 x 153 floats = 76.5 KB)
#define RS_MAXT 1024              // cache rows limit: the scores of one (stream, head) stay in LDS
#define RS_SI(k) ((k) + ((k) >> 5))   // score k's LDS index: flash tile starts land on different banks
static_assert(RI_MAXHD <= 192, "the fourth wave must stay free of PV work");

struct RowInvStepArgs {
    const float *q, *k, *v, *ku, *vu;
    float *out, *out_u;
    const int32_t *t, *slot;
    int64_t qr, kw, kr, ur, orr;               // row strides of q, k_u = v_u, out = out_u; slot / row stride of the cache (floats)
    int32_t slots, rows, H, hd;
    float scale;
};

__global__ __launch_bounds__(256) void octattn_rowinv_step_kernel(const RowInvStepArgs a) {
    __shared__ float sK[RS_KT * RI_LDQ];
    __shared__ float sQ[RI_MAXHD], sD[2][RI_MAXHD];
    __shared__ float sS[RS_MAXT + RS_MAXT / 32];
    __shared__ float sMt[32], sMn[32], sAlpha[32], sDiag[2], sML[2];
    const int tid = threadIdx.x, hd = a.hd, h = blockIdx.x, s = blockIdx.y;
    const int sl = a.slot[s];
    if (sl < 0 || sl >= a.slots) return;          // (uniform over the workgroup) a slot the cache does not have: the row is left alone
    const int t = a.t[sl];
    if (t < 0 || t >= a.rows) return;
    const float *kb = a.k + (int64_t)sl * a.kw + (int64_t)h * hd;
    const float *vb = a.v + (int64_t)sl * a.kw + (int64_t)h * hd;
    const int wv = tid >> 6, ln = tid & 63;

    for (int d = tid; d < hd; d += 256) {
        sQ[d] = a.q[(int64_t)s * a.qr + (int64_t)h * hd + d];
        sD[0][d] = a.out ? kb[(int64_t)t * a.kr + d] : 0.f;
        sD[1][d] = a.out_u ? a.ku[(int64_t)s * a.ur + (int64_t)h * hd + d] : 0.f;
    }
    __syncthreads();
    if (tid == 128 || tid == 192) {               // the diagonal scores, on the waves the score pass leaves idle
        const int which = tid == 192;
        float sc = 0.f;
        for (int d = 0; d < hd; ++d) sc = fmaf(sQ[d], sD[which][d], sc);
        sDiag[which] = sc * a.scale;
    }
    // 1. scores of the keys below t
    for (int k0 = 0; k0 < t; k0 += RS_KT) {
        const int nkt = min(RS_KT, t - k0);
        __syncthreads();                          // the previous tile is consumed
#pragma unroll 4
        for (int j = wv; j < nkt; j += 4) {
            const float *kr = kb + (int64_t)(k0 + j) * a.kr;
            for (int d = ln; d < hd; d += 64) sK[j * RI_LDQ + d] = kr[d];
        }
        __syncthreads();
        if (tid < nkt) {
            float sc = 0.f;
            for (int d = 0; d < hd; ++d) sc = fmaf(sQ[d], sK[tid * RI_LDQ + d], sc);
            sS[RS_SI(k0 + tid)] = sc * a.scale;
        }
    }
    __syncthreads();
    // 2. flash state over tiles of RI_KT keys
    const int ntile = (t + RI_KT - 1) / RI_KT;
    if (tid < ntile) {
        const int k0 = tid * RI_KT, nk = min(RI_KT, t - k0);
        float mt = sS[RS_SI(k0)];
        for (int j = 1; j < nk; ++j) mt = fmaxf(mt, sS[RS_SI(k0 + j)]);
        sMt[tid] = mt;
    }
    __syncthreads();
    if (tid == 0) {
        float M = -INFINITY;
        for (int i = 0; i < ntile; ++i) {
            const float mn = fmaxf(M, sMt[i]);
            sAlpha[i] = __expf(M - mn);
            sMn[i] = mn;
            M = mn;
        }
        sML[0] = M;
    }
    __syncthreads();
    for (int k = tid; k < t; k += 256) sS[RS_SI(k)] = __expf(sS[RS_SI(k)] - sMn[k >> 5]);
    __syncthreads();
    float acc = 0.f;
    if (wv == 3) {                                // L' = L alpha + sum_j p_j: lane i sums tile i, the chain runs on shuffled values
        float ps = 0.f, al = 0.f;
        if (ln < ntile) {
            const int k0 = ln * RI_KT, nk = min(RI_KT, t - k0);
            for (int j = 0; j < nk; ++j) ps += sS[RS_SI(k0 + j)];
            al = sAlpha[ln];
        }
        float L = 0.f;
        for (int i = 0; i < ntile; ++i) L = L * __shfl(al, i) + __shfl(ps, i);
        if (ln == 0) sML[1] = L;
    } else if (tid < hd) {
        // 3. PV: channel tid of the head
        float vn[RI_KT];
#pragma unroll
        for (int j = 0; j < RI_KT; ++j) vn[j] = j < t ? vb[(int64_t)j * a.kr + tid] : 0.f;
        for (int i = 0; i < ntile; ++i) {
            const int k0 = i * RI_KT, nk = min(RI_KT, t - k0);
            float vx[RI_KT];
#pragma unroll
            for (int j = 0; j < RI_KT; ++j) vx[j] = vn[j];
#pragma unroll
            for (int j = 0; j < RI_KT; ++j) vn[j] = k0 + RI_KT + j < t ? vb[(int64_t)(k0 + RI_KT + j) * a.kr + tid] : 0.f;
            acc *= sAlpha[i];
#pragma unroll
            for (int j = 0; j < RI_KT; ++j)
                if (j < nk) acc = fmaf(sS[RS_SI(k0 + j)], vx[j], acc);
        }
    }
    __syncthreads();
    // 4. the diagonal term
    if (tid < hd) {
        const float M = sML[0], L = sML[1];
        for (int which = 0; which < 2; ++which) {
            float *ob = which == 0 ? a.out : a.out_u;
            if (!ob) continue;
            const float sd = sDiag[which];
            const float m2 = fmaxf(M, sd);
            const float a2 = __expf(M - m2), p2 = __expf(sd - m2);
            const float L2 = L * a2 + p2;
            const float vr = which == 0 ? vb[(int64_t)t * a.kr + tid] : a.vu[(int64_t)s * a.ur + (int64_t)h * hd + tid];
            ob[(int64_t)s * a.orr + (int64_t)h * hd + tid] = (acc * a2 + p2 * vr) / L2;
        }
    }
}

// S launch rows, one query row each.  q_u, k_u, v_u, out, out_u: row s at s * (their row stride).  k / v: the known stream's cache,
// `slots` windows of `rows` rows (slot stride kw, row stride kr); launch row s reads rows 0 .. t[slot[s]] - 1 of slot slot[s] (and
// row t itself when `out` is wanted).  t int32 [slots] and slot int32 [S] are DEVICE arrays.  A row whose slot lies outside
// [0, slots) or whose t lies outside [0, rows) is not written.
extern "C" SCP_API int scp_octattn_attention_rowinv_step(const float *q_u, int64_t qr, const float *k, const float *v, int64_t kw, int64_t kr,
                                                         int32_t slots, int32_t rows, const float *k_u, const float *v_u, int64_t ur, float *out,
                                                         float *out_u, int64_t orr, const int32_t *t, const int32_t *slot, int32_t S, int32_t H,
                                                         int32_t hd, void *stream) {
    if (!q_u || !k || !v || !t || !slot || (!out && !out_u) || (out_u && (!k_u || !v_u)) || S <= 0 || H <= 0 || hd <= 0 || hd > RI_MAXHD ||
        slots <= 0 || rows <= 0 || rows > RS_MAXT || qr < (int64_t)H * hd || kr < (int64_t)H * hd || kw < 0 || (slots > 1 && kw < (int64_t)rows * kr) ||
        (out_u && ur < (int64_t)H * hd) || orr < (int64_t)H * hd)
        return SCP_EINVAL;
    RowInvStepArgs a;
    a.q = q_u; a.k = k; a.v = v; a.ku = k_u; a.vu = v_u; a.out = out; a.out_u = out_u; a.t = t; a.slot = slot;
    a.qr = qr; a.kw = kw; a.kr = kr; a.ur = ur; a.orr = orr;
    a.slots = slots; a.rows = rows; a.H = H; a.hd = hd;
    a.scale = 1.0f / sqrtf((float)hd);
    hipLaunchKernelGGL(octattn_rowinv_step_kernel, dim3((unsigned)H, (unsigned)S), dim3(256), 0, (hipStream_t)stream, a);
    LAUNCH_CHECK();
    return SCP_OK;
}
