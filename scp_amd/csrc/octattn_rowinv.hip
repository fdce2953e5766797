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
