// Chunk-parallel range coder (include/scp.h, "Chunk-parallel range coder"; DESIGN.md 6, "Chunked payloads"), gfx950.  A payload of n
// symbols is cut by symbol index into C = ceil(n / N) chunks, every chunk an independently terminated stream of the host coder
// (rangecoder.cpp on the slice), so all chunks of a payload are coded, and decoded, at once: one lane per chunk, the step being
// ac_chunk.h's restatement of the host coder.  Nothing here knows about attributes: pairs in, bytes out; bytes, tables and contexts in,
// symbols out.
//
//   scp_ac_chunks_encode_lohi   acc_encode_kernel  one lane per chunk into a private slot of acc_slot_bytes(N) bytes (the bound is derived
//                                                  in ac_chunk.h; every store is checked against it anyway), whole words only;
//                               acc_scan_kernel    one workgroup: exclusive scan of the lengths -> offsets int64 [C + 1], the total
//                                                  against `cap`;
//                               acc_pack_kernel    workgroups copy slot c to out + offsets[c]: aligned destination words assembled from
//                                                  two aligned slot words, the ragged head and tail by bytes.  Nothing is written
//                                                  when the total exceeds cap.
//   scp_ac_chunks_decode_ctx    acc_decode_kernel  the tables and the context -> table map go into LDS once per workgroup (one wave), then
//                                                  one lane per chunk: exact division (acc_div), the host's binary search on the LDS row;
//                                                  the chunk's bytes and the contexts are fetched one step ahead of their use.
//
// Lanes of a wave run different chunks, so the two renormalisation branches, the pending bursts and the search diverge; that is the
// price of a serial coder per lane and is accepted - the parallelism is across chunks.  A lane strides through lohi / ctx / sym at
// N elements, one cache line per lane and 16 (pairs) to 64 (contexts) symbols per line; the pairs are read as 16-byte vectors where the
// chunk start is 16-byte aligned.
#include "scp_internal.h"
#include "ac_chunk.h"

#define ACC_WAVE 64
#define ACC_COPY_THREADS 256
#define ACC_LDS_MAX 65536

namespace {

__global__ __launch_bounds__(ACC_WAVE) void acc_encode_kernel(const uint32_t *__restrict__ lohi, int64_t n, int N, int64_t C, int64_t slot,
                                                              uint8_t *__restrict__ slots, uint32_t *__restrict__ lengths, int32_t *__restrict__ status) {
    const int64_t c = (int64_t)blockIdx.x * ACC_WAVE + threadIdx.x;
    if (c >= C) return;
    const int64_t b = c * N;
    const int64_t m = (n - b < N ? n - b : (int64_t)N);
    const uint32_t *p = lohi + b;
    acc_enc e;
    acc_enc_init(e, (uint32_t *)(slots + c * slot), slot);
    int64_t i = 0;
    if (((uintptr_t)p & 15) == 0) {
        for (; i + 4 <= m; i += 4) {
            const uint4 v = *(const uint4 *)(p + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t hi = w[t] >> 16;
                acc_enc_step(e, w[t] & 0xFFFFu, hi ? hi : 0x10000u);
            }
        }
    }
    for (; i < m; ++i) {
        const uint32_t v = p[i], hi = v >> 16;
        acc_enc_step(e, v & 0xFFFFu, hi ? hi : 0x10000u);
    }
    lengths[c] = acc_enc_flush(e);
    if (e.overflow) *status = SCP_ESMALL;
}

__global__ __launch_bounds__(ACC_COPY_THREADS) void acc_scan_kernel(const uint32_t *__restrict__ lengths, int64_t C, int64_t cap, int64_t *__restrict__ offsets,
                                                                    int32_t *__restrict__ status) {
    __shared__ int64_t s[ACC_COPY_THREADS];
    const int t = threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < C; base += ACC_COPY_THREADS) {
        const int64_t i = base + t;
        const int64_t x = i < C ? (int64_t)lengths[i] : 0;
        s[t] = x;
        __syncthreads();
        for (int o = 1; o < ACC_COPY_THREADS; o <<= 1) {
            const int64_t y = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += y;
            __syncthreads();
        }
        if (i < C) offsets[i] = carry + s[t] - x;
        carry += s[ACC_COPY_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) {
        offsets[C] = carry;
        if (carry > cap) *status = SCP_ESMALL;
    }
}

__global__ __launch_bounds__(ACC_COPY_THREADS) void acc_pack_kernel(const uint8_t *__restrict__ slots, int64_t slot, const int64_t *__restrict__ offsets, int64_t C,
                                                                    int64_t cap, uint8_t *__restrict__ out) {
    if (offsets[C] > cap) return;                                    // SCP_ESMALL (acc_scan_kernel): nothing is written
    const int64_t c = blockIdx.x;
    const int64_t off = offsets[c];
    int64_t len = offsets[c + 1] - off;
    if (len > slot) len = slot;                                      // (a slot that overflowed: SCP_ESMALL as well; reads stay inside it)
    const uint8_t *src = slots + c * slot;
    const uint32_t *srcw = (const uint32_t *)src;
    const int64_t end = off + len;
    const int64_t w0 = (off + 3) >> 2, w1 = end >> 2;                // whole destination words [w0, w1)
    const int64_t stride = (int64_t)gridDim.y * ACC_COPY_THREADS;
    const int64_t t = (int64_t)blockIdx.y * ACC_COPY_THREADS + threadIdx.x;
    if (w0 >= w1) {                                                  // no whole word: bytes
        for (int64_t j = t; j < len; j += stride) out[off + j] = src[j];
        return;
    }
    uint32_t *outw = (uint32_t *)out;                                // `out` is 4-byte aligned (checked by the entry)
    for (int64_t j = w0 + t; j < w1; j += stride) {
        const int64_t pos = 4 * j - off;                             // 0 <= pos, pos + 4 <= len
        const int64_t sw = pos >> 2;
        const int sh = (int)(pos & 3) * 8;
        // sh != 0: byte pos + 3 < len lies in word sw + 1, which therefore starts inside the slot (a whole number of words)
        outw[j] = sh ? (srcw[sw] >> sh) | (srcw[sw + 1] << (32 - sh)) : srcw[sw];
    }
    if (t < 4) {
        const int64_t head = 4 * w0 - off, tail0 = 4 * w1 - off;     // bytes [0, head) and [tail0, len)
        if (t < head) out[off + t] = src[t];
        if (tail0 + t < len) out[off + tail0 + t] = src[tail0 + t];
    }
}

__global__ __launch_bounds__(ACC_WAVE) void acc_decode_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ offsets, int64_t n, int N, int64_t C,
                                                              const uint16_t *__restrict__ tables, int ntab, int Lp, const uint8_t *__restrict__ table_of, int nctx,
                                                              const uint8_t *__restrict__ ctx, int16_t *__restrict__ sym) {
    extern __shared__ uint32_t acc_lds[];
    uint16_t *tab = (uint16_t *)acc_lds;                             // [ntab][Lp], then the map uint8 [nctx] (clamped below ntab)
    const int words = (ntab * Lp + 1) / 2;
    uint8_t *map = (uint8_t *)(acc_lds + words);
    const int total = ntab * Lp;
    if (((uintptr_t)tables & 3) == 0) {
        const uint32_t *tw = (const uint32_t *)tables;
        for (int i = threadIdx.x; i < total / 2; i += ACC_WAVE) acc_lds[i] = tw[i];
        if ((total & 1) && threadIdx.x == 0) tab[total - 1] = tables[total - 1];
    } else {
        for (int i = threadIdx.x; i < total; i += ACC_WAVE) tab[i] = tables[i];
    }
    for (int i = threadIdx.x; i < nctx; i += ACC_WAVE) {
        const int g = table_of[i];
        map[i] = (uint8_t)(g < ntab ? g : ntab - 1);
    }
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * ACC_WAVE + threadIdx.x;
    if (c >= C) return;
    const int64_t b = c * N;
    const int64_t m = (n - b < N ? n - b : (int64_t)N);
    const int64_t o0 = offsets[c], o1 = offsets[c + 1];
    acc_dec d;
    acc_dec_init(d, bytes + o0, o1 - o0);
    const uint8_t *cx = ctx + b;
    int16_t *out = sym + b;
    const int max_symbol = Lp - 2;
    int64_t i = 0;
    if (((uintptr_t)cx & 15) == 0 && m >= 16) {
        // 16 contexts per load, the next 16 fetched while these are decoded: like the chunk's bytes (acc_dec.next) they are in registers
        // before a symbol needs them, so a symbol waits for LDS only
        uint4 cur = *(const uint4 *)cx;
        for (; i + 16 <= m; i += 16) {
            uint4 nxt = cur;
            if (i + 32 <= m) nxt = *(const uint4 *)(cx + i + 16);
#pragma unroll 1
            for (int j = 0; j < 16; ++j) {
                int k = (int)(cur.x & 0xFFu);
                cur.x = (cur.x >> 8) | (cur.y << 24);
                cur.y = (cur.y >> 8) | (cur.z << 24);
                cur.z = (cur.z >> 8) | (cur.w << 24);
                cur.w >>= 8;
                k = k < nctx ? k : nctx - 1;
                out[i + j] = (int16_t)acc_dec_step(d, (const uint16_t *)(tab + (int)map[k] * Lp), max_symbol);
            }
            cur = nxt;
        }
    }
    for (; i < m; ++i) {
        int k = cx[i];
        k = k < nctx ? k : nctx - 1;
        out[i] = (int16_t)acc_dec_step(d, (const uint16_t *)(tab + (int)map[k] * Lp), max_symbol);
    }
}

bool acc_sizes_ok(int64_t n, int64_t N) { return n >= 0 && n <= (1ll << 31) && N >= ACC_MIN_CHUNK && N <= ACC_MAX_CHUNK; }

}  // namespace

extern "C" int64_t scp_ac_chunks_workspace_bytes(int64_t n, int64_t N) {
    if (!acc_sizes_ok(n, N)) return SCP_EINVAL;
    const int64_t C = cdiv64(n, N);
    return (C + 1) * 8 + C * acc_slot_bytes(N);
}

extern "C" int scp_ac_chunks_encode_lohi(const uint32_t *lohi, int64_t n, int64_t N, uint32_t *lengths, uint8_t *out, int64_t cap, int32_t *status,
                                         void *workspace, int64_t workspace_bytes, void *stream) {
    if (!acc_sizes_ok(n, N) || cap < 0 || !status || ((uintptr_t)out & 3) || ((uintptr_t)lohi & 3)) return SCP_EINVAL;
    if (n > 0 && (!lohi || !lengths || (!out && cap > 0))) return SCP_EINVAL;
    const int64_t need = scp_ac_chunks_workspace_bytes(n, N);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return SCP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    if (n == 0) return SCP_OK;
    const int64_t C = cdiv64(n, N), slot = acc_slot_bytes(N);
    int64_t *offsets = (int64_t *)workspace;
    uint8_t *slots = (uint8_t *)workspace + (C + 1) * 8;
    hipLaunchKernelGGL(acc_encode_kernel, dim3((unsigned)cdiv64(C, ACC_WAVE)), dim3(ACC_WAVE), 0, st, lohi, n, (int)N, C, slot, slots, lengths, status);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(acc_scan_kernel, dim3(1), dim3(ACC_COPY_THREADS), 0, st, (const uint32_t *)lengths, C, cap, offsets, status);
    LAUNCH_CHECK();
    int64_t gy = slot / (ACC_COPY_THREADS * 4 * 8);
    gy = gy < 1 ? 1 : (gy > 32 ? 32 : gy);
    hipLaunchKernelGGL(acc_pack_kernel, dim3((unsigned)C, (unsigned)gy), dim3(ACC_COPY_THREADS), 0, st, (const uint8_t *)slots, slot, (const int64_t *)offsets, C, cap, out);
    LAUNCH_CHECK();
    return SCP_OK;
}

extern "C" int scp_ac_chunks_decode_ctx(const uint8_t *bytes, const int64_t *offsets, int64_t n, int64_t N, const uint16_t *tables, int32_t ntab, int32_t Lp,
                                        const uint8_t *table_of, int32_t nctx, const uint8_t *ctx, int16_t *sym, void *stream) {
    if (!acc_sizes_ok(n, N) || ntab < 1 || ntab > 256 || Lp < 2 || Lp > 32768 || nctx < 1 || nctx > 256) return SCP_EINVAL;
    if (!offsets || !tables || !table_of || (n > 0 && (!ctx || !sym)) || ((uintptr_t)tables & 1) || ((uintptr_t)offsets & 7)) return SCP_EINVAL;
    const int64_t lds = (((int64_t)ntab * Lp + 1) / 2) * 4 + ((nctx + 3) / 4) * 4;
    if (lds > ACC_LDS_MAX) return SCP_EINVAL;
    if (n == 0) return SCP_OK;
    const int64_t C = cdiv64(n, N);
    hipLaunchKernelGGL(acc_decode_kernel, dim3((unsigned)cdiv64(C, ACC_WAVE)), dim3(ACC_WAVE), (size_t)lds, (hipStream_t)stream, bytes, offsets, n, (int)N, C, tables,
                       (int)ntab, (int)Lp, table_of, (int)nctx, ctx, sym);
    LAUNCH_CHECK();
    return SCP_OK;
}
