// What the attribute layers share (csrc/attr.hip: reflectance, csrc/color.hip: colour): the tree of a Morton-ordered leaf list -
// keys, per level head flags, a three-launch scan and the entry lists (key, first) with their counts on the device - the workspace layout,
// the <= 8 children of a parent by slot, the quantisation step and the pair order of the three lifting stages.  Whoever builds the tree or
// evaluates a step through these gets the same entries and the same bits.
#pragma once
#include "scp_internal.h"

#define AT_THREADS 256
#define AT_ITEMS 4
#define AT_TILE (AT_THREADS * AT_ITEMS)

namespace {

struct at_layout {
    int64_t cap[SCP_MAX_DEPTH + 1], off[SCP_MAX_DEPTH + 1];
    int64_t total, nblk;
    int64_t b_counts, b_key, b_first, b_w, b_val, b_bsum, bytes;
};

// level j holds at most min(U, 8^(D-j)) entries (keys are masked to 3 D bits)
bool at_make_layout(int64_t U, int D, at_layout &L) {
    if (U < 0 || U - 1 > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH) return false;
    int64_t t = 0;
    for (int j = 0; j <= D; ++j) {
        const int sh = 3 * (D - j);
        const int64_t full = sh >= 40 ? INT64_MAX : (1ll << sh);
        L.cap[j] = U < full ? U : full;
        L.off[j] = t;
        t += L.cap[j];
    }
    L.total = t;
    L.nblk = cdiv64(U > 0 ? U : 1, AT_TILE);
    int64_t b = 0;
    L.b_counts = b; b += 8 * (SCP_MAX_DEPTH + 3);
    L.b_key = b;    b += 8 * t;
    L.b_first = b;  b += 4 * t;
    L.b_w = b;      b += 4 * t;
    L.b_val = b;    b += 4 * t;
    L.b_bsum = b;   b += 4 * (L.nblk + 1);
    L.bytes = (b + 7) & ~7ll;
    return true;
}

__device__ __forceinline__ uint64_t at_morton(int32_t x, int32_t y, int32_t z, int D) {
    uint64_t k = 0;
    for (int b = 0; b < D; ++b)
        k |= (uint64_t)((((uint32_t)x >> b) & 1u) * 4u + (((uint32_t)y >> b) & 1u) * 2u + (((uint32_t)z >> b) & 1u)) << (3 * b);
    return k;
}

__device__ __forceinline__ int64_t at_floordiv(int64_t a, int64_t b) {      // b > 0
    int64_t q = a / b;
    if (a % b < 0) --q;
    return q;
}

// step(w1, w2) = max(1, isqrt((Q Q (w1 + w2)) // (w1 w2))); the quotient is at most 2 Q Q = 130 050, exact in a float
__device__ __forceinline__ uint32_t at_step(uint32_t w1, uint32_t w2, uint32_t Q) {
    const uint64_t x = ((uint64_t)Q * Q * ((uint64_t)w1 + w2)) / ((uint64_t)w1 * w2);
    uint32_t r = (uint32_t)__builtin_sqrtf((float)x);
    while ((uint64_t)r * r > x) --r;
    while ((uint64_t)(r + 1) * (r + 1) <= x) ++r;
    return r < 1u ? 1u : r;
}

// exclusive scan of one value per thread over the 256 threads of a block
__device__ __forceinline__ uint32_t at_block_scan(uint32_t x, uint32_t *s, uint32_t &total) {
    const int t = threadIdx.x;
    s[t] = x;
    __syncthreads();
    for (int o = 1; o < AT_THREADS; o <<= 1) {
        const uint32_t y = t >= o ? s[t - o] : 0u;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    total = s[AT_THREADS - 1];
    const uint32_t incl = s[t];
    __syncthreads();
    return incl - x;
}

__global__ __launch_bounds__(AT_THREADS) void attr_keys_kernel(const int32_t *__restrict__ leaves, int64_t U, int D, uint64_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i < U) key[i] = at_morton(leaves[3 * i], leaves[3 * i + 1], leaves[3 * i + 2], D);
}

__global__ __launch_bounds__(AT_THREADS) void attr_level0_kernel(const uint8_t *__restrict__ a, int64_t U, uint32_t *__restrict__ w, int32_t *__restrict__ val,
                                                                 int64_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i == 0) counts[0] = U;
    if (i < U) {
        w[i] = 1u;
        if (a) val[i] = (int32_t)a[i];
    }
}

__device__ __forceinline__ uint32_t at_head(const uint64_t *key, int64_t e) { return (e == 0 || (key[e] >> 3) != (key[e - 1] >> 3)) ? 1u : 0u; }

__global__ __launch_bounds__(AT_THREADS) void attr_count_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ n_prev_p, uint32_t *__restrict__ bsum) {
    __shared__ uint32_t s[AT_THREADS];
    const int64_t n = *n_prev_p;
    const int64_t e0 = ((int64_t)blockIdx.x * AT_THREADS + threadIdx.x) * AT_ITEMS;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < AT_ITEMS; ++i)
        if (e0 + i < n) c += at_head(key, e0 + i);
    uint32_t total;
    at_block_scan(c, s, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: exclusive scan of the block counts in place, the level's entry count to *count_out
__global__ __launch_bounds__(AT_THREADS) void attr_scan_kernel(uint32_t *bsum, int64_t nblk_cap, const int64_t *__restrict__ n_prev_p, int64_t *count_out) {
    __shared__ uint32_t s[AT_THREADS];
    int64_t nblk = (*n_prev_p + AT_TILE - 1) / AT_TILE;
    if (nblk > nblk_cap) nblk = nblk_cap;
    uint32_t carry = 0;
    for (int64_t base = 0; base < nblk; base += AT_THREADS) {
        const int64_t i = base + threadIdx.x;
        const uint32_t x = i < nblk ? bsum[i] : 0u;
        uint32_t total;
        const uint32_t ex = at_block_scan(x, s, total);
        if (i < nblk) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *count_out = (int64_t)carry;
}

__global__ __launch_bounds__(AT_THREADS) void attr_assign_kernel(const uint64_t *__restrict__ key, const int64_t *__restrict__ n_prev_p, const uint32_t *__restrict__ bsum,
                                                                 int64_t cap_j, uint32_t *__restrict__ first_j, uint64_t *__restrict__ key_j) {
    __shared__ uint32_t s[AT_THREADS];
    const int64_t n = *n_prev_p;
    const int64_t e0 = ((int64_t)blockIdx.x * AT_THREADS + threadIdx.x) * AT_ITEMS;
    uint32_t f[AT_ITEMS], c = 0;
#pragma unroll
    for (int i = 0; i < AT_ITEMS; ++i) {
        f[i] = e0 + i < n ? at_head(key, e0 + i) : 0u;
        c += f[i];
    }
    uint32_t total;
    uint32_t p = at_block_scan(c, s, total) + bsum[blockIdx.x];
#pragma unroll
    for (int i = 0; i < AT_ITEMS; ++i) {
        if (f[i]) {
            if ((int64_t)p < cap_j) {
                first_j[p] = (uint32_t)(e0 + i);
                key_j[p] = key[e0 + i] >> 3;
            }
            ++p;
        }
    }
}

// the <= 8 children of parent p, by slot; w == 0 marks an empty slot
struct at_children {
    int64_t b;          // first child
    int n;              // children read (<= 8)
    int32_t v[8];
    uint32_t w[8];
    uint32_t slot_of[8];
};

template <bool VALUES>
__device__ __forceinline__ void at_load(at_children &c, int64_t p, int64_t n_j, int64_t n_prev, const uint32_t *first_j, const uint64_t *key_c,
                                        const uint32_t *w_c, const int32_t *val_c) {
    c.b = (int64_t)first_j[p];
    int64_t end = p + 1 < n_j ? (int64_t)first_j[p + 1] : n_prev;
    if (end > n_prev) end = n_prev;
    int64_t n = end - c.b;
    c.n = (int)(n < 0 ? 0 : (n > 8 ? 8 : n));
#pragma unroll
    for (int s = 0; s < 8; ++s) { c.v[s] = 0; c.w[s] = 0u; c.slot_of[s] = 8u; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < c.n) {
            const uint32_t slot = (uint32_t)(key_c[c.b + i] & 7u);
            const uint32_t w = w_c[c.b + i];
            const int32_t v = VALUES ? val_c[c.b + i] : 0;
            c.slot_of[i] = slot;
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (slot == (uint32_t)s) { c.v[s] = v; c.w[s] = w; }
        }
    }
}

// pair t of the coding order: stage 3 (bit 4, lo 0), stage 2 (bit 2, lo 0 and 4), stage 1 (bit 1, lo 0, 2, 4, 6)
#define AT_PAIR_LO(t) ((t) == 0 ? 0 : (t) == 1 ? 0 : (t) == 2 ? 4 : 2 * ((t) - 3))
#define AT_PAIR_BIT(t) ((t) == 0 ? 4 : (t) <= 2 ? 2 : 1)

inline unsigned at_grid(int64_t n, int64_t per) {
    const int64_t b = cdiv64(n > 0 ? n : 1, per);
    return (unsigned)b;
}

// keys, level 0 and the levels' entry lists (key, first) with their counts; U >= 1
int at_build_tree(const int32_t *leaves, const uint8_t *a, int64_t U, int D, const at_layout &L, uint8_t *ws, hipStream_t st) {
    int64_t *counts = (int64_t *)(ws + L.b_counts);
    uint64_t *key = (uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w), *bsum = (uint32_t *)(ws + L.b_bsum);
    int32_t *val = (int32_t *)(ws + L.b_val);
    hipLaunchKernelGGL(attr_keys_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, leaves, U, D, key);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(attr_level0_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, a, U, w, val, counts);
    LAUNCH_CHECK();
    for (int j = 1; j <= D; ++j) {
        const uint64_t *key_c = key + L.off[j - 1];
        const unsigned nb = at_grid(L.cap[j - 1], AT_TILE);
        hipLaunchKernelGGL(attr_count_kernel, dim3(nb), dim3(AT_THREADS), 0, st, key_c, counts + (j - 1), bsum);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(attr_scan_kernel, dim3(1), dim3(AT_THREADS), 0, st, bsum, (int64_t)nb, counts + (j - 1), counts + j);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(attr_assign_kernel, dim3(nb), dim3(AT_THREADS), 0, st, key_c, counts + (j - 1), bsum, L.cap[j], first + L.off[j], key + L.off[j]);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

bool at_ws_ok(const void *ws, int64_t bytes, int64_t need) { return ws && (((uintptr_t)ws) & 7) == 0 && bytes >= need; }

}  // namespace
