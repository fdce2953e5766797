// What the attribute layers share (csrc/attr.hip: reflectance, csrc/color.hip: colour): the tree of a Morton-ordered leaf list -
// keys, per level head flags, a three-launch scan and the entry lists (key, first) with their counts on the device - the workspace layout,
// the <= 8 children of a parent by slot, the quantisation step, the pair order of the three lifting stages, a point's leaf and a leaf's
// rounded mean.  Whoever builds the tree or evaluates a step through these gets the same entries and the same bits.  The lifting itself,
// for any number of channels on this tree: lift.h.
//
// No access leaves the buffers, whatever the leaves: the scan stores a level's entry count clamped to the level's capacity in the
// workspace (at_make_layout), every later kernel reads that count, and the count as scanned goes to a second row that only the host reads.
#pragma once
#include "scp_internal.h"

#define AT_THREADS 256
#define AT_ITEMS 4
#define AT_TILE (AT_THREADS * AT_ITEMS)
#define AT_COUNT_ROW (SCP_MAX_DEPTH + 3)        // counts[j]: entries of level j, clamped; counts[AT_COUNT_ROW + j]: as scanned

namespace {

struct at_layout {
    int64_t cap[SCP_MAX_DEPTH + 1], off[SCP_MAX_DEPTH + 1];
    int64_t total, nblk;
    int64_t b_counts, b_key, b_first, b_w, b_val, b_bsum, bytes;
};

// level 0 holds the U leaves, level j >= 1 at most min(U, 8^(D-j)) entries (keys are masked to 3 D bits)
bool at_make_layout(int64_t U, int D, at_layout &L) {
    if (U < 0 || U - 1 > (1ll << 31) || D < 1 || D > SCP_MAX_DEPTH) return false;
    int64_t t = 0;
    for (int j = 0; j <= D; ++j) {
        const int sh = 3 * (D - j);
        const int64_t full = sh >= 40 ? INT64_MAX : (1ll << sh);
        L.cap[j] = (j == 0 || U < full) ? U : full;
        L.off[j] = t;
        t += L.cap[j];
    }
    L.total = t;
    L.nblk = cdiv64(U > 0 ? U : 1, AT_TILE);
    int64_t b = 0;
    L.b_counts = b; b += 8 * 2 * AT_COUNT_ROW;
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

// first leaf with key k, or -1 if the cell (x, y, z) is outside 0 .. 2^D - 1 or no leaf
__device__ __forceinline__ int64_t at_find_leaf(const uint64_t *__restrict__ key, int64_t U, int32_t x, int32_t y, int32_t z, int D) {
    if ((x | y | z) < 0 || (((int64_t)x | (int64_t)y | (int64_t)z) >> D) != 0) return -1;
    const uint64_t k = at_morton(x, y, z, D);
    int64_t lo = 0, hi = U;                         // first leaf with key >= k
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < U && key[lo] == k ? lo : -1;
}

// (2 sum + cnt) // (2 cnt) of 8-bit values, 0 where cnt <= 0
__device__ __forceinline__ int32_t at_round_mean(unsigned long long sum, int32_t cnt) {
    const unsigned long long c = (unsigned long long)(cnt > 0 ? cnt : 0);
    const unsigned long long m = c ? (2ull * sum + c) / (2ull * c) : 0ull;
    return (int32_t)(m > 255ull ? 255ull : m);
}

// the keys of the leaves; with w and counts also level 0 of a tree: weight 1 per leaf, U entries
__global__ __launch_bounds__(AT_THREADS) void attr_keys_kernel(const int32_t *__restrict__ leaves, int64_t U, int D, uint64_t *__restrict__ key,
                                                               uint32_t *__restrict__ w, int64_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i == 0 && counts) counts[0] = counts[AT_COUNT_ROW] = U;
    if (i < U) {
        key[i] = at_morton(leaves[3 * i], leaves[3 * i + 1], leaves[3 * i + 2], D);
        if (w) w[i] = 1u;
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

// one block: exclusive scan of the block counts in place; the level's entry count, clamped to the level's capacity, to counts[j] - what
// every later kernel reads, so that no index derived from it leaves the level - and the count as scanned to the second row
__global__ __launch_bounds__(AT_THREADS) void attr_scan_kernel(uint32_t *bsum, int64_t nblk_cap, int64_t cap_j, int64_t *counts, int j) {
    __shared__ uint32_t s[AT_THREADS];
    int64_t nblk = (counts[j - 1] + AT_TILE - 1) / AT_TILE;
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
    if (threadIdx.x == 0) {
        counts[j] = (int64_t)carry < cap_j ? (int64_t)carry : cap_j;
        counts[AT_COUNT_ROW + j] = (int64_t)carry;
    }
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

// the <= 8 children of parent p, by slot, with their values of C planes (C = 0: weights and slots only); w == 0 marks an empty slot
template <int C>
struct at_children {
    int64_t b;          // first child
    int n;              // children read (<= 8)
    int32_t v[C > 0 ? C : 1][8];
    uint32_t w[8];
    uint32_t slot_of[8];
};

// val_c[ch]: the children's level of plane ch.  A value goes to its slot under the comparison that places the weight, and lives in the
// struct beside it: placed in a pass of their own, the 64 comparisons stay live as scalar masks (72 spilled SGPRs and one wave less per
// SIMD in the one-plane lift kernel), and in an array of the caller's the same kernel comes out 3 % longer.
template <int C>
__device__ __forceinline__ void at_load(at_children<C> &c, int64_t p, int64_t n_j, int64_t n_prev, const uint32_t *first_j, const uint64_t *key_c,
                                        const uint32_t *w_c, int32_t *const *val_c = nullptr) {
    c.b = (int64_t)first_j[p];
    int64_t end = p + 1 < n_j ? (int64_t)first_j[p + 1] : n_prev;
    if (end > n_prev) end = n_prev;
    int64_t n = end - c.b;
    c.n = (int)(n < 0 ? 0 : (n > 8 ? 8 : n));
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) c.v[ch][s] = 0;
        c.w[s] = 0u;
        c.slot_of[s] = 8u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < c.n) {
            const uint32_t slot = (uint32_t)(key_c[c.b + i] & 7u);
            const uint32_t w = w_c[c.b + i];
            int32_t x[C > 0 ? C : 1];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) x[ch] = val_c[ch][c.b + i];
            c.slot_of[i] = slot;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (slot == (uint32_t)s) {
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) c.v[ch][s] = x[ch];
                    c.w[s] = w;
                }
            }
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

// keys, level 0 (weights) and the levels' entry lists (key, first) with their counts; U >= 1
int at_build_tree(const int32_t *leaves, int64_t U, int D, const at_layout &L, uint8_t *ws, hipStream_t st) {
    int64_t *counts = (int64_t *)(ws + L.b_counts);
    uint64_t *key = (uint64_t *)(ws + L.b_key);
    uint32_t *first = (uint32_t *)(ws + L.b_first), *w = (uint32_t *)(ws + L.b_w), *bsum = (uint32_t *)(ws + L.b_bsum);
    hipLaunchKernelGGL(attr_keys_kernel, dim3(at_grid(U, AT_THREADS)), dim3(AT_THREADS), 0, st, leaves, U, D, key, w, counts);
    LAUNCH_CHECK();
    for (int j = 1; j <= D; ++j) {
        const uint64_t *key_c = key + L.off[j - 1];
        const unsigned nb = at_grid(L.cap[j - 1], AT_TILE);
        hipLaunchKernelGGL(attr_count_kernel, dim3(nb), dim3(AT_THREADS), 0, st, key_c, counts + (j - 1), bsum);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(attr_scan_kernel, dim3(1), dim3(AT_THREADS), 0, st, bsum, (int64_t)nb, L.cap[j], counts, j);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(attr_assign_kernel, dim3(nb), dim3(AT_THREADS), 0, st, key_c, counts + (j - 1), bsum, L.cap[j], first + L.off[j], key + L.off[j]);
        LAUNCH_CHECK();
    }
    return SCP_OK;
}

// level_counts of the host: the counts as scanned, so that a leaf list that overflows a level shows there
inline hipError_t at_copy_counts(int64_t *level_counts, const uint8_t *ws, const at_layout &L, int D, hipStream_t st) {
    return hipMemcpyAsync(level_counts, (const int64_t *)(ws + L.b_counts) + AT_COUNT_ROW, (size_t)(D + 1) * 8, hipMemcpyDeviceToDevice, st);
}

bool at_ws_ok(const void *ws, int64_t bytes, int64_t need) { return ws && (((uintptr_t)ws) & 7) == 0 && bytes >= need; }

}  // namespace
