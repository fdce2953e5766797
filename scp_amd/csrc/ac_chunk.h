// One chunk of a chunked range-coder payload (include/scp.h, "Chunk-parallel range coder"): the coder step, the flush and the decoder step
// of rangecoder.cpp restated as plain C++ that compiles for the host alone (g++, tests/src/ac_chunk_host.cpp) and for a device lane
// (ac_chunks.hip: one lane per chunk).  rangecoder.cpp stays the definition; a chunk is by definition what scp_ac_encode_lohi returns on
// its pairs, and decodes to what scp_ac_dec_run_ctx returns on its bytes.
//
// What differs from rangecoder.cpp is the memory side only:
//   * the encoder collects bits in a 64-bit accumulator and stores whole 32-bit words (byte-swapped: the stream is MSB first) into a
//     4-byte-aligned private slot; every store is bounds-checked against the slot and an overflow is remembered, as BitSink does;
//   * pending (underflow) runs leave as words of 32 equal bits, never bit by bit;
//   * the decoder reads bytes below its chunk's length only, four at a time and one refill ahead; bits behind the end read as zero, as
//     in scp_ac_dec; its division is a float estimate with exact correction (acc_div).
//
// Slot size.  Before a step the state is normalised: the top bits of low and high differ and the pair is not (01.., 10..), so
// span = high - low + 1 > 2^30.  A pair of width 1 (the narrowest a valid table holds) leaves floor(span (c + 1) / 2^16) - floor(span c /
// 2^16) >= floor(span / 2^16) >= 2^14 of it.  Every shift of the renormalisation, emitted or pending, doubles the span, and the span
// never exceeds 2^32: a symbol moves at most 32 - 14 = 18 bits.  (18 is reached: a width-1 interval of exactly 2^14 aligned so that 17
// shifts end on low = 0x40000000, high = 0xBFFFFFFF takes one more underflow shift.)  The flush adds 2 bits, the last byte is padded:
// a chunk of N symbols needs at most ceil((18 N + 2) / 8) bytes, rounded up here to whole words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ACC_HD __host__ __device__ __forceinline__
#else
#define ACC_HD inline
#endif

#define ACC_MIN_CHUNK 64
#define ACC_MAX_CHUNK (1 << 20)

ACC_HD int64_t acc_slot_bytes(int64_t N) { return ((18 * N + 2 + 31) / 32) * 4; }

ACC_HD int acc_clz(uint32_t v) { return v ? __builtin_clz(v) : 32; }

struct acc_enc {
    uint32_t *out;          // the slot, 4-byte aligned
    uint32_t cap_words;
    uint32_t words;         // whole words produced so far (stored or not)
    uint64_t acc;           // bits collected MSB-first in the low `nbits` bits; nbits < 32 between calls
    int nbits;
    uint32_t low, high, pending;   // (pending <= 18 N < 2^25)
    bool overflow;
};

ACC_HD void acc_enc_init(acc_enc &e, uint32_t *slot, int64_t slot_bytes) {
    e.out = slot;
    e.cap_words = (uint32_t)(slot_bytes / 4);
    e.words = 0;
    e.acc = 0;
    e.nbits = 0;
    e.low = 0;
    e.high = 0xFFFFFFFFu;
    e.pending = 0;
    e.overflow = false;
}

ACC_HD void acc_enc_word(acc_enc &e, uint32_t w) {
    if (e.words < e.cap_words) e.out[e.words] = __builtin_bswap32(w); else e.overflow = true;
    ++e.words;
}

ACC_HD void acc_enc_drain(acc_enc &e) {     // nbits <= 63 on entry, < 32 on return
    if (e.nbits >= 32) {
        acc_enc_word(e, (uint32_t)(e.acc >> (e.nbits - 32)));
        e.nbits -= 32;
    }
}

ACC_HD void acc_enc_put_bits(acc_enc &e, uint32_t v, int k) {   // the low k (<= 31) bits of v, MSB first
    e.acc = (e.acc << k) | (uint64_t)v;
    e.nbits += k;
    acc_enc_drain(e);
}

ACC_HD void acc_enc_put_run(acc_enc &e, uint32_t bit, uint32_t count) {   // `count` copies of `bit`: one word per turn
    const uint64_t fill = bit ? ~0ull : 0ull;
    while (count) {
        const int k = count > 32u ? 32 : (int)count;
        e.acc = (e.acc << k) | (fill >> (64 - k));
        e.nbits += k;
        count -= (uint32_t)k;
        acc_enc_drain(e);
    }
}

ACC_HD void acc_enc_put_with_pending(acc_enc &e, uint32_t bit) {
    acc_enc_put_bits(e, bit, 1);
    if (e.pending) { acc_enc_put_run(e, bit ^ 1u, e.pending); e.pending = 0; }
}

// Coder::step.  c_high is 1 .. 65536 (a stored 0 is expanded by the caller).
ACC_HD void acc_enc_step(acc_enc &e, uint32_t c_low, uint32_t c_high) {
    uint32_t low = e.low, high = e.high;
    const uint64_t span = (uint64_t)high - (uint64_t)low + 1;
    high = (low - 1) + (uint32_t)((span * (uint64_t)c_high) >> 16);
    low = low + (uint32_t)((span * (uint64_t)c_low) >> 16);
    const uint32_t diff = low ^ high;
    if (!(diff & 0x80000000u)) {                         // (1) k shared leading bits (k <= 31 on valid pairs: low < high)
        const int k = diff ? __builtin_clz(diff) : 31;
        const uint32_t top = low >> (32 - k);
        acc_enc_put_with_pending(e, top >> (k - 1));
        if (k > 1) acc_enc_put_bits(e, top & ((1u << (k - 1)) - 1u), k - 1);
        low <<= k;
        high = (high << k) | ((1u << k) - 1u);
    }
    if (low >= 0x40000000u && high < 0xC0000000u) {      // (2) u underflow positions
        const int a = acc_clz(~(low << 1)), b = acc_clz(high << 1);
        int u = a < b ? a : b;
        if (u > 31) u = 31;
        e.pending += (uint32_t)u;
        low = (low << u) & 0x7FFFFFFFu;
        high = (high << u) | 0x80000000u | ((1u << u) - 1u);
    }
    e.low = low;
    e.high = high;
}

// Coder::flush + BitSink::finish -> the chunk's length in bytes (what a large enough slot would hold; e.overflow tells whether this one did)
ACC_HD uint32_t acc_enc_flush(acc_enc &e) {
    e.pending += 1;
    acc_enc_put_with_pending(e, e.low < 0x40000000u ? 0u : 1u);
    const uint32_t tail = (uint32_t)(e.nbits + 7) >> 3;  // 0 .. 4 bytes, the last one zero-padded
    const uint32_t len = e.words * 4u + tail;
    if (tail) acc_enc_word(e, (uint32_t)(e.acc << (32 - e.nbits)));
    return len;
}

struct acc_dec {
    const uint8_t *in;
    int64_t len, ptr;       // ptr: the first chunk byte behind `next`
    uint64_t win;           // the next `nwin` chunk bits, left-aligned (bit 63 first)
    int nwin;
    uint32_t next;          // the four bytes behind the window, MSB first, fetched one refill ahead of their use (a device lane never
                            // waits for memory inside a symbol); zeros behind the end of the chunk
    uint32_t low, high, value;
};

ACC_HD uint32_t acc_dec_load4(const acc_dec &d, int64_t p) {   // chunk bytes p .. p + 3, MSB first; no byte at or behind len is read
    if (p + 4 <= d.len) return ((uint32_t)d.in[p] << 24) | ((uint32_t)d.in[p + 1] << 16) | ((uint32_t)d.in[p + 2] << 8) | (uint32_t)d.in[p + 3];
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j) w = (w << 8) | (p + j < d.len ? (uint32_t)d.in[p + j] : 0u);
    return w;
}

// scp_ac_dec::refill keeps the window above 56 bits byte by byte; the bits a take() returns do not depend on when they were fetched, so
// this one adds 32 bits at a time (nwin <= 31 on entry: take() asks for at most 31 bits and refills only when short)
ACC_HD void acc_dec_refill(acc_dec &d) {
    d.win |= (uint64_t)d.next << (32 - d.nwin);
    d.nwin += 32;
    d.next = acc_dec_load4(d, d.ptr);
    d.ptr += 4;
}

ACC_HD uint32_t acc_dec_take(acc_dec &d, int k) {       // the next k (0 .. 31) bits, MSB first
    if (k <= 0) return 0;
    if (d.nwin < k) acc_dec_refill(d);
    const uint32_t v = (uint32_t)(d.win >> (64 - k));
    d.win <<= k;
    d.nwin -= k;
    return v;
}

ACC_HD void acc_dec_init(acc_dec &d, const uint8_t *bytes, int64_t len) {
    d.in = bytes;
    d.len = len > 0 ? len : 0;
    d.win = 0;
    d.nwin = 0;
    d.low = 0;
    d.high = 0xFFFFFFFFu;
    d.next = acc_dec_load4(d, 0);
    d.ptr = 4;
    const uint32_t hi = acc_dec_take(d, 16);
    d.value = (hi << 16) | acc_dec_take(d, 16);
}

// num / span, exact.  In the coder's regime - span > 2^24 (a normalised state has span > 2^30) and a quotient below 2^16 (value inside
// [low, high]) - a float estimate on the top 32 bits of num is off by a few units at most and two correction loops on the exact 64-bit
// remainder settle it, whatever the estimate was; anything else takes the 64-bit division.  (tests/src/ac_chunk_host.cpp holds it
// against the plain division on the edges of both conditions and on random operands.)
ACC_HD uint64_t acc_div(uint64_t num, uint64_t span) {
    if (span == 0) return 0;
    if (span <= (1ull << 24) || span > (1ull << 32) || (num >> 16) >= span) return num / span;
    const float est = (float)(uint32_t)(num >> 16) / (float)span * 65536.0f;
    int64_t q = est < 65535.0f ? (int64_t)est : 65535;
    int64_t r = (int64_t)num - q * (int64_t)span;
    while (r < 0) { --q; r += (int64_t)span; }
    while (r >= (int64_t)span) { ++q; r -= (int64_t)span; }
    return (uint64_t)q;
}

// ac_search_ref: largest s with row[s] <= count over [0, max_symbol], step for step
template <class Row>
ACC_HD int acc_search(Row row, uint16_t count, int max_symbol) {
    uint32_t left = 0, right = (uint32_t)max_symbol + 1;
    while (left + 1 < right) {
        const uint32_t mid = (left + right) / 2;
        const uint16_t v = row[mid];
        if (v < count) left = mid; else if (v > count) right = mid; else return (int)mid;
    }
    return (int)left;
}

// ac_dec_step<false>.  The division is exact (acc_div); a span of 0 - reachable only through tables with zero-width symbols, where the
// host divides by zero - gives count 0 here.
template <class Row>
ACC_HD int acc_dec_step(acc_dec &d, Row row, int max_symbol) {
    uint32_t low = d.low, high = d.high, value = d.value;
    const uint64_t span = (uint64_t)high - (uint64_t)low + 1;
    const uint64_t num = ((uint64_t)value - (uint64_t)low + 1) * 0x10000ull - 1;
    const uint16_t count = (uint16_t)acc_div(num, span);
    const int sy = acc_search(row, count, max_symbol);
    const uint32_t c_low = row[sy], c_high = sy == max_symbol ? 0x10000u : (uint32_t)row[sy + 1];
    high = (low - 1) + (uint32_t)((span * (uint64_t)c_high) >> 16);
    low = low + (uint32_t)((span * (uint64_t)c_low) >> 16);
    const uint32_t diff = low ^ high;
    if (!(diff & 0x80000000u)) {
        const int k = diff ? __builtin_clz(diff) : 31;
        low <<= k;
        high = (high << k) | ((1u << k) - 1u);
        value = (value << k) | acc_dec_take(d, k);
    }
    if (low >= 0x40000000u && high < 0xC0000000u) {
        const int a = acc_clz(~(low << 1)), b = acc_clz(high << 1);
        int u = a < b ? a : b;
        if (u > 31) u = 31;
        low = (low << u) & 0x7FFFFFFFu;
        high = (high << u) | 0x80000000u | ((1u << u) - 1u);
        value = ((value << u) ^ 0x80000000u) | acc_dec_take(d, u);
    }
    d.low = low; d.high = high; d.value = value;
    return sy;
}
