// csrc/ac_chunk.h (the coder and decoder step every device lane runs) compiled for the host and held against rangecoder.cpp, chunk by
// chunk: the encoder's bytes equal scp_ac_encode_lohi's on the slice, the decoder's symbols equal scp_ac_dec_run_ctx's on the chunk's
// bytes (whole, and cut by 1 .. 4 bytes) - on table-coded chunks and on the adversarial pair sets' chunks alike.  Every buffer has its exact size on the heap, so under -fsanitize=address a read or write past
// a slot or a chunk is caught.
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "scp.h"
#include "ac_chunk.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }

// ntab monotone rows of Lp entries: alphabet = Lp - 1 symbols of width >= 1, widths summing to 65536 (the last entry wraps to 0)
static std::vector<uint16_t> make_tables(int ntab, int Lp) {
    const int A = Lp - 1;
    std::vector<uint16_t> t((size_t)ntab * Lp);
    for (int g = 0; g < ntab; ++g) {
        std::vector<uint32_t> w(A, 1);
        uint32_t left = 65536 - A;
        const int mode = g % 4;
        while (left) {
            const int k = mode == 0 ? rnd() % A : (mode == 1 ? rnd() % 4 : (mode == 2 ? (int)(rnd() % 8) * (A / 8) : A - 1 - rnd() % 3));
            uint32_t a = 1 + rnd() % (left < 6000 ? left : 6000);
            if (a > left) a = left;
            w[k] += a;
            left -= a;
        }
        uint32_t c = 0;
        for (int j = 0; j < A; ++j) { t[(size_t)g * Lp + j] = (uint16_t)c; c += w[j]; }
        t[(size_t)g * Lp + A] = (uint16_t)c;
    }
    return t;
}

static int fail(const char *what, int a, int b) { printf("FAIL %s (%d, %d)\n", what, a, b); return 1; }

// the header's encoder on every chunk of `lohi` against scp_ac_encode_lohi on the slice; the chunks are appended to `chunks`
static int check_encode(const std::vector<uint32_t> &lohi, int N, std::vector<std::vector<uint8_t>> *chunks, int id) {
    const int64_t n = (int64_t)lohi.size(), slot = acc_slot_bytes(N);
    for (int64_t b = 0; b < n; b += N) {
        const int64_t m = n - b < N ? n - b : N;
        std::vector<uint32_t> exact(lohi.begin() + b, lohi.begin() + b + m);
        std::vector<uint8_t> want((size_t)m * 4 + 64);
        size_t wl = 0;
        if (scp_ac_encode_lohi(exact.data(), m, want.data(), want.size(), &wl)) return fail("host encode", id, (int)b);
        std::vector<uint32_t> buf((size_t)slot / 4);
        acc_enc e;
        acc_enc_init(e, buf.data(), slot);
        for (int64_t i = 0; i < m; ++i) { const uint32_t hi = exact[i] >> 16; acc_enc_step(e, exact[i] & 0xFFFFu, hi ? hi : 0x10000u); }
        const uint32_t len = acc_enc_flush(e);
        if (e.overflow) return fail("slot overflow", id, (int)b);
        if (len != wl || memcmp(buf.data(), want.data(), wl)) return fail("encoder bytes", id, (int)b);
        // a slot one word short of what the chunk needs reports the overflow and writes nothing behind it
        if (len > 4) {
            std::vector<uint32_t> small((len - 1) / 4);
            acc_enc s;
            acc_enc_init(s, small.data(), (int64_t)small.size() * 4);
            for (int64_t i = 0; i < m; ++i) { const uint32_t hi = exact[i] >> 16; acc_enc_step(s, exact[i] & 0xFFFFu, hi ? hi : 0x10000u); }
            if (acc_enc_flush(s) != len || !s.overflow) return fail("short slot", id, (int)b);
        }
        if (chunks) chunks->push_back(std::vector<uint8_t>(want.begin(), want.begin() + wl));
    }
    return 0;
}

static int check_decode(const std::vector<uint8_t> &chunk, const std::vector<uint16_t> &tabs, int ntab, int Lp, const std::vector<uint8_t> &table_of,
                        const uint8_t *ctx, int64_t m, const int16_t *src, int id) {
    std::vector<uint16_t> rows((size_t)table_of.size() * Lp);              // the host decoder indexes by context: expand the map
    for (size_t c = 0; c < table_of.size(); ++c) memcpy(&rows[c * Lp], &tabs[(size_t)table_of[c] * Lp], (size_t)Lp * 2);
    for (int cut = 0; cut <= 4; ++cut) {
        if ((size_t)cut > chunk.size()) break;
        std::vector<uint8_t> bytes(chunk.begin(), chunk.end() - cut);       // exact size
        std::vector<uint8_t> cx(ctx, ctx + m);
        std::vector<int16_t> want(m), got(m);
        scp_ac_dec *d = nullptr;
        if (scp_ac_dec_new(&d, bytes.data(), bytes.size(), Lp)) return fail("dec_new", id, cut);
        if (scp_ac_dec_run_ctx(d, rows.data(), (int32_t)table_of.size(), cx.data(), m, want.data())) return fail("run_ctx", id, cut);
        scp_ac_dec_free(d);
        acc_dec a;
        acc_dec_init(a, bytes.data(), (int64_t)bytes.size());
        for (int64_t i = 0; i < m; ++i) got[i] = (int16_t)acc_dec_step(a, (const uint16_t *)&tabs[(size_t)table_of[cx[i]] * Lp], Lp - 2);
        if (memcmp(want.data(), got.data(), (size_t)m * 2)) return fail("decoder symbols", id, cut);
        if (cut == 0 && src && memcmp(got.data(), src, (size_t)m * 2)) return fail("round trip", id, 0);
    }
    return 0;
}

// acc_div against the plain 64-bit division: the edges of its fast path (span around 2^24, 2^30 and 2^32, quotients around 0 and 2^16,
// remainders 0 and span - 1) and random operands of the coder's regime and outside it
static int check_div() {
    const uint64_t spans[] = {0, 1, 2, 65535, (1ull << 24) - 1, 1ull << 24, (1ull << 24) + 1, (1ull << 30) - 1, 1ull << 30, (1ull << 30) + 1, 0x7FFFFFFFull,
                              0x80000000ull, 0x80000001ull, 0xFFFFFFFEull, 0xFFFFFFFFull, 1ull << 32, (1ull << 32) + 1, 3000000019ull, 1073741827ull};
    for (uint64_t span : spans) {
        for (uint64_t q = 0; q <= 65537; q += (q < 4 || q > 65530 ? 1 : 257)) {
            for (int e = -2; e <= 2; ++e) {
                const uint64_t rems[] = {0, 1, span / 2, span - 1};
                for (uint64_t rem : rems) {
                    const uint64_t num = q * span + (span ? rem % span : 0) + (uint64_t)(int64_t)e * (span ? span : 1);
                    if (acc_div(num, span) != (span ? num / span : 0)) { printf("FAIL acc_div(%llu, %llu)\n", (unsigned long long)num, (unsigned long long)span); return 1; }
                }
            }
        }
    }
    for (int t = 0; t < 4000000; ++t) {
        uint64_t span = ((uint64_t)rnd() << 16 | (rnd() & 0xFFFF));
        if (t & 1) span = (1ull << 30) + 1 + span % ((3ull << 30));                      // the normalised states: 2^30 < span <= 2^32
        else span >>= rnd() % 33;
        uint64_t num = (((uint64_t)rnd() << 32) | ((uint64_t)rnd() << 16) | (rnd() & 0xFFFF)) >> (t % 5 == 0 ? rnd() % 40 : 0);
        if (t & 2) num %= (span ? span : 1) << 16;                                        // a value inside [low, high]
        if (acc_div(num, span) != (span ? num / span : 0)) { printf("FAIL acc_div(%llu, %llu)\n", (unsigned long long)num, (unsigned long long)span); return 1; }
    }
    return 0;
}

int main() {
    const int chunk_sizes[3] = {64, 100, 256};
    int id = 0;
    if (check_div()) return 1;
    // 200 random cases: both alphabets, 16 tables behind a context map (ntab < nctx), n a multiple of N and not
    for (int trial = 0; trial < 200; ++trial, ++id) {
        const int Lp = trial & 1 ? 1022 : 512, ntab = 16, nctx = 40, N = chunk_sizes[trial % 3];
        const std::vector<uint16_t> tabs = make_tables(ntab, Lp);
        std::vector<uint8_t> table_of(nctx);
        for (auto &t : table_of) t = (uint8_t)(rnd() % ntab);
        const int64_t n = trial % 5 == 0 ? (int64_t)N * (1 + rnd() % 4) : 1 + rnd() % 1500;
        std::vector<uint8_t> ctx(n);
        std::vector<int16_t> sym(n);
        std::vector<uint32_t> lohi(n);
        for (int64_t i = 0; i < n; ++i) {
            ctx[i] = (uint8_t)(rnd() % nctx);
            const uint16_t *row = &tabs[(size_t)table_of[ctx[i]] * Lp];
            const int mode = rnd() % 3;
            int s = mode == 0 ? rnd() % (Lp - 1) : (mode == 1 ? rnd() % 4 : Lp - 2 - rnd() % 3);
            sym[i] = (int16_t)s;
            lohi[i] = (uint32_t)row[s] | ((uint32_t)row[s + 1] << 16);     // (row[Lp - 1] holds 65536 as 0)
        }
        std::vector<std::vector<uint8_t>> chunks;
        if (check_encode(lohi, N, &chunks, id)) return 1;
        for (size_t c = 0; c < chunks.size(); ++c) {
            const int64_t b = (int64_t)c * N, m = n - b < N ? n - b : N;
            if (check_decode(chunks[c], tabs, ntab, Lp, table_of, ctx.data() + b, m, sym.data() + b, id)) return 1;
        }
    }
    // adversarial pair sets (encoder): width 1 only, midpoint straddles whole and broken, full width only, all interleaved
    const std::vector<uint16_t> adv_tabs_511 = make_tables(16, 512), adv_tabs_1021 = make_tables(16, 1022);
    for (int set = 0; set < 6; ++set) {
        for (int rep = 0; rep < 8; ++rep, ++id) {
            const int N = chunk_sizes[rep % 3];
            const int64_t n = rep < 3 ? 4 * N : 1 + rnd() % 3000;
            std::vector<uint32_t> lohi(n);
            for (int64_t i = 0; i < n; ++i) {
                const int kind = set < 4 ? set : (set == 4 ? (int)(rnd() % 4) : (int)((i / 37) % 4));
                uint32_t lo, hi;
                if (kind == 0) { lo = rnd() % 65536; hi = lo + 1; }                                   // width 1 anywhere
                else if (kind == 1) { lo = 0x7FFF; hi = 0x8001; }                                     // straddles the midpoint
                else if (kind == 2) { if (rnd() % 257 == 0) { lo = 0x7FF0 + rnd() % 8; hi = lo + 1 + rnd() % 8; } else { lo = 0x7FFF; hi = 0x8001; } }
                else { lo = 0; hi = 65536; }                                                          // the whole range
                lohi[i] = lo | ((hi & 0xFFFFu) << 16);
            }
            std::vector<std::vector<uint8_t>> chunks;
            if (check_encode(lohi, N, &chunks, id)) return 1;
            // these chunks are not coded under any table; as bytes they still decode, and the header's decoder must return what
            // scp_ac_dec_run_ctx returns on them, whole and cut, under the random tables of both alphabets
            const int Lp = rep & 1 ? 1022 : 512, nctx = 40;
            const std::vector<uint16_t> &tabs = Lp == 512 ? adv_tabs_511 : adv_tabs_1021;
            std::vector<uint8_t> table_of(nctx), ctx(n);
            for (auto &t : table_of) t = (uint8_t)(rnd() % 16);
            for (auto &c : ctx) c = (uint8_t)(rnd() % nctx);
            for (size_t c = 0; c < chunks.size(); ++c) {
                const int64_t b = (int64_t)c * N, m = n - b < N ? n - b : N;
                if (check_decode(chunks[c], tabs, 16, Lp, table_of, ctx.data() + b, m, nullptr, id)) return 1;
            }
        }
    }
    // a table of width-1 symbols (all but one) through the decoder: the largest expansion, decoded back
    for (int rep = 0; rep < 6; ++rep, ++id) {
        const int Lp = rep & 1 ? 1022 : 512, A = Lp - 1, N = chunk_sizes[rep % 3];
        std::vector<uint16_t> tab(Lp);
        for (int j = 0; j < A; ++j) tab[j] = (uint16_t)j;                  // symbol A - 1 takes the rest
        tab[A] = 0;
        const int64_t n = 3 * N + 17;
        std::vector<uint8_t> ctx(n, 0), table_of(1, 0);
        std::vector<int16_t> sym(n);
        std::vector<uint32_t> lohi(n);
        for (int64_t i = 0; i < n; ++i) {
            const int s = rnd() % (A - 1);
            sym[i] = (int16_t)s;
            lohi[i] = (uint32_t)tab[s] | ((uint32_t)tab[s + 1] << 16);
        }
        std::vector<std::vector<uint8_t>> chunks;
        if (check_encode(lohi, N, &chunks, id)) return 1;
        for (size_t c = 0; c < chunks.size(); ++c) {
            const int64_t b = (int64_t)c * N, m = n - b < N ? n - b : N;
            if (check_decode(chunks[c], tab, 1, Lp, table_of, ctx.data() + b, m, sym.data() + b, id)) return 1;
        }
    }
    printf("%d chunk cases ok\n", id);
    return 0;
}
