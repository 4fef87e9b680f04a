// filter_byte_rule_check.cpp -- a stand-alone host program around csrc/byte_rule.h and the format helpers and setters of
// csrc/container_internal.h as format version 16 (filter-auto with bytes; INTEGRATION.md 4b "Filter: auto with bytes") left them.
// It is meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/filter_byte_rule_check.cpp -o filter_byte_rule_check && ./filter_byte_rule_check [dump]
// Part 1, the rule: byte_mag() over every pair; byte_stride_word() and the lag clamp at their edges; the serial byte_sums() of a
// small buffer against a brute force in the other loop order, the 0xFFFFFFFF words and the winners with it; 1023 counted bytes
// give stride 0 and 1024 a candidate; byte_pick() over fifteen costs against a recursive restatement (a byte candidate needs the
// margin over a pick of one plane only), GRID_NO_COST never picked, the first thirteen grid_rule.h's walk.  With a dump from the model (tests/test_cpu_container_filter_byte.py writes it: the
// length, the bytes, the 16 lag sums, the 65537 stride sums, the two winners, the fifteen costs and the pick, little-endian) the
// serial sums, the winners and the walk are held against the model's.
// Part 2, the words: frame-word legality by brute force under versions 10, 13, 14 and 16 against the rule stated outright -- every
// low byte, the strides at their edges, every pattern of bits 25..30 -- and under every other version 0..18 only the word 0; a
// bit-31-clear word is legal under 16 exactly when it is under 14; the packing round trip for every lag and every stride; the
// stream header's triple through parse_frame_filter_format() over versions 0 to 18: parse_container_format()'s answer, or
// (16, 0, 0).
// Part 3, the setters: every state the setters reach from the default wants filter-byte on only with filter-grid on, format_of()
// version 16 exactly then and what it was with the setting off, reader() with the version-16 bit exactly then, a refused call
// changing nothing, set_filter_byte(1) accepted exactly with filter-grid on, and no other setter switching it on.  It prints
//   filter_byte_rule_check: ok, <legal> legal byte words, <packings> packings, <states> states, <calls> calls, dump <0 or 1>
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"
#include "../gpu-lossless-compression_amd/csrc/byte_rule.h"

#include <stdio.h>
#include <string.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    printf("filter_byte_rule_check: FAILED %s at (%llu, %llu, %llu)\n", what, a, b, c);
    return 1;
}

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint32_t loop_bitlen(uint32_t v)
{
    uint32_t n = 0;
    while (v) { n++; v >>= 1; }
    return n;
}

// the walk over the first n candidates, restated: a byte candidate (13, 14) needs no margin over a pick of elem 2, 4 or 8 (1 .. 12)
static uint32_t pick_upto(const unsigned long long *cost, uint32_t n)
{
    if (n == 1) return 0;
    const uint32_t p = pick_upto(cost, n - 1);
    if (n - 1 >= 13 && p >= 1 && p <= 12) return cost[n - 1] < cost[p] ? n - 1 : p;
    return 33 * cost[n - 1] < 32 * cost[p] ? n - 1 : p;
}

// the rule of a frame word under `version`, stated outright
static bool want_word(uint32_t version, uint32_t word)
{
    if (version != 10 && version != 13 && version != 14 && version != 16) return word == 0;
    if (word >> 31) {
        const uint32_t low = word & 0xFF, mid = (word >> 8) & 0x1FFFF;
        if (version == 16 && low == 1) return !((word >> 29) & 3) && (mid == 0 || (mid >= 2 && mid <= 65536));
        if (version != 14 && version != 16) return false;
        return !((word >> 25) & 31) && (low == 2 || low == 4 || low == 8) && mid >= 2 && mid <= 65536;
    }
    const uint32_t elem = word & 0xFFFF, flags = word >> 16;
    if (elem == 0) return flags == 0;
    if (elem != 2 && elem != 4 && elem != 8) return false;
    if (flags <= 1) return true;
    if (version == 10) return false;
    return (flags & 1) && !(flags & ~0x0F03u) && (flags & 0x0F02u);
}

static auto key(const CtSettings &s)
{
    return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.filter_lag, s.filter_grid, s.filter_byte, s.lag, s.fold,
                           s.grid_width, s.grid_fold, s.byte_lag, s.byte_stride);
}

static bool read_all(const char *path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    // ---- part 1: the rule
    for (uint32_t x = 0; x < 256; x++)
        for (uint32_t p = 0; p < 256; p++) {
            const int s = (int)(int8_t)(uint8_t)(x - p);           // the signed difference: m = |s| for s >= 0, -s - 1 below
            if (byte_mag(x, p) != (uint32_t)(s >= 0 ? s : -s - 1)) return fail("byte_mag", x, p, byte_mag(x, p));
            const uint32_t d = (x - p) & 255, f = ((d << 1) ^ (0u - (d >> 7))) & 255;
            if (grid_pair_bits(x, p, 1) != loop_bitlen(f)) return fail("grid_pair_bits at element size 1", x, p, 0);
        }
    for (uint32_t v : {0u, 1u, 2u, 16u, 17u, 18u, 65535u, 65536u, 65537u, 0x20000u, 0x80000011u, 0xFFFFFFFFu}) {
        if (byte_stride_word(v) != (v >= 17 && v <= 65536 ? v : 0u)) return fail("byte_stride_word", v, 0, 0);
        if (lag_clamp(v) < 1 || lag_clamp(v) > 16 || (v >= 1 && v <= 16 && lag_clamp(v) != v)) return fail("lag_clamp", v, 0, 0);
    }
    {
        // rows of 3 x 29 bytes, three interleaved ramps, every row the same but for noise: 2 * 2048 + 77 bytes and 5 that do not count
        std::vector<uint8_t> x(2 * 2048 + 77 + 5);
        for (size_t i = 0; i < x.size(); i++) x[i] = (uint8_t)((i % 87) / 3 * 2 + (i % 3) * 60 + rnd() % 3);
        std::vector<uint32_t> S(BYTE_SUM_ROW), B(BYTE_SUM_ROW, GRID_NO_SUM);
        unsigned long long A[BYTE_LAGS], C[BYTE_LAGS] = {};
        uint32_t win[2];
        byte_sums(x.data(), x.size(), A, S.data(), win);
        const size_t P = x.size() - x.size() % 8;
        for (size_t i = 0; i < P; i++)
            for (uint32_t l = 1; l <= BYTE_LAGS; l++) {
                const int s = (int)(int8_t)(uint8_t)(x[i] - (i % 2048 >= l ? x[i - l] : 0));
                C[l - 1] += (unsigned long long)(s >= 0 ? s : -s - 1);
            }
        for (uint32_t l = 0; l < BYTE_LAGS; l++)
            if (A[l] != C[l]) return fail("the lag sums", l + 1, A[l], C[l]);
        if (win[0] != 3) return fail("the lag of three interleaved ramps", win[0], 0, 0);
        const uint32_t wm = (uint32_t)(P / 2);
        for (uint32_t w = 17; w <= wm; w++) B[w] = 0;
        for (uint32_t t = 0; t < 32; t++) {
            const unsigned long long b = wm + (unsigned long long)t * (P - wm - 256) / 31;
            for (uint32_t j = 0; j < 256; j++)
                for (uint32_t w = 17; w <= wm; w++) {
                    const uint32_t d = (uint32_t)(x[b + j] - x[b + j - w]) & 255;
                    B[w] += loop_bitlen(((d << 1) ^ (0u - (d >> 7))) & 255);
                }
        }
        uint32_t best = 17;
        for (uint32_t w = 18; w <= wm; w++)
            if (B[w] < B[best]) best = w;
        for (size_t i = 0; i < BYTE_SUM_ROW; i++)
            if (S[i] != B[i]) return fail("the stride sums", i, S[i], B[i]);
        if (win[1] != best || best % 87) return fail("the stride winner", win[1], best, 0);
        if (S[16] != GRID_NO_SUM || S[17] == GRID_NO_SUM || S[wm] == GRID_NO_SUM || S[wm + 1] != GRID_NO_SUM) return fail("the ends of the row", 0, 0, 0);
        byte_sums(x.data(), 1023 + 8, A, S.data(), win);           // 1024 counted bytes: a candidate
        if (!win[1] || S[512] == GRID_NO_SUM || S[513] != GRID_NO_SUM) return fail("1024 bytes", win[1], 0, 0);
        byte_sums(x.data(), 1023, A, S.data(), win);               // 1016 counted bytes: none, but the lag sums stand
        if (win[1] || S[17] != GRID_NO_SUM || win[0] != 3) return fail("1023 bytes", win[0], win[1], 0);
        std::vector<uint8_t> z(4096, 0);
        byte_sums(z.data(), z.size(), A, S.data(), win);
        if (win[0] != 1 || win[1] != 17) return fail("zeros", win[0], win[1], 0);
        byte_sums(z.data(), 0, A, S.data(), win);
        if (win[0] != 1 || win[1] != 0) return fail("nothing", win[0], win[1], 0);
    }
    for (int i = 0; i < 300000; i++) {
        unsigned long long cost[BYTE_CANDS];
        const unsigned long long base = 1 + rnd() % (1ull << 42);
        for (uint32_t c = 0; c < BYTE_CANDS; c++) {
            const uint32_t how = (uint32_t)(rnd() % 5);
            cost[c] = how == 0 ? rnd() % (1ull << 43) : how == 1 ? base * 32 / 33 + rnd() % 5 - 2 : how == 2 ? base : how == 3 ? 0 : GRID_NO_COST;
            if (how < 3 && cost[c] > (1ull << 43)) cost[c] = 0;
        }
        if (cost[0] == GRID_NO_COST) cost[0] = base;              // (candidate 0 is the filter probe's: always a real cost)
        const uint32_t p = byte_pick(cost);
        if (p != pick_upto(cost, BYTE_CANDS)) return fail("byte_pick", p, pick_upto(cost, BYTE_CANDS), (unsigned long long)i);
        if (cost[p] == GRID_NO_COST) return fail("a candidate without a cost was picked", p, 0, (unsigned long long)i);
        if (pick_upto(cost, GRID_CANDS) != grid_pick(cost)) return fail("the first thirteen are grid_rule.h's walk", 0, 0, (unsigned long long)i);
    }
    int dumped = 0;
    if (argc > 1) {
        std::vector<uint8_t> d;
        if (!read_all(argv[1], d) || d.size() < 8) return fail("the dump cannot be read", 0, 0, 0);
        unsigned long long len;
        memcpy(&len, d.data(), 8);
        const size_t want = 8 + len + 8 * BYTE_LAGS + 4 * BYTE_SUM_ROW + 8 + 8 * BYTE_CANDS + 4;
        if (d.size() != want) return fail("the dump's size", d.size(), want, len);
        const uint8_t *x = d.data() + 8, *q = x + len;
        std::vector<uint32_t> S(BYTE_SUM_ROW), MS(BYTE_SUM_ROW);
        unsigned long long A[BYTE_LAGS], MA[BYTE_LAGS], cost[BYTE_CANDS];
        uint32_t win[2], mwin[2], mpick;
        memcpy(MA, q, sizeof MA); q += sizeof MA;
        memcpy(MS.data(), q, 4 * BYTE_SUM_ROW); q += 4 * BYTE_SUM_ROW;
        memcpy(mwin, q, 8); q += 8;
        memcpy(cost, q, sizeof cost); q += sizeof cost;
        memcpy(&mpick, q, 4);
        byte_sums(x, len, A, S.data(), win);
        for (uint32_t l = 0; l < BYTE_LAGS; l++)
            if (A[l] != MA[l]) return fail("the model's lag sums", l + 1, A[l], MA[l]);
        for (size_t i = 0; i < BYTE_SUM_ROW; i++)
            if (S[i] != MS[i]) return fail("the model's stride sums", i, S[i], MS[i]);
        if (win[0] != mwin[0] || win[1] != mwin[1]) return fail("the model's winners", win[0], win[1], mwin[1]);
        if (byte_pick(cost) != mpick) return fail("the model's pick", byte_pick(cost), mpick, 0);
        dumped = 1;
    }

    // ---- part 2: the words
    const uint32_t mids[] = {0, 1, 2, 3, 16, 17, 640, 1281, 65535, 65536, 65537, 0x10001, 0x1FFFF};
    unsigned legal = 0;
    for (uint32_t version = 0; version <= 18; version++) {
        CtFormat st;
        st.version = version;
        for (uint32_t low = 0; low < 256; low++)
            for (uint32_t mid : mids)
                for (uint32_t top = 0; top < 64; top++) {         // bits 25 .. 30
                    const uint32_t word = low | mid << 8 | top << 25 | 1u << 31;
                    const bool want = want_word(version, word);
                    if (ct_frame_word_legal(st, word) != want) return fail("ct_frame_word_legal of a bit-31 word", version, word, want);
                    if (!want || low != 1) continue;
                    legal++;
                    const CtFormat f = ct_frame_format(st, word);
                    if (!f.bytes() || f.grid() || f.elem != 1 || f.width != mid || f.lag() != (top & 15) + 1 || f.fold() || !f.delta() || !f.filtered() ||
                        f.flags != (1u | (mid ? 4u : 0u) | (top & 15) << 8)) return fail("ct_frame_format of a byte word", version, word, 0);
                    if (ct_frame_word(f) != word) return fail("ct_frame_word of a byte frame's format", version, word, 0);
                }
        for (uint32_t flags = 0; flags < 32768; flags += (version == 16 || version == 14 ? 1 : 3))
            for (uint32_t elem = 0; elem <= 17; elem++) {
                const uint32_t word = elem | flags << 16;
                if (ct_frame_word_legal(st, word) != want_word(version, word)) return fail("ct_frame_word_legal of a bit-31-clear word", version, word, 0);
            }
    }
    if (legal != 9 * 16) return fail("the count of legal byte words among those tried", legal, 0, 0);
    CtFormat s16, s14;
    s16.version = CT_VERSION_FILTER_BYTE;
    s14.version = CT_VERSION_FILTER_GRID;
    for (uint32_t flags = 0; flags < 32768; flags++)
        for (uint32_t elem = 0; elem <= 17; elem++) {
            const uint32_t word = elem | flags << 16;
            if (ct_frame_word_legal(s16, word) != ct_frame_word_legal(s14, word)) return fail("a bit-31-clear word under 16 and 14", flags, elem, 0);
            if (!ct_frame_word_legal(s16, word)) continue;
            const CtFormat a = ct_frame_format(s16, word), b = ct_frame_format(s14, word);
            if (a.bytes() || a.grid() || a.width || a.elem != b.elem || a.flags != b.flags || a.lag() != b.lag() || a.fold() != b.fold()) return fail("its format", flags, elem, 0);
        }
    for (uint32_t e = 2; e <= 8; e *= 2)
        for (uint32_t w : {2u, 640u, 65536u})
            for (uint32_t fold = 0; fold < 2; fold++) {
                const uint32_t word = e | w << 8 | fold << 30 | 1u << 31;
                const CtFormat a = ct_frame_format(s16, word), b = ct_frame_format(s14, word);
                if (!a.grid() || a.bytes() || a.elem != b.elem || a.width != b.width || a.flags != b.flags || a.fold() != fold || ct_frame_word(a) != word)
                    return fail("a grid word under version 16", word, 0, 0);
            }
    unsigned long long packings = 0;
    for (uint32_t lag = 1; lag <= 16; lag++)
        for (uint32_t stride = 0; stride <= 65536; stride++) {
            if (stride == 1) continue;
            const uint32_t lags[LAG_ELEMS] = {1, 1, 1}, widths[LAG_ELEMS] = {0, 0, 0};
            const GridCand c = byte_cand(stride ? GRID_CANDS + 1 : GRID_CANDS, lags, widths, lag, stride);
            CtFormat ff = s16;                                    // as Encoder::frame() makes it
            ff.elem = c.elem;
            ff.flags = CT_FLAG_DELTA | (c.fold ? CT_FLAG_FOLD : 0u) | (c.lag - 1u) << CT_LAG_SHIFT | (c.width ? CT_FLAG_GRID : 0u);
            ff.width = c.width;
            const uint32_t word = ct_frame_word(ff);
            if (word != (1u | stride << 8 | (lag - 1) << 25 | 1u << 31)) return fail("the packing", lag, stride, word);
            if (!ct_frame_word_legal(s16, word) || ct_frame_word_legal(s14, word)) return fail("the packed word's legality", lag, stride, word);
            const CtFormat back = ct_frame_format(s16, word);
            if (!back.bytes() || back.lag() != lag || back.width != stride || back.elem != 1 || back.flags != ff.flags) return fail("the way back", lag, stride, word);
            packings++;
        }
    for (uint32_t v = 0; v <= 18; v++)
        for (uint32_t f = 0; f < 65536; f += (v >= 15 ? 1 : 257))
            for (uint32_t w3 : {0u, 1u, 2u, 4u, 8u, 9u, 1u | 2u << 8, 1u | 1281u << 8, 2u | 640u << 8, 1u << 31 | 1u}) {
                const uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, w3, 0, 0, 0, 0};
                CtFormat a, b;
                const bool pa = parse_container_format(h, &a), pb = parse_frame_filter_format(h, &b);
                if (pb != (pa || (v == 16 && f == 0 && w3 == 0)) || (v >= 16 && pa)) return fail("parse_frame_filter_format", v, f, w3);
                if (pb && pa && (a.version != b.version || a.flags != b.flags || a.elem != b.elem || a.width != b.width)) return fail("another version's format changed", v, f, w3);
                if (pb && v == 16 && (b.reads() != CT_READS_FILTER_BYTE || b.kinds() != ct_kinds(8) || b.filtered() || b.grid() || b.bytes() || b.lag() != 1 || b.fold() ||
                                      !b.frame_filters())) return fail("version 16's format", v, f, w3);
            }
    if (ct_kinds(16) != 0) return fail("ct_kinds' table", ct_kinds(16), 0, 0);

    // ---- part 3: the setters
    const uint32_t lagv[3][2] = {{1, 0}, {3, 1}, {0, 0}};
    const uint32_t grids[3][2] = {{0, 0}, {1024, 1}, {1, 0}};
    const uint32_t bytes[4][2] = {{0, 0}, {3, 1281}, {17, 0}, {1, 0}};
    std::set<decltype(key(CtSettings()))> seen;
    std::vector<CtSettings> todo{CtSettings()};
    seen.insert(key(todo[0]));
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const CtSettings s = todo.back();
        todo.pop_back();
        if (s.filter_byte && !s.filter_grid) return fail("filter-byte is on without filter-grid", s.codec, s.mode, s.shuffle);
        if (s.filter_grid && !s.filter_lag) return fail("filter-grid is on without filter-lag", s.codec, s.mode, s.shuffle);
        if (s.filter_lag && !s.filter_auto) return fail("filter-lag is on without filter-auto", s.codec, s.mode, s.shuffle);
        if (s.filter_byte && s.byte_on()) return fail("filter-byte and byte-delta are both on", s.byte_lag, 0, 0);
        const CtFormat f = format_of(s);
        if ((f.version == CT_VERSION_FILTER_BYTE) != s.filter_byte) return fail("format_of's version", f.version, f.flags, f.elem);
        if (s.filter_byte && (f.flags || f.elem || f.width)) return fail("version 16's triple", f.version, f.flags, f.elem);
        if (((s.reader() & CT_READS_FILTER_BYTE) != 0) != s.filter_byte) return fail("reader", s.reader(), 0, 0);
        if (s.filter_byte && (!(s.reader() & CT_READS_FILTER_GRID) || !(s.reader() & CT_READS_FILTER_LAG) || !(s.reader() & CT_READS_FILTER) || (s.reader() & CT_READS_BYTE)))
            return fail("a filter-byte plan reads versions 14, 13 and 10 and not 15", s.reader(), 0, 0);
        CtSettings off = s;
        off.filter_byte = false;
        const CtFormat g = format_of(off);
        if (g.version == CT_VERSION_FILTER_BYTE || (s.filter_byte && g.version != CT_VERSION_FILTER_GRID)) return fail("format_of with the setting off", g.version, g.flags, g.elem);
        if (!s.filter_byte && (g.version != f.version || g.flags != f.flags || g.elem != f.elem || g.width != f.width)) return fail("format_of changed", g.version, g.flags, g.elem);
        for (int k = 0; k < 15; k++) {
            const uint32_t vals[8] = {0, 1, 2, 3, 4, 8, 9, 1u << 31};
            for (int i = 0; i < (k == 9 || k == 10 ? 3 : k == 13 ? 4 : 8); i++) {
                CtSettings t = s;
                bool ok;
                switch (k) {
                case 0: ok = t.set_shuffle(vals[i]); break;
                case 1: ok = t.set_delta(vals[i]); break;
                case 2: ok = t.set_codec(vals[i]); break;
                case 3: ok = t.set_mode(CT_MODE_SPARSE, vals[i]); break;
                case 4: ok = t.set_mode(CT_MODE_RUNS, vals[i]); break;
                case 5: ok = t.set_mode(CT_MODE_ANS, vals[i]); break;
                case 6: ok = t.set_mode(CT_MODE_AUTO, vals[i]); break;
                case 7: ok = t.set_mode(CT_MODE_DEDUP, vals[i]); break;
                case 8: ok = t.set_filter_auto(vals[i]); break;
                case 9: ok = t.set_delta_lag(lagv[i][0], lagv[i][1]); break;
                case 10: ok = t.set_delta_grid(grids[i][0], grids[i][1]); break;
                case 11: ok = t.set_filter_lag(vals[i]); break;
                case 12: ok = t.set_filter_grid(vals[i]); break;
                case 13: ok = t.set_byte_delta(bytes[i][0], bytes[i][1]); break;
                default: ok = t.set_filter_byte(vals[i]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (unsigned long long)k, (unsigned long long)i, 0);
                if (k == 14) {
                    if (ok != (vals[i] == 0 || (vals[i] == 1 && s.filter_grid))) return fail("set_filter_byte's answer", vals[i], s.filter_grid, 0);
                    if (ok && t.filter_byte != (vals[i] == 1)) return fail("set_filter_byte's effect", vals[i], 0, 0);
                    CtSettings u = t;
                    u.filter_byte = s.filter_byte;
                    if (key(u) != key(s)) return fail("set_filter_byte changed another setting", vals[i], 0, 0);
                } else if (ok && s.filter_byte && t.filter_grid && !t.filter_byte) {
                    return fail("a call that leaves filter-grid on switched filter-byte off", (unsigned long long)k, vals[i], 0);
                } else if (ok && !s.filter_byte && t.filter_byte) {
                    return fail("another setter switched filter-byte on", (unsigned long long)k, vals[i], 0);
                }
                if (k == 13 && s.filter_byte && bytes[i][0] && ok) return fail("byte-delta was accepted while filter-byte is on", bytes[i][0], 0, 0);
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }
    printf("filter_byte_rule_check: ok, %u legal byte words, %llu packings, %zu states, %llu calls, dump %d\n", legal, packings, seen.size(), calls, dumped);
    return 0;
}
