// filter_grid_rule_check.cpp -- a stand-alone host program around csrc/grid_rule.h and the format helpers and setters of
// csrc/container_internal.h as format version 14 (filter-auto with grid; INTEGRATION.md 4b "Filter: auto with grid") left them.  It
// is meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/filter_grid_rule_check.cpp -o filter_grid_rule_check && ./filter_grid_rule_check
// Part 1, the rule: grid_pair_bits() against the zigzag of the signed difference and a loop; grid_wmax() and grid_tile_start() at
// their edges (every target and its element Wmax back lie inside the segment); the serial grid_sums() of a small buffer against a
// brute force that walks targets first and widths second, the 0xFFFFFFFF words and the winners with it; 1023 elements give width
// 0 and 1024 a candidate; grid_argmin() with ties; grid_pick() over thirteen costs against a recursive restatement, GRID_NO_COST
// never picked; grid_width_word() at its edges.
// Part 2, the words: every word the writer can make (lag_rule.h's and elem 2, 4, 8 x every width with the fold) is legal under
// version 14 and parses back; a bit-31 word is legal exactly by the rule stated outright, over every elem byte, the widths at the
// edges and every pattern of bits 25..30, and under no other version; a bit-31-clear word is legal under 14 exactly when it is
// under 13; the stream header's triple: (14, 0, 0) alone, through parse_header_format() only.
// Part 3, the setters: every state the setters reach from the default wants filter-grid on only with filter-lag on (and that only
// with filter-auto), format_of() version 14 exactly then and what it was with the setting off, reader() with the version-14 bit
// exactly then, a refused call changing nothing, and set_filter_grid(1) accepted exactly with filter-lag on.  It prints
//   filter_grid_rule_check: ok, <words> writer words, <legal> legal grid words, <states> states, <calls> calls
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"
#include "../gpu-lossless-compression_amd/csrc/grid_rule.h"

#include <stdio.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    printf("filter_grid_rule_check: FAILED %s at (%llu, %llu, %llu)\n", what, a, b, c);
    return 1;
}

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint32_t loop_bitlen(unsigned long long v)
{
    uint32_t n = 0;
    while (v) { n++; v >>= 1; }
    return n;
}

// bitlen(fold(x - p)) from the signed difference: the zigzag is 2 s for s >= 0 and -2 s - 1 for s < 0, modulo 2^(8 e)
static uint32_t want_bits(unsigned long long x, unsigned long long p, uint32_t e)
{
    const unsigned long long m = e == 8 ? ~0ull : (1ull << (8 * e)) - 1, d = (x - p) & m;
    const unsigned long long f = ((d >> (8 * e - 1)) & 1) ? ((~d & m) * 2 + 1) & m : (d * 2) & m;
    return loop_bitlen(f);
}

static uint32_t pick_upto(const unsigned long long *cost, uint32_t n)      // the walk over the first n candidates, restated
{
    if (n == 1) return 0;
    const uint32_t p = pick_upto(cost, n - 1);
    return 33 * cost[n - 1] < 32 * cost[p] ? n - 1 : p;
}

// the rule of a bit-31 word, stated outright
static bool want_grid_word(uint32_t version, uint32_t word)
{
    if (version != 14) return false;
    const uint32_t elem = word & 0xFF, width = (word >> 8) & 0x1FFFF;
    if ((word >> 25) & 31) return false;
    return (elem == 2 || elem == 4 || elem == 8) && width >= 2 && width <= 65536;
}

static auto key(const CtSettings &s)
{
    return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.filter_lag, s.filter_grid, s.lag, s.fold, s.grid_width,
                           s.grid_fold);
}

int main()
{
    // ---- part 1: the rule
    for (uint32_t e = 2; e <= 8; e *= 2) {
        const unsigned long long mask = e == 8 ? ~0ull : (1ull << (8 * e)) - 1;
        for (int i = 0; i < 100000; i++) {
            const unsigned long long x = rnd() & mask, p = i < 64 ? (x - (unsigned long long)(i - 32)) & mask : (i & 1) ? rnd() & mask : (x + (rnd() >> (rnd() & 63))) & mask;
            if (grid_pair_bits(x, p, e) != want_bits(x, p, e)) return fail("grid_pair_bits", x, p, e);
        }
        if (grid_pair_bits(5, 5, e) != 0 || grid_pair_bits(0, 1, e) != 1 || grid_pair_bits(0, mask / 2 + 1, e) != 8 * e) return fail("grid_pair_bits at the ends", e, 0, 0);
    }
    for (unsigned long long N : {1024ull, 1025ull, 2047ull, 4096ull, 131071ull, 131072ull, 131073ull, 1ull << 20, (1ull << 30) - 1, 1ull << 30}) {
        const uint32_t wm = grid_wmax(N);
        if (wm != (N / 2 < 65536 ? N / 2 : 65536) || wm < GRID_W_MIN) return fail("grid_wmax", N, wm, 0);
        unsigned long long last = 0;
        for (uint32_t t = 0; t < GRID_TILES; t++) {
            const unsigned long long b = grid_tile_start(N, wm, t);
            if (b < wm || b + GRID_TILE > N || b < last) return fail("grid_tile_start", N, t, b);
            last = b;
        }
        if (grid_tile_start(N, wm, 0) != wm || grid_tile_start(N, wm, GRID_TILES - 1) != N - GRID_TILE) return fail("the first and the last tile", N, 0, 0);
    }
    {
        // rows of 37 elements of 2 bytes, a ramp down the rows with noise, 2063 elements and 5 bytes: the serial sums against a brute
        // force in the other loop order, for every element size
        std::vector<uint8_t> x(2 * 2063 + 5);
        for (size_t i = 0; i < x.size() / 2; i++) {
            const uint32_t v = (uint32_t)(i / 37 * 7 + (i % 37) * 300 + rnd() % 3);
            x[2 * i] = (uint8_t)v; x[2 * i + 1] = (uint8_t)(v >> 8);
        }
        std::vector<uint32_t> S(GRID_SUMS), B(GRID_SUMS, GRID_NO_SUM);
        uint32_t widths[LAG_ELEMS];
        grid_sums(x.data(), x.size(), S.data(), widths);
        const size_t P = x.size() - x.size() % 8;
        for (uint32_t k = 0; k < LAG_ELEMS; k++) {
            const uint32_t e = 2u << k;
            const unsigned long long N = P / e;
            if (N < GRID_MIN_ELEMS) {
                if (widths[k] != 0) return fail("a width without a candidate", e, widths[k], 0);
                continue;
            }
            auto at = [&](unsigned long long i) { unsigned long long v = 0; for (uint32_t b = 0; b < e; b++) v |= (unsigned long long)x[i * e + b] << (8 * b); return v; };
            const uint32_t wm = (uint32_t)(N / 2);
            uint32_t *row = B.data() + (size_t)k * GRID_SUM_ROW;
            for (uint32_t w = 2; w <= wm; w++) row[w] = 0;
            for (uint32_t t = 0; t < 32; t++) {
                const unsigned long long b = wm + (unsigned long long)t * (N - wm - 256) / 31;
                for (uint32_t j = 0; j < 256; j++)
                    for (uint32_t w = 2; w <= wm; w++) row[w] += want_bits(at(b + j), at(b + j - w), e);
            }
            uint32_t best = 2;
            for (uint32_t w = 3; w <= wm; w++)
                if (row[w] < row[best]) best = w;
            if (widths[k] != best) return fail("the winner", e, widths[k], best);
        }
        for (size_t i = 0; i < GRID_SUMS; i++)
            if (S[i] != B[i]) return fail("grid_sums", i / GRID_SUM_ROW, i % GRID_SUM_ROW, S[i]);
        if (widths[0] != 37 || widths[1] == 0 || widths[2] != 0) return fail("the winners of rows of 37", widths[0], widths[1], widths[2]);
        if (S[0] != GRID_NO_SUM || S[1] != GRID_NO_SUM || S[2] == GRID_NO_SUM || S[1032] == GRID_NO_SUM || S[1033] != GRID_NO_SUM) return fail("the ends of a row", 0, 0, 0);
        // 1023 elements of 2 bytes: no candidate; 1024: one
        grid_sums(x.data(), 2 * 1023 + 1, S.data(), widths);
        if (widths[0] || widths[1] || widths[2] || S[2] != GRID_NO_SUM) return fail("1023 elements", widths[0], 0, 0);
        grid_sums(x.data(), 2 * 1024, S.data(), widths);
        if (!widths[0] || widths[1] || widths[2] || S[512] == GRID_NO_SUM || S[513] != GRID_NO_SUM) return fail("1024 elements", widths[0], 0, 0);
        std::vector<uint8_t> z(4096, 0);
        grid_sums(z.data(), z.size(), S.data(), widths);
        if (widths[0] != 2 || widths[1] != 2 || widths[2] != 0) return fail("zeros", widths[0], widths[1], widths[2]);
    }
    for (int i = 0; i < 20000; i++) {
        uint32_t S[40];
        const uint32_t wm = 2 + (uint32_t)(rnd() % 38);
        for (uint32_t w = 0; w < 40; w++) S[w] = (uint32_t)(rnd() % (i % 2 ? 3 : 1000));
        uint32_t best = 2;
        for (uint32_t w = 2; w <= wm; w++)
            if (S[w] < S[best]) best = w;
        if (grid_argmin(S, wm) != best) return fail("grid_argmin", wm, best, (unsigned long long)i);
    }
    for (int i = 0; i < 300000; i++) {
        unsigned long long cost[GRID_CANDS];
        const unsigned long long base = 1 + rnd() % (1ull << 42);
        for (uint32_t c = 0; c < GRID_CANDS; c++) {
            const uint32_t how = (uint32_t)(rnd() % 5);
            cost[c] = how == 0 ? rnd() % (1ull << 43) : how == 1 ? base * 32 / 33 + rnd() % 5 - 2 : how == 2 ? base : how == 3 ? 0 : GRID_NO_COST;
            if (how < 3 && cost[c] > (1ull << 43)) cost[c] = 0;
        }
        if (cost[0] == GRID_NO_COST) cost[0] = base;              // (candidate 0 is the filter probe's: always a real cost)
        const uint32_t p = grid_pick(cost);
        if (p != pick_upto(cost, GRID_CANDS)) return fail("grid_pick", p, pick_upto(cost, GRID_CANDS), (unsigned long long)i);
        if (cost[p] == GRID_NO_COST) return fail("a candidate without a width was picked", p, 0, (unsigned long long)i);
        if (pick_upto(cost, LAG_CANDS) != lag_pick(cost)) return fail("the first ten are lag_rule.h's walk", 0, 0, (unsigned long long)i);
    }
    if (33 * GRID_NO_COST / 33 != GRID_NO_COST) return fail("33 GRID_NO_COST overflows", 0, 0, 0);
    for (uint32_t v : {0u, 1u, 2u, 3u, 65535u, 65536u, 65537u, 0x20000u, 0x80000002u, 0xFFFFFFFFu}) {
        const uint32_t c = grid_width_word(v);
        if (c != (v >= 2 && v <= 65536 ? v : 0u)) return fail("grid_width_word", v, c, 0);
    }

    // ---- part 2: the words
    CtFormat s14, s13, s10;
    s14.version = CT_VERSION_FILTER_GRID;
    s13.version = CT_VERSION_FILTER_LAG;
    s10.version = CT_VERSION_FILTER;
    unsigned words = 0, legal = 0;
    for (uint32_t width = 2; width <= 65536; width += (width < 70 || width > 65500 ? 1 : 97)) {
        const uint32_t lag = 1 + width % 16;
        const uint32_t lags[LAG_ELEMS] = {lag, lag, lag}, widths[LAG_ELEMS] = {width, width, width};
        for (uint32_t i = 0; i < GRID_CANDS; i++) {
            const GridCand c = grid_cand(i, lags, widths);
            CtFormat ff = s14;                                // as Encoder::frame() makes it
            ff.elem = c.elem > 1 ? c.elem : 0;
            ff.flags = c.delta ? CT_FLAG_DELTA | (c.fold ? CT_FLAG_FOLD : 0u) | (c.lag - 1u) << CT_LAG_SHIFT | (c.width ? CT_FLAG_GRID : 0u) : 0;
            ff.width = c.width;
            const uint32_t word = ct_frame_word(ff);
            words++;
            if (!ct_frame_word_legal(s14, word)) return fail("a writer's word is not legal", word, i, width);
            const CtFormat back = ct_frame_format(s14, word);
            if (back.elem != ff.elem || back.flags != ff.flags || back.width != ff.width || back.grid() != (i >= LAG_CANDS) || back.lag() != c.lag ||
                back.fold() != c.fold || back.delta() != (c.delta != 0)) return fail("a writer's word does not parse back", word, i, width);
            if (i < LAG_CANDS) {
                if (word >> 31 || !ct_frame_word_legal(s13, word) || ct_frame_word(ct_frame_format(s13, word)) != word) return fail("the first ten are version 13's words", word, i, 0);
            } else {
                if (word != (c.elem | width << 8 | 1u << 30 | 1u << 31)) return fail("the grid word", word, i, width);
                if (ct_frame_word_legal(s13, word) || ct_frame_word_legal(s10, word)) return fail("a grid word under version 13 or 10", word, i, width);
                if (c.fold != 1 || c.delta != 1 || c.lag != 1 || c.elem != (2u << (i - LAG_CANDS))) return fail("grid_cand", i, width, 0);
            }
        }
    }
    const uint32_t wfield[] = {0, 1, 2, 3, 640, 65535, 65536, 65537, 0x10001, 0x1FFFF};
    for (uint32_t version : {14u, 13u, 10u, 8u, 11u, 12u})
        for (uint32_t elem = 0; elem < 256; elem++)
            for (uint32_t w : wfield)
                for (uint32_t top = 0; top < 64; top++) {         // bits 25 .. 30
                    CtFormat st;
                    st.version = version;
                    const uint32_t word = elem | w << 8 | top << 25 | 1u << 31;
                    const bool want = want_grid_word(version, word);
                    if (ct_frame_word_legal(st, word) != want) return fail("ct_frame_word_legal of a bit-31 word", version, word, want);
                    if (!want) continue;
                    legal++;
                    const CtFormat f = ct_frame_format(st, word);
                    if (!f.grid() || f.elem != elem || f.width != w || f.fold() != (top >> 5) || f.lag() != 1 || !f.delta() || !f.filtered())
                        return fail("ct_frame_format of a grid word", version, word, 0);
                    if (ct_frame_word(f) != word) return fail("ct_frame_word of a grid frame's format", version, word, 0);
                }
    if (legal != 3 * 5 * 2) return fail("the count of legal grid words among those tried", legal, 0, 0);
    for (uint32_t flags = 0; flags < 32768; flags++)
        for (uint32_t elem = 0; elem <= 17; elem++) {
            const uint32_t word = elem | flags << 16;
            if (ct_frame_word_legal(s14, word) != ct_frame_word_legal(s13, word)) return fail("a bit-31-clear word under 14 and 13", flags, elem, 0);
            if (!ct_frame_word_legal(s14, word)) continue;
            const CtFormat a = ct_frame_format(s14, word), b = ct_frame_format(s13, word);
            if (a.grid() || a.width || a.elem != b.elem || a.flags != b.flags || a.lag() != b.lag() || a.fold() != b.fold()) return fail("its format", flags, elem, 0);
        }
    for (uint32_t v = 0; v <= 16; v++)
        for (uint32_t f = 0; f < 65536; f += (v == 14 ? 1 : 257))
            for (uint32_t e = 0; e <= 9; e++) {
                const uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, e, 0, 0, 0, 0};
                CtFormat a, b;
                const bool pa = parse_stream_format(h, &a), pb = parse_header_format(h, &b);
                if (pb != (pa || (v == 14 && f == 0 && e == 0)) || (v >= 14 && pa)) return fail("parse_header_format", v, f, e);
                if (pb && v == 14 && (b.reads() != CT_READS_FILTER_GRID || b.kinds() != ct_kinds(8) || b.filtered() || b.grid() || b.lag() != 1 || b.fold()))
                    return fail("version 14's format", v, f, e);
            }

    // ---- part 3: the setters
    const uint32_t lags[8][2] = {{1, 0}, {2, 0}, {1, 1}, {3, 1}, {16, 1}, {0, 0}, {17, 0}, {1, 2}};
    std::set<decltype(key(CtSettings()))> seen;
    std::vector<CtSettings> todo{CtSettings()};
    seen.insert(key(todo[0]));
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const CtSettings s = todo.back();
        todo.pop_back();
        if (s.filter_grid && !s.filter_lag) return fail("filter-grid is on without filter-lag", s.codec, s.mode, s.shuffle);
        if (s.filter_lag && !s.filter_auto) return fail("filter-lag is on without filter-auto", s.codec, s.mode, s.shuffle);
        const CtFormat f = format_of(s);
        if ((f.version == CT_VERSION_FILTER_GRID) != s.filter_grid) return fail("format_of's version", f.version, f.flags, f.elem);
        if (s.filter_grid && (f.flags || f.elem || f.width)) return fail("version 14's triple", f.version, f.flags, f.elem);
        if (((s.reader() & CT_READS_FILTER_GRID) != 0) != s.filter_grid) return fail("reader", s.reader(), 0, 0);
        if (s.filter_grid && (!(s.reader() & CT_READS_FILTER_LAG) || !(s.reader() & CT_READS_FILTER))) return fail("a filter-grid plan reads versions 13 and 10", s.reader(), 0, 0);
        CtSettings off = s;
        off.filter_grid = false;
        const CtFormat g = format_of(off);
        if (g.version == CT_VERSION_FILTER_GRID || (s.filter_grid && g.version != CT_VERSION_FILTER_LAG)) return fail("format_of with the setting off", g.version, g.flags, g.elem);
        if (!s.filter_grid && (g.version != f.version || g.flags != f.flags || g.elem != f.elem || g.width != f.width)) return fail("format_of changed", g.version, g.flags, g.elem);
        for (int k = 0; k < 13; k++) {
            const uint32_t vals[8] = {0, 1, 2, 3, 4, 8, 9, 1u << 31};
            for (int i = 0; i < 8; i++) {
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
                case 9: ok = t.set_delta_lag(lags[i][0], lags[i][1]); break;
                case 10: ok = t.set_delta_grid(vals[i] == 9 ? 1000 : vals[i], i & 1); break;
                case 11: ok = t.set_filter_lag(vals[i]); break;
                default: ok = t.set_filter_grid(vals[i]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (unsigned long long)k, (unsigned long long)i, 0);
                if (k == 12) {
                    if (ok != (vals[i] == 0 || (vals[i] == 1 && s.filter_lag))) return fail("set_filter_grid's answer", vals[i], s.filter_lag, 0);
                    if (ok && t.filter_grid != (vals[i] == 1)) return fail("set_filter_grid's effect", vals[i], 0, 0);
                    CtSettings u = t;
                    u.filter_grid = s.filter_grid;
                    if (key(u) != key(s)) return fail("set_filter_grid changed another setting", vals[i], 0, 0);
                } else if (ok && s.filter_grid && t.filter_lag && !t.filter_grid) {
                    return fail("a call that leaves filter-lag on switched filter-grid off", (unsigned long long)k, vals[i], 0);
                } else if (ok && !s.filter_grid && t.filter_grid) {
                    return fail("another setter switched filter-grid on", (unsigned long long)k, vals[i], 0);
                }
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }
    printf("filter_grid_rule_check: ok, %u writer words, %u legal grid words, %zu states, %llu calls\n", words, legal, seen.size(), calls);
    return 0;
}
