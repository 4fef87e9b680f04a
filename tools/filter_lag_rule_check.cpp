// filter_lag_rule_check.cpp -- a stand-alone host program around csrc/lag_rule.h and the format helpers and setters of
// csrc/container_internal.h as format version 13 (filter-auto with lag; INTEGRATION.md 4b "Filter: auto with lag") left them.  It is
// meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/filter_lag_rule_check.cpp -o filter_lag_rule_check && ./filter_lag_rule_check
// Part 1, the rule: lag_bitlen() against a loop; lag_fold() against the zigzag of the signed difference; lag_argmin() with ties
// against the first minimum; lag_sums() of a small buffer against a direct restatement; lag_pick() over ten costs against a
// recursive restatement on random costs, costs near the margin among them; lag_clamp() over every word near its edges.
// Part 2, the words: every word the writer can make (the seven of filter_rule.h and elem 2, 4, 8 x lag 1..16 with the fold) is
// legal under version 13 and parses back to its elem, delta, lag and fold; ct_frame_word_legal() under versions 13 and 10 against
// the rule stated outright over every (flags < 65536, elem <= 17), the refusal list of tests/filter_lag_model.py by name; the
// stream header's triple: (13, 0, 0) alone, through parse_stream_format() only.
// Part 3, the setters: every state the setters reach from the default wants filter-lag on only with filter-auto on, format_of()
// version 13 exactly then and what it was with the setting off, reader() with the version-13 bit exactly then, a refused call
// changing nothing, and set_filter_lag(1) accepted exactly with filter-auto on.  It prints
//   filter_lag_rule_check: ok, <words> writer words, <legal> legal words, <states> states, <calls> calls
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"
#include "../gpu-lossless-compression_amd/csrc/lag_rule.h"

#include <stdio.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    printf("filter_lag_rule_check: FAILED %s at (%llu, %llu, %llu)\n", what, a, b, c);
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

static uint32_t pick_upto(const unsigned long long *cost, uint32_t n)      // the walk over the first n candidates, restated
{
    if (n == 1) return 0;
    const uint32_t p = pick_upto(cost, n - 1);
    return 33 * cost[n - 1] < 32 * cost[p] ? n - 1 : p;
}

// the frame word's rule, stated outright
static bool want_word(uint32_t version, uint32_t flags, uint32_t elem)
{
    if (version != 10 && version != 13) return flags == 0 && elem == 0;
    if (elem == 0) return flags == 0;
    if (elem != 2 && elem != 4 && elem != 8) return false;
    if (flags <= 1) return true;
    return version == 13 && (flags & 1) && !(flags & 0xF0FC) && (flags & 0x0F02);
}

static auto key(const CtSettings &s)
{
    return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.filter_lag, s.lag, s.fold, s.grid_width, s.grid_fold);
}

int main()
{
    // ---- part 1: the rule
    for (uint32_t k = 0; k < 64; k++)
        for (long long d = -2; d <= 2; d++) {
            const unsigned long long v = (1ull << k) + (unsigned long long)d;
            if (lag_bitlen(v) != loop_bitlen(v)) return fail("lag_bitlen", v, k, 0);
        }
    if (lag_bitlen(0) != 0 || lag_bitlen(~0ull) != 64) return fail("lag_bitlen at the ends", 0, 0, 0);
    for (int i = 0; i < 200000; i++) {
        const unsigned long long v = rnd() >> (rnd() & 63);
        if (lag_bitlen(v) != loop_bitlen(v)) return fail("lag_bitlen", v, 0, 0);
    }
    for (uint32_t e = 2; e <= 8; e *= 2) {
        const uint32_t W = 8 * e;
        const unsigned long long mask = W == 64 ? ~0ull : (1ull << W) - 1;
        for (int i = 0; i < 100000; i++) {
            const unsigned long long d = (i < 8 ? (unsigned long long)(i - 4) : i < 12 ? (1ull << (W - 1)) + (unsigned long long)(i - 10) : rnd() >> (rnd() & 63)) & mask;
            const bool neg = (d >> (W - 1)) & 1;
            // the signed difference s: zigzag is 2 s for s >= 0 and -2 s - 1 for s < 0, modulo 2^W
            const unsigned long long want = neg ? ((~d & mask) * 2 + 1) & mask : (d * 2) & mask;
            if (lag_fold(d, e) != want) return fail("lag_fold", d, e, want);
        }
    }
    for (int i = 0; i < 100000; i++) {
        unsigned long long S[LAG_MAX];
        for (uint32_t l = 0; l < LAG_MAX; l++) S[l] = rnd() % (i % 3 == 0 ? 3 : i % 3 == 1 ? 17 : 1ull << 36);     // (small ranges: ties)
        uint32_t w = 0;
        for (uint32_t l = 0; l < LAG_MAX; l++) {
            bool smaller_before = false;
            for (uint32_t m = 0; m < l; m++) smaller_before = smaller_before || S[m] <= S[l];
            bool smaller_after = false;
            for (uint32_t m = l + 1; m < LAG_MAX; m++) smaller_after = smaller_after || S[m] < S[l];
            if (!smaller_before && !smaller_after) w = l + 1;
        }
        if (lag_argmin(S) != w) return fail("lag_argmin", w, lag_argmin(S), (unsigned long long)i);
    }
    {
        const unsigned long long zero[LAG_MAX] = {};
        if (lag_argmin(zero) != 1) return fail("lag_argmin of zeros", 0, 0, 0);
    }
    {
        // 3 runs and a bit of 2-byte elements, 4-channel data with noise: the sums against a direct restatement
        std::vector<uint8_t> x(2 * 2048 * 3 + 531);
        for (size_t i = 0; i < x.size(); i++) x[i] = (uint8_t)((i / 2 % 4) * 37 + (i % 2 ? 0 : rnd() % 5));
        unsigned long long S[LAG_SUMS];
        lag_sums(x.data(), x.size(), S);
        const size_t P = x.size() - x.size() % 8;
        for (uint32_t e = 2; e <= 8; e *= 2)
            for (uint32_t l = 1; l <= LAG_MAX; l++) {
                unsigned long long want = 0;
                for (size_t i = 0; i < P / e; i++) {
                    unsigned long long cur = 0, prev = 0;
                    for (uint32_t b = 0; b < e; b++) cur |= (unsigned long long)x[i * e + b] << (8 * b);
                    if (i % 2048 >= l) for (uint32_t b = 0; b < e; b++) prev |= (unsigned long long)x[(i - l) * e + b] << (8 * b);
                    const unsigned long long m = e == 8 ? ~0ull : (1ull << (8 * e)) - 1, d = (cur - prev) & m;
                    const unsigned long long f = ((d >> (8 * e - 1)) & 1) ? ((~d & m) * 2 + 1) & m : (d * 2) & m;
                    want += loop_bitlen(f);
                }
                if (S[lag_sum_row(e, l)] != want) return fail("lag_sums", e, l, want);
            }
        if (lag_argmin(S) != 4) return fail("the winner of four 2-byte channels", lag_argmin(S), 0, 0);
    }
    for (int i = 0; i < 300000; i++) {
        unsigned long long cost[LAG_CANDS];
        const unsigned long long base = 1 + rnd() % (1ull << 42);
        for (uint32_t c = 0; c < LAG_CANDS; c++) {
            const uint32_t how = (uint32_t)(rnd() % 4);
            // free, at the margin of the base (33 c < 32 base flips within +-2), equal, or zero
            cost[c] = how == 0 ? rnd() % (1ull << 43) : how == 1 ? base * 32 / 33 + rnd() % 5 - 2 : how == 2 ? base : 0;
            if (cost[c] > (1ull << 43)) cost[c] = 0;
        }
        if (lag_pick(cost) != pick_upto(cost, LAG_CANDS)) return fail("lag_pick", lag_pick(cost), pick_upto(cost, LAG_CANDS), (unsigned long long)i);
        if (pick_upto(cost, FILTER_CANDS) != filter_pick(cost)) return fail("the first seven are filter_rule.h's walk", 0, 0, (unsigned long long)i);
    }
    for (uint32_t v : {0u, 1u, 2u, 15u, 16u, 17u, 18u, 32u, 33u, 0xFFFFFFFFu, 0x80000000u}) {
        const uint32_t c = lag_clamp(v);
        if (c < 1 || c > LAG_MAX || (v >= 1 && v <= LAG_MAX && c != v)) return fail("lag_clamp", v, c, 0);
    }
    if (lag_clamp(0) != 16 || lag_clamp(17) != 1) return fail("lag_clamp of 0 and 17", lag_clamp(0), lag_clamp(17), 0);
    if (lag_sum_row(2, 1) != 0 || lag_sum_row(4, 1) != 16 || lag_sum_row(8, 16) != 47 || lag_plane_row(2) != 0 || lag_plane_row(4) != 2 ||
        lag_plane_row(8) != 6 || lag_plane_row(8) + 8 != LAG_ROWS) return fail("the row layout", 0, 0, 0);

    // ---- part 2: the words
    CtFormat s13, s10;
    s13.version = CT_VERSION_FILTER_LAG;
    s10.version = CT_VERSION_FILTER;
    unsigned words = 0, legal = 0;
    for (uint32_t lag = 1; lag <= LAG_MAX; lag++) {
        const uint32_t lags[LAG_ELEMS] = {lag, lag, lag};
        for (uint32_t i = 0; i < LAG_CANDS; i++) {
            if (i < FILTER_CANDS && lag > 1) continue;
            const LagCand c = lag_cand(i, lags);
            CtFormat ff = s13;                                // as Encoder::frame() makes it
            ff.elem = c.elem > 1 ? c.elem : 0;
            ff.flags = c.delta ? CT_FLAG_DELTA | (c.fold ? CT_FLAG_FOLD : 0u) | (c.lag - 1u) << CT_LAG_SHIFT : 0;
            const uint32_t word = ct_frame_word(ff);
            words++;
            if (!ct_frame_word_legal(s13, word)) return fail("a writer's word is not legal", word, i, lag);
            const CtFormat back = ct_frame_format(s13, word);
            if (back.elem != ff.elem || back.delta() != (c.delta != 0) || back.lag() != c.lag || back.fold() != c.fold || back.grid())
                return fail("a writer's word does not parse back", word, i, lag);
            if (i < FILTER_CANDS) {
                if (!ct_frame_word_legal(s10, word) || ct_frame_word(ct_frame_format(s10, word)) != word) return fail("the first seven are version 10's words", word, i, 0);
            } else if (ct_frame_word_legal(s10, word)) return fail("a lag word under version 10", word, i, lag);
            if (i >= FILTER_CANDS && (c.fold != 1 || c.delta != 1 || c.elem != (2u << (i - FILTER_CANDS)))) return fail("lag_cand", i, lag, 0);
        }
    }
    for (uint32_t version : {13u, 10u, 8u, 11u, 12u})
        for (uint32_t flags = 0; flags < 65536; flags++)
            for (uint32_t elem = 0; elem <= 17; elem++) {
                CtFormat st;
                st.version = version;
                const uint32_t word = elem | flags << 16;
                if (ct_frame_word_legal(st, word) != want_word(version, flags, elem)) return fail("ct_frame_word_legal", version, flags, elem);
                if (version != 13 || !want_word(version, flags, elem)) continue;
                legal++;
                const CtFormat f = ct_frame_format(st, word);
                const bool lagged = flags > 1;
                if (f.elem != elem || f.lag() != (lagged ? (flags >> 8 & 15) + 1 : 1u) || f.fold() != (lagged ? flags >> 1 & 1 : 0u) ||
                    f.delta() != ((flags & 1) != 0)) return fail("ct_frame_format", version, flags, elem);
            }
    if (legal != 1 + 3 * 2 + 3 * 31) return fail("the count of legal words", legal, 0, 0);
    {
        // the refusal list by name, on the word (2, lag 8, fold): 2 | (1 | 2 | 7 << 8) << 16
        const uint32_t fl = 1 | 2 | 7 << 8;
        const uint32_t bad[] = {0u | fl << 16, 2u | (fl | 4) << 16, 2u | (fl | 0x80) << 16, 2u | (fl | 0x1000) << 16, 2u | (fl | 0x8000) << 16,
                                3u | fl << 16, 16u | fl << 16, 1u | fl << 16, 2u | 2u << 16, 2u | (fl & ~1u) << 16};
        for (uint32_t w : bad)
            if (ct_frame_word_legal(s13, w)) return fail("an illegal word of the refusal list is legal", w, 0, 0);
        if (!ct_frame_word_legal(s13, 2u | fl << 16) || !ct_frame_word_legal(s13, 8u | (1u | 15u << 8) << 16)) return fail("(lag > 1, fold 0) is legal", 0, 0, 0);
    }
    for (uint32_t v = 0; v <= 15; v++)
        for (uint32_t f = 0; f < 65536; f += (v == 13 ? 1 : 257))
            for (uint32_t e = 0; e <= 9; e++) {
                const uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, e, 0, 0, 0, 0};
                CtFormat a, b;
                const bool pa = parse_format(h, &a), pb = parse_stream_format(h, &b);
                if (pb != (pa || (v == 13 && f == 0 && e == 0)) || (v >= 13 && pa)) return fail("parse_stream_format", v, f, e);
                if (pb && v == 13 && (b.reads() != CT_READS_FILTER_LAG || b.kinds() != ct_kinds(8) || b.filtered() || b.lag() != 1 || b.fold())) return fail("version 13's format", v, f, e);
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
        if (s.filter_lag && !s.filter_auto) return fail("filter-lag is on without filter-auto", s.codec, s.mode, s.shuffle);
        if (s.filter_auto && (s.codec != CT_CODEC_HUFF0 || s.mode != CT_MODE_AUTO || s.shuffle)) return fail("filter-auto's prerequisites", s.codec, s.mode, s.shuffle);
        const CtFormat f = format_of(s);
        if ((f.version == CT_VERSION_FILTER_LAG) != s.filter_lag) return fail("format_of's version", f.version, f.flags, f.elem);
        if (s.filter_lag && (f.flags || f.elem || f.width)) return fail("version 13's triple", f.version, f.flags, f.elem);
        if (((s.reader() & CT_READS_FILTER_LAG) != 0) != s.filter_lag) return fail("reader", s.reader(), 0, 0);
        if (s.filter_lag && !(s.reader() & CT_READS_FILTER)) return fail("a filter-lag plan reads version 10", s.reader(), 0, 0);
        CtSettings off = s;
        off.filter_lag = false;
        const CtFormat g = format_of(off);
        if (g.version == CT_VERSION_FILTER_LAG || (s.filter_lag && g.version != CT_VERSION_FILTER)) return fail("format_of with the setting off", g.version, g.flags, g.elem);
        if (!s.filter_lag && (g.version != f.version || g.flags != f.flags || g.elem != f.elem || g.width != f.width)) return fail("format_of changed", g.version, g.flags, g.elem);
        for (int k = 0; k < 12; k++) {
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
                default: ok = t.set_filter_lag(vals[i]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (unsigned long long)k, (unsigned long long)i, 0);
                if (k == 11) {
                    if (ok != (vals[i] == 0 || (vals[i] == 1 && s.filter_auto))) return fail("set_filter_lag's answer", vals[i], s.filter_auto, 0);
                    if (ok && t.filter_lag != (vals[i] == 1)) return fail("set_filter_lag's effect", vals[i], 0, 0);
                    CtSettings u = t;
                    u.filter_lag = s.filter_lag;
                    if (key(u) != key(s)) return fail("set_filter_lag changed another setting", vals[i], 0, 0);
                } else if (ok && s.filter_lag && t.filter_auto && !t.filter_lag) {
                    return fail("a call that leaves filter-auto on switched filter-lag off", (unsigned long long)k, vals[i], 0);
                } else if (ok && !s.filter_lag && t.filter_lag) {
                    return fail("another setter switched filter-lag on", (unsigned long long)k, vals[i], 0);
                }
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }
    printf("filter_lag_rule_check: ok, %u writer words, %u legal words, %zu states, %llu calls\n", words, legal, seen.size(), calls);
    return 0;
}
