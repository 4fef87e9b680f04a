// byte_format_check.cpp -- a stand-alone host program around the format rule and the setters of csrc/container_internal.h as format
// version 15 (the byte predictor; INTEGRATION.md 4b "Delta: bytes") left them.  It is meant to be built with the host sanitizers and
// run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/byte_format_check.cpp -o byte_format_check && ./byte_format_check
// Part 1, the rule by brute force: parse_container_format() over versions 0 to 17, every flags word and a set of word-3 values,
// against parse_header_format() for every version but 15 (their answers must not have changed) and against version 15's rule
// stated outright below; the fields of a legal version-15 format.  It prints one line "legal <flags> <word 3>" per legal pair at
// the strides 0, 2, 1281 and 65536 for tests/test_cpu_byte_delta.py to hold against the model.
// Part 2, the packing round trip: for every lag 1..16 and every stride 0, 2..65536 the writer's format_of() gives flags
// 1 | (stride ? 4 : 0) | (lag - 1) << 8 and word 3 1 | stride << 8, and the reader gets lag and stride back from those words.
// Part 3 walks every state the setters reach from the default (each setter with in-range, boundary and out-of-range values, the
// byte-delta setter with (0,0) (1,0) (3,1281) (16,65536) and the bad (17,0) (3,1) (3,65537)) and wants in every state: the setting is
// on only with the order-0 codec, the auto mode, the shuffle off and filter-auto off; format_of() is version 15 exactly when it is
// on and is the format of the same settings without it when it is off; reader() has the version-15 bit exactly when it is on; a
// refused call changes nothing; while it is on the shuffle at 2, 4 or 8 and filter-auto are refused.
// Part 4, the range rounding rule: ct_byte_step() is 2048 at stride 0 and otherwise the smallest multiple of 2048 that holds 32
// rows, and the byte a range read starts its inverse at is the largest multiple of it at or below the range's first byte.
// It prints
//   byte_format_check: ok, <legal> legal, <packings> packings, <states> states, <calls> calls
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    printf("byte_format_check: FAILED %s at (%llu, %llu, %llu)\n", what, a, b, c);
    return 1;
}

// version 15's rule over the header's words, stated outright
static bool want15(uint32_t f, uint32_t w3)
{
    const uint32_t stride = w3 >> 8;
    if ((w3 & 255) != 1) return false;
    if (stride == 1 || stride > 65536) return false;
    if (!(f & 1)) return false;
    for (uint32_t bit = 0; bit < 16; bit++)
        if ((f >> bit & 1) && bit != 0 && bit != 2 && !(bit >= 8 && bit <= 11)) return false;
    return ((f >> 2 & 1) != 0) == (stride != 0);
}

static auto key(const CtSettings &s)
{
    return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.filter_lag, s.filter_grid, s.lag, s.fold, s.grid_width,
                           s.grid_fold, s.byte_lag, s.byte_stride);
}

int main()
{
    // ---- part 1: the rule
    std::vector<uint32_t> words;
    const uint32_t strides[12] = {0, 1, 2, 3, 64, 600, 1281, 65535, 65536, 65537, 1u << 20, (1u << 24) - 1};
    const uint32_t lows[8] = {0, 1, 2, 3, 4, 8, 9, 255};
    for (uint32_t s : strides)
        for (uint32_t e : lows) words.push_back(e | s << 8);
    unsigned long long legal = 0;
    for (uint32_t v = 0; v <= 17; v++)
        for (uint32_t f = 0; f < 65536; f++)
            for (uint32_t w3 : words) {
                if (v != CT_VERSION_BYTE && f > 32 && ((w3 >> 8) > 2 || (w3 & 255) > 4)) continue;      // (every flags word at 15 words, 33 at the rest)
                const uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, w3, 0, 0, 0, 0};
                CtFormat a, b;
                const bool pa = parse_header_format(h, &a), pb = parse_container_format(h, &b);
                if (v != CT_VERSION_BYTE) {
                    if (pa != pb) return fail("another version's answer changed", v, f, w3);
                    if (pb && (b.bytes() || b.reads() == CT_READS_BYTE)) return fail("another version's format", v, f, w3);
                    continue;
                }
                if (pa) return fail("parse_header_format accepts version 15", v, f, w3);
                if (pb != want15(f, w3) || pb != ct_byte_legal(f, w3)) return fail("version 15's rule", v, f, w3);
                if (!pb) continue;
                legal++;
                const uint32_t stride = w3 >> 8;
                if (stride == 0 || stride == 2 || stride == 1281 || stride == 65536) printf("legal %u %u\n", f, w3);
                if (!b.bytes() || b.grid() || !b.delta() || !b.filtered() || b.elem != 1 || b.width != stride || b.lag() != (f >> 8 & 15) + 1 || b.fold() ||
                    b.word3() != w3 || b.reads() != CT_READS_BYTE || b.kinds() != ct_kinds(8) || b.frame_filters())
                    return fail("version 15's fields", v, f, w3);
                if (ct_frame_word_legal(b, 1) || !ct_frame_word_legal(b, 0)) return fail("version 15's frame word", v, f, w3);
            }
    if (ct_kinds(15) != ct_kinds(8) || ct_kinds(16) != 0) return fail("ct_kinds", ct_kinds(15), ct_kinds(16), 0);

    // ---- part 2: the packing round trip
    unsigned long long packings = 0;
    for (uint32_t lag = 1; lag <= 16; lag++)
        for (uint32_t stride = 0; stride <= 65536; stride++) {
            if (stride == 1) continue;
            CtSettings s;
            if (!s.set_codec(CT_CODEC_HUFF0) || !s.set_mode(CT_MODE_AUTO, 1) || !s.set_byte_delta(lag, stride)) return fail("the setters on the way", lag, stride, 0);
            const CtFormat f = format_of(s);
            if (f.version != 15 || f.flags != (1u | (stride ? 4u : 0u) | (lag - 1) << 8) || f.word3() != (1u | stride << 8)) return fail("the packing", lag, stride, f.flags);
            uint32_t h[8];
            h[0] = CT_MAGIC_STREAM; h[1] = f.version | (f.flags << 16); h[2] = 4096; h[3] = f.word3(); h[4] = h[5] = h[6] = h[7] = 0;
            CtFormat back;
            if (!parse_container_format(h, &back) || back.lag() != lag || back.width != stride || !back.bytes() || back.elem != 1) return fail("the way back", lag, stride, 0);
            packings++;
        }

    // ---- part 3: the setters
    const uint32_t bytes[7][2] = {{0, 0}, {1, 0}, {3, 1281}, {16, 65536}, {17, 0}, {3, 1}, {3, 65537}};
    const uint32_t lags[3][2] = {{1, 0}, {3, 1}, {0, 0}};
    const uint32_t grids[3][2] = {{0, 0}, {1024, 1}, {1, 0}};
    std::set<decltype(key(CtSettings()))> seen;
    std::vector<CtSettings> todo{CtSettings()};
    seen.insert(key(todo[0]));
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const CtSettings s = todo.back();
        todo.pop_back();
        if (s.byte_on() && (s.codec != CT_CODEC_HUFF0 || s.mode != CT_MODE_AUTO || s.shuffle || s.delta || s.filter_auto || s.lag_on() || s.grid_on()))
            return fail("the setting is on without its prerequisites", s.byte_lag, s.codec, s.shuffle);
        if (s.byte_lag > 16 || s.byte_stride == 1 || s.byte_stride > 65536 || (!s.byte_on() && s.byte_stride)) return fail("the setting is out of range", s.byte_lag, s.byte_stride, 0);
        const CtFormat f = format_of(s);
        if ((f.version == CT_VERSION_BYTE) != s.byte_on()) return fail("format_of's version", f.version, s.byte_lag, s.byte_stride);
        if (s.byte_on() && (f.lag() != s.byte_lag || f.width != s.byte_stride || f.elem != 1)) return fail("format_of's byte fields", f.flags, f.word3(), 0);
        if (!s.byte_on() && !format_legal(f) && !f.frame_filters()) return fail("format_of is not legal", f.version, f.flags, f.word3());
        if (((s.reader() & CT_READS_BYTE) != 0) != s.byte_on()) return fail("reader", s.reader(), s.byte_lag, 0);
        if (s.byte_on() && (s.reader() & (CT_READS_LAG | CT_READS_GRID | CT_READS_FILTER))) return fail("reader speaks another setting's version", s.reader(), 0, 0);
        if (s.byte_on()) {
            CtSettings off = s;
            off.byte_lag = 0; off.byte_stride = 0;
            const CtFormat g = format_of(off);
            if (g.version != CT_VERSION_AUTO || g.flags || g.elem || g.width) return fail("format_of with the setting off", g.version, g.flags, g.elem);
        }
        for (int k = 0; k < 14; k++) {
            const uint32_t vals[8] = {0, 1, 2, 3, 4, 8, 9, 1u << 31};
            for (int i = 0; i < (k == 9 || k == 10 ? 3 : k == 13 ? 7 : 8); i++) {
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
                case 10: ok = t.set_delta_grid(grids[i][0], grids[i][1]); break;
                case 11: ok = t.set_filter_lag(vals[i]); break;
                case 12: ok = t.set_filter_grid(vals[i]); break;
                default: ok = t.set_byte_delta(bytes[i][0], bytes[i][1]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (unsigned long long)k, (unsigned long long)i, 0);
                if (k == 13) {
                    const bool good = i < 4, off = i == 0;
                    const bool fits = s.codec == CT_CODEC_HUFF0 && s.mode == CT_MODE_AUTO && !s.shuffle && !s.filter_auto;
                    if (ok != (good && (off || fits))) return fail("set_byte_delta's answer", bytes[i][0], bytes[i][1], s.shuffle);
                    if (ok && (t.byte_lag != bytes[i][0] || t.byte_stride != bytes[i][1])) return fail("set_byte_delta's effect", bytes[i][0], bytes[i][1], 0);
                    CtSettings u = t;
                    u.byte_lag = s.byte_lag; u.byte_stride = s.byte_stride;
                    if (key(u) != key(s)) return fail("set_byte_delta changed another setting", bytes[i][0], bytes[i][1], 0);
                } else if (s.byte_on()) {
                    if (k == 0 && vals[i] > 1 && ok) return fail("the shuffle was accepted while the setting is on", vals[i], 0, 0);
                    if (k == 8 && vals[i] == 1 && ok) return fail("filter-auto was accepted while the setting is on", vals[i], 0, 0);
                    const bool fits = t.codec == CT_CODEC_HUFF0 && t.mode == CT_MODE_AUTO;
                    if (ok && fits && (t.byte_lag != s.byte_lag || t.byte_stride != s.byte_stride)) return fail("a call that ends no prerequisite changed the setting", (unsigned long long)k, vals[i], 0);
                    if (ok && !fits && t.byte_on()) return fail("a call that ends a prerequisite kept the setting", (unsigned long long)k, vals[i], 0);
                } else if (ok && t.byte_on()) {
                    return fail("another setter switched the setting on", (unsigned long long)k, vals[i], 0);
                }
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }

    // ---- part 4: the range rounding rule
    if (ct_byte_step(0) != 2048) return fail("the step at stride 0", ct_byte_step(0), 0, 0);
    for (uint32_t stride = 2; stride <= 65536; stride++) {
        uint32_t p = 2048;
        while (p < 32 * stride) p += 2048;
        if (ct_byte_step(stride) != p || !ct_byte_stride_ok(stride)) return fail("the step", stride, p, ct_byte_step(stride));
    }
    if (!ct_byte_stride_ok(0) || ct_byte_stride_ok(1) || ct_byte_stride_ok(65537) || ct_byte_stride_ok(~0u) || ct_byte_lag_ok(0) || ct_byte_lag_ok(17) || !ct_byte_lag_ok(16))
        return fail("the ranges", 0, 0, 0);
    const uint32_t some[6] = {0, 2, 65, 600, 1281, 65536};
    for (uint32_t stride : some) {
        const unsigned long long step = ct_byte_step(stride);
        for (unsigned long long a = 0; a < 5 * step; a += (a % step < 3 || a % step > step - 4) ? 1 : 509) {
            unsigned long long want = 0;
            while (want + step <= a) want += step;
            if (a - a % step != want) return fail("the rounding", stride, a, want);
        }
    }
    printf("byte_format_check: ok, %llu legal, %llu packings, %zu states, %llu calls\n", legal, packings, seen.size(), calls);
    return 0;
}
