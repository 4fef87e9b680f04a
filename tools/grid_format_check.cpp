// grid_format_check.cpp -- a stand-alone host program around the format rule and the setters of csrc/container_internal.h as format
// version 12 (the 2-D predictor; INTEGRATION.md 4b "Delta: grid") left them.  It is meant to be built with the host sanitizers and
// run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/grid_format_check.cpp -o grid_format_check && ./grid_format_check
// Part 1, the rule by brute force: format_legal() through parse_format() against the rule stated outright below, over every flag
// word with a set of (elem, width) pairs and over every width 0 .. 2^17 with every elem <= 9 and a set of flag words, for versions
// 0 to 13 (so also: word 3 is split under version 12 only); the period P(W) against the smallest multiple of 2048 that holds 32
// rows; the writer's packing, format_of() of a plan with the setting on, for every width, elem and fold.  It prints one line
// "legal <version> <flags> <word 3>" per legal triple at the widths 2, 1000 and 65536 for tests/test_cpu_container_grid.py to hold
// against the model.
// Part 2 walks every state the setters reach from the default (each setter with in-range, boundary and out-of-range values, the
// delta-lag setter with (1,0) (3,1) (0,0), the grid setter with (0,0) (2,0) (1024,1) (65536,1) and the bad (1,0) (65537,0) (1024,2))
// and wants in every state: the grid is off unless the lag's prerequisites hold and the lag is (1, 0); format_of() is legal, is
// version 12 exactly when the grid is on and then says its width and fold, and is what it is without the setting when it is off;
// reader() has the version-12 bit exactly when it is on and never together with version 11's; a refused call changes nothing; the
// delta-lag setter takes only (1, 0) while the grid is on.  It prints
//   grid_format_check: ok, <legal> legal, <states> states, <calls> calls
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static int fail(const char *what, uint32_t a, uint32_t b, uint32_t c)
{
    printf("grid_format_check: FAILED %s at (%u, %u, %u)\n", what, a, b, c);
    return 1;
}

// the rule over the header's words, stated outright
static bool want_legal(uint32_t v, uint32_t f, uint32_t w3)
{
    const uint32_t e = v == 12 ? w3 & 255 : w3, w = v == 12 ? w3 >> 8 : 0;
    const bool elem248 = e == 2 || e == 4 || e == 8;
    if (v == 1) return f == 0 && e == 0;
    if (v == 2) return f == 0 && elem248;
    if (v == 3) return f == 0 && (e == 0 || elem248);
    if (v == 4) return f == 1 && elem248;
    if (v >= 5 && v <= 9) return (f == 0 && (e == 0 || elem248)) || (f == 1 && elem248);
    if (v == 10) return f == 0 && e == 0;
    if (v == 11) return (f & 1) && !(f & 0xF0FC) && (f & 0x0F02) && elem248;
    if (v == 12) return (f == 5 || f == 7) && elem248 && w >= 2 && w <= 65536;
    return false;
}

static unsigned long long legal = 0;

static int one(uint32_t v, uint32_t f, uint32_t e, uint32_t w)
{
    const uint32_t w3 = e | w << 8;
    const uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, w3, 0, 0, 0, 0};
    CtFormat fmt;
    const bool ok = parse_format(h, &fmt);
    if (ok != want_legal(v, f, w3)) return fail("format_legal", v, f, w3);
    if (v != CT_VERSION_GRID && (fmt.elem != w3 || fmt.width != 0)) return fail("word 3 split under another version", v, f, w3);
    if (!ok) return 0;
    legal++;
    if (w == 2 || w == 1000 || w == 65536 || v != CT_VERSION_GRID) printf("legal %u %u %u\n", v, f, w3);
    if (fmt.word3() != w3 || fmt.grid() != (v == 12) || fmt.delta() != ((f & 1) != 0)) return fail("word3 / grid / delta", v, f, w3);
    if (v == 12 && (fmt.elem != e || fmt.width != w || fmt.fold() != (f >> 1 & 1) || fmt.lag() != 1 || fmt.reads() != CT_READS_GRID ||
                    fmt.kinds() != ct_kinds(8)))
        return fail("version 12's fields", v, f, w3);
    if (v != 12 && fmt.reads() == CT_READS_GRID) return fail("reads", v, f, w3);
    return 0;
}

static auto key(const CtSettings &s)
{
    return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.lag, s.fold, s.grid_width, s.grid_fold);
}

int main()
{
    const uint32_t pairs[14][2] = {{0, 0}, {2, 0}, {4, 0}, {8, 0}, {2, 1}, {2, 2}, {4, 3}, {8, 64}, {3, 1000}, {4, 1000}, {8, 65535}, {2, 65536}, {4, 65537}, {8, 1u << 20}};
    for (uint32_t v = 0; v <= 13; v++)
        for (uint32_t f = 0; f < 65536; f++)
            for (int i = 0; i < 14; i++)
                if (one(v, f, pairs[i][0], pairs[i][1])) return 1;
    const uint32_t words[20] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 5 | 1 << 8, 7 | 1 << 8, 5 | 0x8000, 7 | 0x10};
    for (uint32_t v = 0; v <= 13; v++)
        for (uint32_t w = 0; w <= 1u << 17; w++) {
            if (v != 12 && w > 2 && w != 1000 && w != 65536) continue;      // (the rule over all widths is version 12's)
            for (uint32_t e = 0; e <= 9; e++)
                for (int i = 0; i < 20; i++) {
                    bool seen = false;                         // (the pairs above had this one)
                    for (int k = 0; k < 14; k++) seen |= pairs[k][0] == e && pairs[k][1] == w;
                    if (!seen && one(v, words[i], e, w)) return 1;
                }
        }
    // the period: the smallest multiple of 2048 that holds 32 rows
    for (uint32_t w = CT_GRID_MIN_WIDTH; w <= CT_GRID_MAX_WIDTH; w++) {
        uint32_t p = 2048;
        while (p < 32 * w) p += 2048;
        if (ct_grid_period(w) != p || p % 2048 || p < w || !ct_grid_width_ok(w)) return fail("the period", w, p, ct_grid_period(w));
    }
    if (ct_grid_width_ok(0) || ct_grid_width_ok(1) || ct_grid_width_ok(65537) || ct_grid_width_ok(~0u)) return fail("width range", 0, 0, 0);
    // the writer's packing
    for (uint32_t w = CT_GRID_MIN_WIDTH; w <= CT_GRID_MAX_WIDTH; w++)
        for (uint32_t e = 2; e <= 8; e *= 2)
            for (uint32_t fold = 0; fold <= 1; fold++) {
                CtSettings s;
                if (!s.set_codec(CT_CODEC_HUFF0) || !s.set_mode(CT_MODE_AUTO, 1) || !s.set_shuffle(e) || !s.set_delta(1) || !s.set_delta_grid(w, fold))
                    return fail("the setters on the way to the grid", w, e, fold);
                const CtFormat f = format_of(s);
                if (f.version != 12 || f.flags != (1u | fold << 1 | 4u) || f.word3() != (e | w << 8) || !format_legal(f)) return fail("the packing", w, e, fold);
            }

    const uint32_t lags[3][2] = {{1, 0}, {3, 1}, {0, 0}};
    const uint32_t grids[7][2] = {{0, 0}, {2, 0}, {1024, 1}, {65536, 1}, {1, 0}, {65537, 0}, {1024, 2}};
    std::set<decltype(key(CtSettings()))> seen;
    std::vector<CtSettings> todo{CtSettings()};
    seen.insert(key(todo[0]));
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const CtSettings s = todo.back();
        todo.pop_back();
        if (s.grid_on() && (!s.lag_fits() || s.lag_on())) return fail("the grid is on without its prerequisites", s.grid_width, s.lag, s.shuffle);
        if (s.grid_width == 1 || s.grid_width > 65536 || s.grid_fold > 1 || (!s.grid_on() && s.grid_fold)) return fail("the setting is out of range", s.grid_width, s.grid_fold, 0);
        const CtFormat f = format_of(s);
        if (!format_legal(f)) return fail("format_of is not legal", f.version, f.flags, f.word3());
        if ((f.version == CT_VERSION_GRID) != s.grid_on() || f.width != s.grid_width || (s.grid_on() && f.fold() != s.grid_fold))
            return fail("format_of's grid", f.version, f.flags, f.word3());
        if (((s.reader() & CT_READS_GRID) != 0) != s.grid_on() || (s.reader() & (CT_READS_GRID | CT_READS_LAG)) == (CT_READS_GRID | CT_READS_LAG))
            return fail("reader", s.reader(), s.grid_width, s.lag);
        if (s.grid_on()) {
            CtSettings off = s;
            off.grid_width = 0; off.grid_fold = 0;
            const CtFormat g = format_of(off);
            if (g.version != CT_VERSION_AUTO || g.flags != CT_FLAG_DELTA || g.elem != f.elem || g.width) return fail("format_of with the grid off", g.version, g.flags, g.elem);
        }
        for (int k = 0; k < 11; k++) {
            const uint32_t vals[8] = {0, 1, 2, 3, 4, 8, 9, 1u << 31};
            for (int i = 0; i < (k == 9 ? 3 : k == 10 ? 7 : 8); i++) {
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
                default: ok = t.set_delta_grid(grids[i][0], grids[i][1]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (uint32_t)k, (uint32_t)i, 0);
                if (k == 10) {
                    const bool good = i < 4, off = i == 0;
                    if (ok != (good && (off || (s.lag_fits() && !s.lag_on())))) return fail("set_delta_grid's answer", grids[i][0], grids[i][1], s.shuffle);
                    if (ok && (t.grid_width != grids[i][0] || t.grid_fold != grids[i][1])) return fail("set_delta_grid's effect", grids[i][0], grids[i][1], 0);
                } else if (k == 9) {
                    if (s.grid_on() && ok != (i == 0)) return fail("set_delta_lag while the grid is on", lags[i][0], lags[i][1], 0);
                    if (s.grid_on() && (t.grid_width != s.grid_width || t.grid_fold != s.grid_fold)) return fail("set_delta_lag changed the grid", lags[i][0], lags[i][1], 0);
                } else if (ok && s.grid_on() && t.lag_fits() && (t.grid_width != s.grid_width || t.grid_fold != s.grid_fold)) {
                    return fail("a call that ends no prerequisite changed the setting", (uint32_t)k, vals[i], 0);
                } else if (ok && !t.lag_fits() && t.grid_on()) {
                    return fail("a call that ends a prerequisite kept the setting", (uint32_t)k, vals[i], 0);
                }
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }
    printf("grid_format_check: ok, %llu legal, %zu states, %llu calls\n", legal, seen.size(), calls);
    return 0;
}
