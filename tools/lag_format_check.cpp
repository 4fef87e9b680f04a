// lag_format_check.cpp -- a stand-alone host program around the format rule and the setters of csrc/container_internal.h as format
// version 11 (the lagged, folded delta; INTEGRATION.md 4b "Delta: lag and fold") left them.  It is meant to be built with the host
// sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/lag_format_check.cpp -o lag_format_check && ./lag_format_check
// Part 1 walks every triple (version <= 12, flags < 65536, elem <= 9): format_legal() against the rule stated outright below,
// lag() and fold() of every legal triple, reads() of every version; it prints one line "legal <version> <flags> <elem>" per legal
// triple for tests/test_cpu_container_lag.py to hold against the model's table.
// Part 2 walks every state the setters reach from the default (each setter with in-range, boundary and out-of-range values, the
// delta-lag setter with (1,0) (2,0) (1,1) (3,1) (16,1) and the bad (0,0) (17,0) (1,2)) and wants in every state: the setting
// is (1, 0) unless the order-0 codec, the auto mode, the shuffle and the delta are on and filter-auto is off; format_of() is legal,
// is version 11 exactly when the setting is on and then says the setting's lag and fold, and is what it was before this version
// with the setting off; reader() has the version-11 bit exactly when the setting is on; a refused call changes nothing.  It prints
//   lag_format_check: ok, <legal> legal triples, <states> states, <calls> calls
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static int fail(const char *what, uint32_t a, uint32_t b, uint32_t c)
{
    printf("lag_format_check: FAILED %s at (%u, %u, %u)\n", what, a, b, c);
    return 1;
}

// the rule, stated outright
static bool want_legal(uint32_t v, uint32_t f, uint32_t e)
{
    const bool elem248 = e == 2 || e == 4 || e == 8;
    if (v == 1) return f == 0 && e == 0;
    if (v == 2) return f == 0 && elem248;
    if (v == 3) return f == 0 && (e == 0 || elem248);
    if (v == 4) return f == 1 && elem248;
    if (v >= 5 && v <= 9) return (f == 0 && (e == 0 || elem248)) || (f == 1 && elem248);
    if (v == 10) return f == 0 && e == 0;
    if (v == 11) return (f & 1) && !(f & 0xF0FC) && (f & 0x0F02) && elem248;
    return false;
}

static auto key(const CtSettings &s) { return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.lag, s.fold); }

int main()
{
    unsigned legal = 0;
    for (uint32_t v = 0; v <= 12; v++)
        for (uint32_t f = 0; f < 65536; f++)
            for (uint32_t e = 0; e <= 9; e++) {
                CtFormat fmt;
                fmt.version = v; fmt.flags = f; fmt.elem = e;
                if (format_legal(fmt) != want_legal(v, f, e)) return fail("format_legal", v, f, e);
                if (!format_legal(fmt)) continue;
                legal++;
                printf("legal %u %u %u\n", v, f, e);
                const uint32_t lag = v == 11 ? (f >> 8 & 15) + 1 : 1, fold = v == 11 ? f >> 1 & 1 : 0;
                if (fmt.lag() != lag || fmt.fold() != fold || fmt.delta() != ((f & 1) != 0)) return fail("lag / fold / delta", v, f, e);
                if ((fmt.reads() == CT_READS_LAG) != (v == 11) || fmt.kinds() != ct_kinds(v == 11 ? 8 : v)) return fail("reads / kinds", v, f, e);
                uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, e, 0, 0, 0, 0};
                CtFormat back;
                if (!parse_format(h, &back) || back.lag() != lag || back.fold() != fold) return fail("parse_format", v, f, e);
            }

    const uint32_t lags[8][2] = {{1, 0}, {2, 0}, {1, 1}, {3, 1}, {16, 1}, {0, 0}, {17, 0}, {1, 2}};
    std::set<decltype(key(CtSettings()))> seen;
    std::vector<CtSettings> todo{CtSettings()};
    seen.insert(key(todo[0]));
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const CtSettings s = todo.back();
        todo.pop_back();
        // the state's own invariants
        if (s.lag_on() && !s.lag_fits()) return fail("the setting is on without its prerequisites", s.lag, s.fold, s.shuffle);
        if (s.lag < 1 || s.lag > 16 || s.fold > 1) return fail("the setting is out of range", s.lag, s.fold, 0);
        const CtFormat f = format_of(s);
        if (!format_legal(f)) return fail("format_of is not legal", f.version, f.flags, f.elem);
        if ((f.version == CT_VERSION_LAG) != s.lag_on() || f.lag() != s.lag || f.fold() != s.fold) return fail("format_of's lag", f.version, f.flags, f.elem);
        if (((s.reader() & CT_READS_LAG) != 0) != s.lag_on()) return fail("reader", s.reader(), s.lag, s.fold);
        CtSettings off = s;
        off.lag = 1; off.fold = 0;
        const CtFormat g = format_of(off);
        if (g.version >= CT_VERSION_LAG || (s.lag_on() && (g.version != CT_VERSION_AUTO || g.flags != CT_FLAG_DELTA || g.elem != f.elem)))
            return fail("format_of with the setting off", g.version, g.flags, g.elem);
        if (!s.lag_on() && (g.version != f.version || g.flags != f.flags || g.elem != f.elem)) return fail("format_of changed", g.version, g.flags, g.elem);
        // every call from here
        for (int k = 0; k < 10; k++) {
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
                default: ok = t.set_delta_lag(lags[i][0], lags[i][1]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (uint32_t)k, (uint32_t)i, 0);
                if (k == 9) {
                    const bool good = i < 5, plain = i == 0;
                    if (ok != (good && (plain || s.lag_fits()))) return fail("set_delta_lag's answer", lags[i][0], lags[i][1], s.shuffle);
                    if (ok && (t.lag != lags[i][0] || t.fold != lags[i][1])) return fail("set_delta_lag's effect", lags[i][0], lags[i][1], 0);
                } else if (ok && s.lag_on() && t.lag_fits() && (t.lag != s.lag || t.fold != s.fold)) {
                    return fail("a call that ends no prerequisite changed the setting", (uint32_t)k, vals[i], 0);
                }
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }
    printf("lag_format_check: ok, %u legal triples, %zu states, %llu calls\n", legal, seen.size(), calls);
    return 0;
}
