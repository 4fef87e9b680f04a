// class_rule_check.cpp -- a stand-alone host program around csrc/class_rule.h, the rule of the CHOOSE codec with filters, and the
// state walk of glcPlanSetContainerChooseFilters (CtSettings, csrc/container_internal.h).  It is meant to be built with the host
// sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/class_rule_check.cpp -o class_rule_check && ./class_rule_check
// It compares class_typed() and class_key() with the same walk done long-hand in 128-bit integers over an explicit candidate table --
// at equal costs, exactly on the margin (33 c = 32 p) and one step to either side, with GRID_NO_COST as the byte cost, at L = 2047
// and 2048, at every level, and over a pseudo-random sweep -- and walks the setters: a pseudo-random sequence of every public
// setter against a shadow of the one field, plus, at every level, reader(), kinds() and format_of() against the order-0 settings
// the level stands for.  It prints
//   case <name> <level> <L> <eight costs> <S2 SR SC M> <key>
// for the named cases (tests/test_cpu_choose_filters.py compares every line with tests/choose_filters_model.py).
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>

using namespace glc;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

static int failures = 0;
static unsigned long long checked = 0, states = 0;

// the walk long-hand: the candidates' element sizes spelled out, the margins in 128 bits
static uint32_t longhand_typed(uint32_t level, u64 L, const u64 c[8])
{
    static const uint32_t elem[7] = {1, 2, 2, 4, 4, 8, 8};
    if (level < 2 || L < 2048) return 0;
    uint32_t p = 0;
    for (uint32_t i = 1; i < 7; i++)
        if ((u128)33 * c[i] < (u128)32 * c[p]) p = i;
    if (level == 5) {
        const bool wins = p == 0 ? (u128)33 * c[7] < (u128)32 * c[0] : c[7] < c[p];
        if (wins) return 1;
    }
    return p ? elem[p] : 0;
}

static void check(const char *name, uint32_t level, u64 L, const u64 c[8], const u64 stats[4])
{
    const uint32_t got = class_key(level, L, c, stats), e = longhand_typed(level, L, c);
    const uint32_t want = e ? e : choose_bwt(L, stats) ? 0xFFu : 0u;
    checked++;
    if (name) {
        printf("case %s %u %llu", name, level, L);
        for (int i = 0; i < 8; i++) printf(" %llu", c[i]);
        for (int i = 0; i < 4; i++) printf(" %llu", stats[i]);
        printf(" %u\n", got);
    }
    if (got != want || class_typed(level, L, c) != e) {
        printf("FAIL %s: level %u L %llu gives %u, long-hand %u\n", name ? name : "sweep", level, L, got, want);
        failures++;
    }
}

// the order-0 settings a level stands for
static CtSettings order0_of(uint32_t level)
{
    CtSettings s;
    bool ok = s.set_codec(CT_CODEC_HUFF0) && s.set_mode(CT_MODE_AUTO, 1);
    if (level >= 2) ok = ok && s.set_filter_auto(1);
    if (level >= 3) ok = ok && s.set_filter_lag(1);
    if (level >= 4) ok = ok && s.set_filter_grid(1);
    if (level >= 5) ok = ok && s.set_filter_byte(1);
    if (!ok) { printf("FAIL: the order-0 settings of level %u are refused\n", level); failures++; }
    return s;
}

static void expect(bool ok, const char *what, uint32_t a = 0, uint32_t b = 0)
{
    states++;
    if (!ok) { printf("FAIL: %s (%u, %u)\n", what, a, b); failures++; }
}

int main()
{
    const u64 bwt[4] = {2046ull * 2045, 2046ull * 2045, 1023ull * 2045, 2046}, flat[4] = {0, 0, 0, 2046};     // X = 2; no collisions
    const u64 big = 1ull << 40;
    static_assert(CLASS_MAX_LEVEL == 5 && CLASS_COSTS == 8 && CLASS_BWT == 0xFF, "the constants the model has");
    for (uint32_t level = 0; level <= CLASS_MAX_LEVEL; level++) {
        const u64 equal[8] = {big, big, big, big, big, big, big, big};
        check("equal", level, 4096, equal, bwt);
        check("equal-flat", level, 4096, equal, flat);
        // candidate 4, (4, 1), exactly on the margin of candidate 0 and one step inside it; 33 * 2^35 = 32 * (33 * 2^30)
        const u64 p = 33ull << 30, on = 1ull << 35;
        const u64 on_margin[8] = {p, p, p, p, on, p, p, GRID_NO_COST}, inside[8] = {p, p, p, p, on - 1, p, p, GRID_NO_COST};
        check("on-margin", level, 4096, on_margin, bwt);
        check("inside-margin", level, 4096, inside, bwt);
        check("inside-margin-2047", level, 2047, inside, bwt);
        check("inside-margin-2048", level, 2048, inside, flat);
        // the byte candidate against a pick of one plane (the margin) and of two (the plain costs)
        const u64 byte_on[8] = {p, p, p, p, p, p, p, on}, byte_in[8] = {p, p, p, p, p, p, p, on - 1};
        check("byte-on-margin", level, 4096, byte_on, bwt);
        check("byte-inside-margin", level, 4096, byte_in, flat);
        const u64 two[8] = {p, p, on - 1, p, p, p, p, on - 1}, two_in[8] = {p, p, on - 1, p, p, p, p, on - 2};
        check("byte-equals-two-planes", level, 4096, two, bwt);
        check("byte-below-two-planes", level, 4096, two_in, bwt);
        const u64 top[8] = {1ull << 43, 1ull << 43, 1ull << 43, 1ull << 43, 1ull << 43, 1ull << 43, (1ull << 43) - (1ull << 39), GRID_NO_COST};
        check("top-costs", level, 1ull << 20, top, bwt);
    }
    u64 x = 0x9E3779B97F4A7C15ull;
    auto next = [&](u64 below) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % below; };
    for (int i = 0; i < 200000; i++) {
        u64 c[8];
        const u64 base = 1 + next(1ull << 43);
        for (int k = 0; k < 8; k++) c[k] = next(4) ? base - next(base / 16 + 1) : next(1ull << 43);     // mostly within a margin of each other
        if (next(8) == 0) c[7] = GRID_NO_COST;
        check(nullptr, (uint32_t)next(6), 2040 + next(16), c, next(2) ? bwt : flat);
    }

    // the versions
    const uint32_t versions[6] = {CT_VERSION_CODEC, CT_VERSION_AUTO, CT_VERSION_FILTER, CT_VERSION_FILTER_LAG, CT_VERSION_FILTER_GRID, CT_VERSION_FILTER_BYTE};
    for (uint32_t level = 0; level <= 5; level++) expect(class_version(level) == versions[level], "class_version", level, class_version(level));

    // the setting at every level against the order-0 settings it stands for
    for (uint32_t level = 0; level <= 5; level++) {
        CtSettings s;
        expect(!s.set_choose_filters(level), "refused under the BWT codec", level);
        expect(s.set_codec(CT_CODEC_HUFF0) && !s.set_choose_filters(level), "refused under the order-0 codec", level);
        expect(s.set_codec(CT_CODEC_CHOOSE) && s.set_choose_filters(level) && s.choose_filters == level, "accepted under CHOOSE", level);
        expect(!s.set_choose_filters(6) && !s.set_choose_filters(~0u) && s.choose_filters == level, "level 6 refused, nothing changed", level);
        expect(s.mode == CT_MODE_PLAIN && !s.filter_auto && !s.filter_lag && !s.filter_grid && !s.filter_byte && !s.shuffle && !s.delta, "the other fields untouched", level);
        expect(!s.set_mode(CT_MODE_AUTO, 1) && !s.set_mode(CT_MODE_SPARSE, 1) && !s.set_mode(CT_MODE_RUNS, 1) && !s.set_filter_auto(1) && !s.set_shuffle(4) &&
                   !s.set_byte_delta(1, 0) && s.choose_filters == level,
               "the refusals under CHOOSE stand", level);
        const CtFormat f = format_of(s);
        expect(f.version == versions[level] && f.flags == 0 && f.elem == 0 && f.width == 0, "format_of", level, f.version);
        if (level) {
            const CtSettings o = order0_of(level);
            const CtFormat fo = format_of(o);
            expect(s.reader() == o.reader(), "reader() is the order-0 plan's", s.reader(), o.reader());
            expect(fo.version == f.version && fo.flags == f.flags && fo.elem == f.elem, "the order-0 plan writes the same triple", level);
            expect(s.kinds() == 0x2Fu && (f.kinds() & s.kinds()) == s.kinds(), "kinds 0, 1, 2, 3 and 5", s.kinds());
        } else {
            expect(s.reader() == 0 && s.kinds() == 0x07u, "level 0 is CHOOSE as it is", s.reader(), s.kinds());
        }
        expect(s.set_codec(CT_CODEC_CHOOSE) && s.choose_filters == 0, "CHOOSE again puts it back to 0", level);
        expect(s.set_choose_filters(level) && s.set_codec(CT_CODEC_BWT) && s.choose_filters == 0 && s.reader() == 0, "another codec puts it back to 0", level);
    }

    // a pseudo-random walk over every setter against a shadow of the field
    {
        CtSettings s;
        uint32_t shadow = 0;
        const uint32_t codecs[5] = {CT_CODEC_BWT, CT_CODEC_HUFF0, CT_CODEC_CHOOSE, 2, 3};
        const CtMode modes[5] = {CT_MODE_SPARSE, CT_MODE_RUNS, CT_MODE_ANS, CT_MODE_AUTO, CT_MODE_DEDUP};
        for (int i = 0; i < 100000; i++) {
            const uint32_t was_codec = s.codec;
            switch (next(12)) {
            case 0: { const uint32_t c = codecs[next(5)]; if (s.set_codec(c)) shadow = 0; else expect(s.codec == was_codec, "a refused codec changes nothing"); break; }
            case 1: case 2: case 3: {
                const uint32_t l = (uint32_t)next(8);
                const bool ok = s.set_choose_filters(l);
                expect(ok == (s.codec == CT_CODEC_CHOOSE && l <= 5), "set_choose_filters' rule", l, s.codec);
                if (ok) shadow = l;
                break;
            }
            case 4: s.set_mode(modes[next(5)], (uint32_t)next(2)); break;
            case 5: s.set_shuffle((uint32_t)next(10)); break;
            case 6: s.set_delta((uint32_t)next(2)); break;
            case 7: s.set_filter_auto((uint32_t)next(2)); break;
            case 8: s.set_filter_lag((uint32_t)next(2)); s.set_filter_grid((uint32_t)next(2)); s.set_filter_byte((uint32_t)next(2)); break;
            case 9: s.set_delta_lag(1 + (uint32_t)next(16), (uint32_t)next(2)); break;
            case 10: s.set_delta_grid((uint32_t)next(3) * 320, (uint32_t)next(2)); break;
            default: s.set_byte_delta((uint32_t)next(4), (uint32_t)next(2) * 640); break;
            }
            expect(s.choose_filters == shadow && (shadow == 0 || s.codec == CT_CODEC_CHOOSE), "the field follows its shadow", s.choose_filters, shadow);
            if (s.codec == CT_CODEC_CHOOSE)
                expect(s.mode == CT_MODE_PLAIN && !s.shuffle && !s.filter_auto && !s.byte_on() && !s.lag_on() && !s.grid_on(), "CHOOSE keeps every mode and filter off");
        }
    }
    if (failures) return 1;
    printf("class_rule_check: ok, %llu keys, %llu states\n", checked, states);
    return 0;
}
