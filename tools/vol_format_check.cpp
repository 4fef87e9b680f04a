// vol_format_check.cpp -- a stand-alone host program around the stream-header rule, the slab arithmetic and the setters of
// csrc/container_internal.h as format version 17 (the 3-D predictor; INTEGRATION.md 4b "Delta: volume") left them.  It is meant to
// be built with the host sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/vol_format_check.cpp -o vol_format_check && ./vol_format_check
// Part 1, the header rule by brute force: check_stream_header() over versions 0 to 19, a set of flag words (every word below 32,
// and the legal ones with one further bit each), a set of words 3 (every elem <= 9 at the widths' edges) and a set of words 7 (0,
// the planes' edges around each width and around 2^24), with word 6 made good the old way (CRC of words 0..5) and the new way
// (words 0..5 followed by word 7), against the rule stated outright: version 17's family under the new CRC, and for every other
// version parse_frame_filter_format()'s answer with word 7 at 0 under the old CRC.  (That answer is the library's own: what it
// says of versions 1 to 16 is pinned by the earlier checkers -- grid_format_check.cpp up to 12, filter_lag_rule_check.cpp,
// filter_grid_rule_check.cpp, byte_format_check.cpp and filter_byte_rule_check.cpp beyond -- and the test holds versions up to 12
// against the models once more; what this program adds for them is that word 7 and the CRC rule stay as they were.)  It prints one line
// "legal <version> <flags> <word 3> <word 7>" per accepted header for tests/test_cpu_container_vol.py to hold against the model.
// Part 2, the slab: ct_vol_slab() against Q = P ceil(16 S / P) counted in 64 bits, over every width with the planes at their
// edges and over every plane step 4099 at a set of widths: a multiple of P and of 2048, 16 S <= Q < 16 S + P, Q <= 2^28 + 2^21,
// exact at S = 2^24 with W = 65536; and the range rounding lo - lo % Q over elements up to 2^40: a multiple of Q, at most lo,
// less than Q below it.
// Part 3 walks every state the setters reach from the default (each setter with in-range, boundary and out-of-range values, the
// grid setter with (0,0) (20,1) (300,0) (65536,1) (1,0), the volume setter with 0, 21, 300, 301, 65537, 2^24 and the bad 2^24 + 1,
// 20 and 1) and wants in every state: the volume is off unless the grid is on at a width below it; format_of() passes
// check_stream_header() once packed, is version 17 exactly when the volume is on and then says its plane, and is what it is
// without the setting when it is off; reader() has version 17's bit exactly when it is on, then with version 12's; a refused call
// changes nothing; the grid setter refuses a width >= plane while it is on and switches it off with the grid; a change among
// elem 2, 4 and 8 keeps it.  It prints
//   vol_format_check: ok, <legal> legal, <slabs> slabs, <states> states, <calls> calls
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>
#include <set>
#include <tuple>
#include <vector>

using namespace glc;

static const CrcTables T = crc_make_tables();

static int fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    printf("vol_format_check: FAILED %s at (%llu, %llu, %llu)\n", what, a, b, c);
    return 1;
}

// version 17's rule over the header's words, stated outright
static bool want17(uint32_t f, uint32_t w3, uint32_t w7)
{
    const uint32_t e = w3 & 255, w = w3 >> 8;
    return (f == 13 || f == 15) && (e == 2 || e == 4 || e == 8) && w >= 2 && w <= 65536 && w7 > w && w7 <= (1u << 24);
}

static unsigned long long legal = 0;

static int one(uint32_t v, uint32_t f, uint32_t w3, uint32_t w7)
{
    for (int newcrc = 0; newcrc <= 1; newcrc++) {
        uint32_t h[8] = {CT_MAGIC_STREAM, v | f << 16, 4096, w3, 12345, 0, 0, w7};
        const uint32_t t[7] = {h[0], h[1], h[2], h[3], h[4], h[5], h[7]};
        h[6] = newcrc ? crc32_bytes(T, t, 28) : crc32_bytes(T, h, 24);
        CtFormat fmt, old;
        uint32_t bl = 0;
        unsigned long long total = 0;
        const bool ok = check_stream_header(T, h, &fmt, &bl, &total);
        const bool want = v == 17 ? newcrc && want17(f, w3, w7) : !newcrc && w7 == 0 && parse_frame_filter_format(h, &old);
        if (ok != want) return fail(newcrc ? "check_stream_header under the new CRC" : "check_stream_header under the old CRC", v, f, ((unsigned long long)w7 << 32) | w3);
        if (!ok) continue;
        legal++;
        printf("legal %u %u %u %u\n", v, f, w3, w7);
        if (bl != 4096 || total != 12345) return fail("block_len / total", v, f, w3);
        if (v == 17) {
            if (!fmt.vol() || fmt.grid() || fmt.elem != (w3 & 255) || fmt.width != w3 >> 8 || fmt.plane != w7 || fmt.fold() != (f >> 1 & 1) || fmt.lag() != 1 ||
                fmt.reads() != CT_READS_VOL || fmt.kinds() != ct_kinds(8) || !fmt.delta() || fmt.word3() != w3 || fmt.frame_filters())
                return fail("version 17's fields", v, f, w3);
        } else if (fmt.vol() || fmt.plane || fmt.reads() == CT_READS_VOL || fmt.version != old.version || fmt.flags != old.flags || fmt.elem != old.elem || fmt.width != old.width) {
            return fail("another version's fields", v, f, w3);
        }
    }
    return 0;
}

static auto key(const CtSettings &s)
{
    return std::make_tuple(s.shuffle, s.delta, s.codec, (uint32_t)s.mode, s.filter_auto, s.lag, s.fold, s.grid_width, s.grid_fold, s.vol_plane);
}

int main()
{
    // part 1
    std::vector<uint32_t> flags;
    for (uint32_t f = 0; f < 32; f++) flags.push_back(f);
    for (uint32_t b = 5; b < 16; b++) { flags.push_back(13 | 1u << b); flags.push_back(15 | 1u << b); }
    std::vector<uint32_t> w3s, w7s = {0, 1, 2, 3, 20, 21, 300, 65536, 65537, 65538, (1u << 24) - 1, 1u << 24, (1u << 24) + 1, 1u << 31, ~0u};
    for (uint32_t e = 0; e <= 9; e++)
        for (uint32_t w : {0u, 1u, 2u, 20u, 65535u, 65536u, 65537u, 1u << 20}) w3s.push_back(e | w << 8);
    for (uint32_t v = 0; v <= 19; v++)
        for (uint32_t f : flags)
            for (uint32_t w3 : w3s)
                for (uint32_t w7 : w7s)
                    if (one(v, f, w3, w7)) return 1;

    // part 2
    unsigned long long slabs = 0;
    auto slab_ok = [&](uint32_t W, uint32_t S) {
        const unsigned long long P = 2048ull * ((W + 63ull) / 64ull), Q = P * ((16ull * S + P - 1) / P), got = ct_vol_slab(W, S);
        slabs++;
        return ct_vol_plane_ok(W, S) && got == Q && Q % P == 0 && Q % 2048 == 0 && Q >= 16ull * S && Q < 16ull * S + P && Q <= (1ull << 28) + (1ull << 21) && P == ct_grid_period(W);
    };
    for (uint32_t W = CT_GRID_MIN_WIDTH; W <= CT_GRID_MAX_WIDTH; W++)
        for (uint32_t S : {W + 1, W + 2, 2 * W, 7 * W + 3, 131072u, (1u << 24) - 1, 1u << 24})
            if (S > W && !slab_ok(W, S)) return fail("the slab", W, S, ct_vol_slab(W, S));
    for (uint32_t W : {2u, 64u, 65u, 1000u, 4096u, 65472u, 65473u, 65536u})
        for (uint32_t S = W + 1; S <= 1u << 24; S += 4099)
            if (!slab_ok(W, S)) return fail("the slab", W, S, ct_vol_slab(W, S));
    if (ct_vol_slab(65536, 1u << 24) != 1u << 28 || ct_vol_slab(65536, (1u << 24) - 1) != 1u << 28 || ct_vol_slab(20, 300) != 6144 || ct_vol_slab(2, 3) != 2048)
        return fail("the slab at the limits", ct_vol_slab(65536, 1u << 24), ct_vol_slab(20, 300), ct_vol_slab(2, 3));
    if (ct_vol_plane_ok(20, 20) || ct_vol_plane_ok(20, 0) || ct_vol_plane_ok(20, (1u << 24) + 1) || ct_vol_plane_ok(65536, 65536) || !ct_vol_plane_ok(65536, 65537) || ct_vol_plane_ok(2, ~0u))
        return fail("the plane range", 0, 0, 0);
    for (uint32_t W : {2u, 20u, 1000u, 65536u})
        for (uint32_t S : {W + 1, 7 * W + 3, 1u << 24}) {
            const unsigned long long Q = ct_vol_slab(W, S);
            for (unsigned long long lo : {0ull, 1ull, Q - 1, Q, Q + 1, 3 * Q - 1, (1ull << 32) - 1, 1ull << 32, (1ull << 40) + 12345}) {
                const unsigned long long i0 = lo - lo % Q;     // (needed_blocks() of container_api.cpp)
                if (i0 > lo || i0 % Q || lo - i0 >= Q) return fail("the range rounding", W, S, lo);
            }
        }

    // part 3
    const uint32_t grids[5][2] = {{0, 0}, {20, 1}, {300, 0}, {65536, 1}, {1, 0}};
    const uint32_t planes[9] = {0, 21, 300, 301, 65537, 1u << 24, (1u << 24) + 1, 20, 1};
    std::set<decltype(key(CtSettings()))> seen;
    std::vector<CtSettings> todo{CtSettings()};
    seen.insert(key(todo[0]));
    unsigned long long calls = 0;
    while (!todo.empty()) {
        const CtSettings s = todo.back();
        todo.pop_back();
        if (s.vol_on() && (!s.grid_on() || !s.lag_fits() || s.lag_on() || !ct_vol_plane_ok(s.grid_width, s.vol_plane)))
            return fail("the volume is on without its prerequisites", s.vol_plane, s.grid_width, s.shuffle);
        const CtFormat f = format_of(s);
        uint32_t h[8] = {CT_MAGIC_STREAM, f.version | f.flags << 16, 4096, f.word3(), 0, 0, 0, f.plane}, bl = 0;
        h[6] = ct_header_crc(h, [&](const uint32_t *w, size_t n) { return crc32_bytes(T, w, n); });
        CtFormat back;
        unsigned long long total = 0;
        if (!check_stream_header(T, h, &back, &bl, &total)) return fail("format_of does not pass the header check", f.version, f.flags, f.word3());
        if (back.version != f.version || back.flags != f.flags || back.elem != f.elem || back.width != f.width || back.plane != f.plane)
            return fail("the header does not give format_of back", f.version, f.flags, f.word3());
        if (f.vol() != s.vol_on() || f.plane != s.vol_plane || (s.vol_on() && (f.width != s.grid_width || f.fold() != s.grid_fold || f.elem != s.shuffle)))
            return fail("format_of's volume", f.version, f.flags, f.plane);
        if (((s.reader() & CT_READS_VOL) != 0) != s.vol_on() || (s.vol_on() && !(s.reader() & CT_READS_GRID)) || (s.vol_on() && (s.reader() & CT_READS_LAG)))
            return fail("reader", s.reader(), s.vol_plane, s.grid_width);
        if (s.vol_on()) {
            CtSettings off = s;
            off.vol_plane = 0;
            const CtFormat g = format_of(off);
            if (g.version != CT_VERSION_GRID || g.flags != (f.flags & ~CT_FLAG_VOL) || g.word3() != f.word3() || g.plane) return fail("format_of with the volume off", g.version, g.flags, g.elem);
        }
        for (int k = 0; k < 12; k++) {
            const uint32_t vals[8] = {0, 1, 2, 3, 4, 8, 9, 1u << 31};
            for (int i = 0; i < (k == 9 ? 2 : k == 10 ? 5 : k == 11 ? 9 : 8); i++) {
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
                case 9: ok = i == 0 ? t.set_delta_lag(1, 0) : t.set_delta_lag(3, 1); break;
                case 10: ok = t.set_delta_grid(grids[i][0], grids[i][1]); break;
                default: ok = t.set_delta_volume(planes[i]); break;
                }
                calls++;
                if (!ok && key(t) != key(s)) return fail("a refused call changed the settings", (uint32_t)k, (uint32_t)i, 0);
                if (k == 11) {
                    const uint32_t p = planes[i];
                    if (ok != (p == 0 || (s.grid_on() && p > s.grid_width && p <= (1u << 24)))) return fail("set_delta_volume's answer", p, s.grid_width, 0);
                    if (ok && (t.vol_plane != p || t.grid_width != s.grid_width || t.grid_fold != s.grid_fold)) return fail("set_delta_volume's effect", p, 0, 0);
                } else if (k == 10 && s.vol_on()) {
                    const uint32_t w = grids[i][0];
                    if (ok != (w == 0 || (w >= 2 && w < s.vol_plane))) return fail("set_delta_grid while the volume is on", w, s.vol_plane, 0);
                    if (ok && t.vol_plane != (w ? s.vol_plane : 0u)) return fail("set_delta_grid's effect on the volume", w, s.vol_plane, t.vol_plane);
                } else if (k == 9 && s.vol_on()) {
                    if (ok != (i == 0) || t.vol_plane != s.vol_plane) return fail("set_delta_lag while the volume is on", (uint32_t)i, 0, 0);
                } else if (ok && s.vol_on() && t.grid_on() && t.vol_plane != s.vol_plane) {
                    return fail("a call that keeps the grid changed the volume", (uint32_t)k, vals[i], 0);
                } else if (ok && !t.grid_on() && t.vol_on()) {
                    return fail("a call that ends the grid kept the volume", (uint32_t)k, vals[i], 0);
                }
                if (k == 0 && s.vol_on() && (vals[i] == 2 || vals[i] == 4 || vals[i] == 8) && (!ok || t.vol_plane != s.vol_plane))
                    return fail("a change of elem lost the volume", vals[i], s.vol_plane, 0);
                if (seen.insert(key(t)).second) todo.push_back(t);
            }
        }
    }
    printf("vol_format_check: ok, %llu legal, %llu slabs, %zu states, %llu calls\n", legal, slabs, seen.size(), calls);
    return 0;
}
