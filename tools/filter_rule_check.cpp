// filter_rule_check.cpp -- a stand-alone host program around csrc/filter_rule.h, the rule that picks a frame's byte-plane filter
// from the filter probe's histograms.  It is meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/filter_rule_check.cpp -o filter_rule_check \
//       && ./filter_rule_check [rows.bin]
// It compares filter_plane_cost() and filter_pick() -- 64-bit integers -- with the same sums and the same comparison in 128-bit
// arithmetic: on pseudo-random counts and at the extremes (one symbol holding 2^31, all 256 symbols equal, N = 0, one count of 1
// beside 2^31 - 1, costs next to the margin and at the top of their range); it checks the plane list against the candidates, and
// prints
//   plane <name> <cost>
// for the named planes.  With a file of k * 22 * 256 little-endian 32-bit counts (k probed segments) it also prints, per segment,
//   costs <c0> ... <c6> pick <i>
// (tests/test_cpu_filter_rule.py compares every line with tests/filter_auto_model.py).
#include "../gpu-lossless-compression_amd/csrc/filter_rule.h"

#include <stdio.h>
#include <vector>

using namespace glc;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

static int failures = 0;

static u128 wide_plane_cost(const uint32_t H[256])
{
    u128 N = 0, sum = 0;
    for (int s = 0; s < 256; s++) N += H[s];
    for (int s = 0; s < 256; s++) {
        if (!H[s]) continue;
        u128 q = (u128)H[s] * 4096 / N;
        if (q < 1) q = 1;
        if (q > 4096) q = 4096;
        sum += (u128)H[s] * AUTO_COST.v[(size_t)q];
    }
    return sum;
}

static void check_plane(const char *name, const uint32_t H[256])
{
    const u64 got = filter_plane_cost(H);
    const u128 want = wide_plane_cost(H);
    if (name) printf("plane %s %llu\n", name, got);
    if ((u128)got != want || (want >> 43) != 0) { printf("FAIL plane %s: %llu\n", name ? name : "sweep", got); failures++; }
}

static uint32_t wide_pick(const u64 c[FILTER_CANDS])
{
    uint32_t pick = 0;
    for (uint32_t i = 1; i < FILTER_CANDS; i++)
        if ((u128)33 * c[i] < (u128)32 * c[pick]) pick = i;
    return pick;
}

static void check_pick(const u64 c[FILTER_CANDS])
{
    if (filter_pick(c) != wide_pick(c)) { printf("FAIL pick: %llu %llu %llu %llu %llu %llu %llu\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6]); failures++; }
}

int main(int argc, char **argv)
{
    // the plane list: every candidate's planes are its elem, in order, and the plain candidates' rows cover A_0..7 once each
    {
        uint32_t next = 0;
        for (uint32_t c = 0; c < FILTER_CANDS; c++) {
            const FilterCand f = filter_cand(c);
            uint32_t seen = 0;
            if (filter_first_plane(c) != next) { printf("FAIL first plane of candidate %u\n", c); failures++; }
            for (uint32_t j = 0; j < f.elem; j++, next++) {
                const FilterPlane p = filter_plane(next);
                bool ok = p.cand == c;
                if (f.delta) ok = ok && p.count == 1 && p.first == filter_delta_row(f.elem) + j && p.first + 1 <= FILTER_ROWS;
                else {
                    ok = ok && p.first == j && p.step == f.elem && p.count * f.elem == 8;
                    for (uint32_t k = 0; k < p.count; k++) seen |= 1u << (p.first + k * p.step);
                }
                if (!ok) { printf("FAIL plane %u\n", next); failures++; }
            }
            if (!f.delta && seen != 0xFFu) { printf("FAIL rows of candidate %u\n", c); failures++; }
        }
        if (next != FILTER_PLANES || filter_first_plane(FILTER_CANDS) != FILTER_PLANES) { printf("FAIL plane count\n"); failures++; }
    }
    uint32_t H[256];
    const uint32_t top = 1u << 31;
    for (int s = 0; s < 256; s++) H[s] = 0;
    check_plane("empty", H);
    H[77] = top;
    check_plane("one-symbol-2^31", H);
    H[77] = 1;
    check_plane("one-byte", H);
    H[77] = top - 1; H[200] = 1;
    check_plane("one-beside-2^31-1", H);
    for (int s = 0; s < 256; s++) H[s] = top / 256;
    check_plane("all-equal-2^31", H);
    for (int s = 0; s < 256; s++) H[s] = 1;
    check_plane("all-equal-256", H);
    for (int s = 0; s < 256; s++) H[s] = s < 255 ? 1u : top - 255;
    check_plane("255-rare", H);
    for (int s = 0; s < 256; s++) H[s] = s < 2 ? top / 2 : 0u;
    check_plane("two-halves", H);
    u64 x = 0x9E3779B97F4A7C15ull;
    auto next = [&](u64 below) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % below; };
    for (int i = 0; i < 20000; i++) {
        // counts that sum to at most 2^31: a budget shared out in random, sometimes tiny, sometimes huge shares
        u64 left = 1 + next(top);
        const uint32_t used = 1 + (uint32_t)next(256);
        for (int s = 0; s < 256; s++) H[s] = 0;
        for (uint32_t k = 0; k < used && left; k++) {
            const u64 share = next(4) == 0 ? left : 1 + next((left >> next(20)) + 1);
            const u64 take = share > left ? left : share;
            H[next(256)] += (uint32_t)take;
            left -= take;
        }
        check_plane(nullptr, H);
    }
    // the walk: at the margin, one step to either side, at the top of the range, and a sweep
    {
        const u64 big = (u64)top * 3072;                                            // the largest cost there is
        u64 c[FILTER_CANDS] = {33 * 1000, 32 * 1000, 32 * 1000 - 1, 0, 0, 0, 0};
        for (int i = 3; i < 7; i++) c[i] = ~0ull >> 21;
        check_pick(c);
        if (filter_pick(c) != 2) { printf("FAIL the margin is strict\n"); failures++; }
        u64 d[FILTER_CANDS] = {big, big, big, big, big, big, big};
        check_pick(d);
        if (filter_pick(d) != 0) { printf("FAIL equal costs keep no filter\n"); failures++; }
        d[6] = big / 33 * 32 - 33;
        check_pick(d);
        u64 z[FILTER_CANDS] = {0, 0, 0, 0, 0, 0, 0};
        check_pick(z);
        if (filter_pick(z) != 0) { printf("FAIL zero costs keep no filter\n"); failures++; }
        for (int i = 0; i < 200000; i++) {
            u64 r[FILTER_CANDS];
            const u64 base = 1 + next(big);
            for (uint32_t k = 0; k < FILTER_CANDS; k++) r[k] = next(3) ? base - next(base / 16 + 1) : next(big + 1);
            check_pick(r);
        }
    }
    if (argc > 1) {
        FILE *f = fopen(argv[1], "rb");
        if (!f) { printf("FAIL cannot open %s\n", argv[1]); return 1; }
        std::vector<uint32_t> rows((size_t)FILTER_ROWS * 256);
        while (fread(rows.data(), 4, rows.size(), f) == rows.size()) {
            u64 c[FILTER_CANDS];
            filter_costs(rows.data(), c);
            printf("costs %llu %llu %llu %llu %llu %llu %llu pick %u\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], filter_pick(c));
            check_pick(c);
        }
        fclose(f);
    }
    if (failures) return 1;
    printf("filter_rule_check: ok\n");
    return 0;
}
