// auto_rule_check.cpp -- a stand-alone host program around csrc/auto_rule.h, the integer pieces of the auto mode's rule (format
// version 8).  It is meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/auto_rule_check.cpp -o auto_rule_check \
//       && ./auto_rule_check
// It prints
//   cost <q> <cost(q)>                                for every q from 1 to 4096, and
//   case <name> <bl> <wS> <wA> <pick5> <H[0]> ... <H[255]>
// for a fixed list of histograms H of blocks of bl bytes, each against several wS: wA - 1, wA, wA + 1 (the tie goes to candidate
// S) and the raw record's words.  tests/test_cpu_container_auto.py compares every line with tests/auto_model.py.
#include "../gpu-lossless-compression_amd/csrc/auto_rule.h"

#include <stdio.h>
#include <vector>

using namespace glc;

struct Case { const char *name; uint32_t bl; std::vector<uint32_t> H; };

static Case make(const char *name, uint32_t bl, std::vector<uint32_t> H)
{
    H.resize(256, 0u);
    return {name, bl, H};
}

// counts that sum to bl from a small generator: `present` symbols, geometrically falling
static Case falling(const char *name, uint32_t bl, uint32_t present, uint32_t seed)
{
    std::vector<uint32_t> H(256, 0u);
    uint32_t left = bl, x = seed;
    for (uint32_t k = 0; k < present && left; k++) {
        x = x * 1664525u + 1013904223u;
        const uint32_t s = (x >> 24) & 255u;
        const uint32_t take = k + 1 == present ? left : (left + 1) / 2;
        H[s] += take;
        left -= take;
    }
    H[0] += left;
    return {name, bl, H};
}

int main()
{
    for (uint32_t q = 1; q <= ANS_M; q++) printf("cost %u %u\n", q, auto_cost(q));
    std::vector<Case> cases;
    cases.push_back(make("one-symbol-2^20", 1u << 20, {1u << 20}));                       // H[s] = 2^20: the 64-bit product
    cases.push_back(make("all-256-even-2^20", 1u << 20, std::vector<uint32_t>(256, 4096u)));
    {
        std::vector<uint32_t> H(256, 1u);                                                  // all 256 present under one: the R < 0 path
        H[0] = 8192 - 255;
        cases.push_back(make("all-256-dominant", 8192, H));
        H.assign(256, 1u);
        H[200] = (1u << 20) - 255;
        cases.push_back(make("all-256-dominant-2^20", 1u << 20, H));
    }
    {
        std::vector<uint32_t> H(256, 0u);                                                  // scattered skew: 90 % zeros, 1 .. 15 even
        H[0] = 65536 - 15 * 437;
        for (uint32_t s = 1; s < 16; s++) H[s] = 437;
        cases.push_back(make("scattered", 65536, H));
    }
    cases.push_back(make("tie", 20, {10, 10}));
    cases.push_back(make("thirds", 3, {1, 1, 1}));
    cases.push_back(make("one-byte", 1, {0, 0, 0, 0, 0, 0, 0, 1}));
    cases.push_back(make("two-chunks-and-one", 65537, {65536, 1}));
    cases.push_back(falling("falling-70000", 70000, 40, 7u));
    cases.push_back(falling("falling-4099", 4099, 9, 99u));
    cases.push_back(falling("falling-2^20", 1u << 20, 200, 12345u));
    for (const Case &c : cases) {
        uint32_t q[256];
        auto_quantise(c.H.data(), c.bl, q);
        uint32_t sum = 0;
        for (uint32_t s = 0; s < 256; s++) {
            if ((q[s] == 0) != (c.H[s] == 0)) { printf("FAIL %s: q[%u] = %u for count %u\n", c.name, s, q[s], c.H[s]); return 1; }
            sum += q[s];
        }
        if (sum != ANS_M) { printf("FAIL %s: the q sum to %u\n", c.name, sum); return 1; }
        const unsigned long long wA = auto_words_a(auto_cost_sum(c.H.data(), q), c.bl);
        const unsigned long long wS[4] = {wA - 1, wA, wA + 1, (c.bl + 3ull) / 4};
        for (unsigned long long w : wS) {
            printf("case %s %u %llu %llu %d", c.name, c.bl, w, wA, auto_pick5(wA, w) ? 1 : 0);
            for (uint32_t s = 0; s < 256; s++) printf(" %u", c.H[s]);
            printf("\n");
        }
    }
    printf("auto_rule_check: ok, %zu histograms\n", cases.size());
    return 0;
}
