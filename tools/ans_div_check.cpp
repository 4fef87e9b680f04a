// ans_div_check.cpp -- a stand-alone host program around ans_div() (csrc/ans_coder.h), the multiply-high division of the rANS
// encoder's state update.  It is meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/ans_div_check.cpp -o ans_div_check \
//       && ./ans_div_check
// The encoder divides a renormalised state x < f * 2^20 by f = q[s], 1 <= f <= 4096.  For every f the program compares
// ans_div with plain division
//   1. at every multiple of f within 64 multiples of 0, of 2^16 (the states' lower bound), of f * 2^20 (the renormalised
//      range's end) and of 2^32, and one either side of each multiple;
//   2. at a few million random x in [0, f * 2^20) and over all 32 bits;
// and checks the whole encoder step ans_put against its definition floor(x / f) * 4096 + x mod f + c.
#include "../gpu-lossless-compression_amd/csrc/ans_coder.h"

#include <stdio.h>
#include <random>

using namespace glc;

static unsigned long long g_checked = 0;

static bool check(uint32_t f, const AnsDiv &d, uint64_t x64)
{
    if (x64 > 0xFFFFFFFFull) return true;
    const uint32_t x = (uint32_t)x64, got = ans_div(x, d.m, d.l);
    g_checked++;
    if (got == x / f) return true;
    printf("FAIL f=%u x=%u: %u, want %u\n", f, x, got, x / f);
    return false;
}

int main()
{
    std::mt19937_64 rng(20261019);
    const uint32_t per_f = 1200;                              // random x per f and range: 4096 * 2 * 1200 = 9.8 million
    for (uint32_t f = 1; f <= ANS_M; f++) {
        const AnsDiv d = ans_div_make(f);
        if (d.l > ANS_PROB_BITS || ans_l(ans_pack(f, ANS_M - 1, d.l)) != d.l || ans_f(ans_pack(f, ANS_M - 1, d.l)) != f ||
            ans_c(ans_pack(f, ANS_M - 1, d.l)) != ANS_M - 1) {
            printf("FAIL f=%u: the packed entry does not hold (f, c, l)\n", f);
            return 1;
        }
        const uint64_t top = (uint64_t)f << 20, ends[4] = {0, ANS_L, top, 1ull << 32};
        for (uint64_t e : ends) {
            const uint64_t k0 = e / f;
            for (uint64_t k = k0 > 64 ? k0 - 64 : 0; k <= k0 + 64; k++)
                for (int s = -1; s <= 1; s++) {
                    if (k * f == 0 && s < 0) continue;
                    if (!check(f, d, k * f + s)) return 1;
                }
        }
        for (uint32_t i = 0; i < per_f; i++)
            if (!check(f, d, rng() % top) || !check(f, d, rng() & 0xFFFFFFFFull)) return 1;
        for (uint32_t i = 0; i < 16; i++) {                    // the step itself, from a renormalised state
            const uint32_t x = (uint32_t)(ANS_L + rng() % (top - ANS_L)), c = (uint32_t)(rng() % ANS_M);
            const uint32_t want = (x / f) * ANS_M + x % f + c;
            if (ans_put(x, ans_pack(f, c, d.l), d.m) != want) { printf("FAIL ans_put f=%u x=%u c=%u\n", f, x, c); return 1; }
        }
    }
    printf("ans_div_check: ok, %llu divisions\n", g_checked);
    return 0;
}
