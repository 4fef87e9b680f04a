// choose_rule_check.cpp -- a stand-alone host program around csrc/choose_rule.h, the rule of the container's CHOOSE codec.  It is
// meant to be built with the host sanitizers and run on the CPU; it touches no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/choose_rule_check.cpp -o choose_rule_check \
//       && ./choose_rule_check
// It compares choose_bwt() -- one 128-bit comparison -- with the same comparison done long-hand on 32-bit limbs, at the extremes
// of what the bigram probe can give (S2 = SR = SC near 2^40 at M = 2^20 - 2), at zero, exactly on the threshold and one step to
// either side of it, and over a pseudo-random sweep; it prints
//   case <name> <L> <S2> <SR> <SC> <M> <bwt>
// for the named cases (tests/test_cpu_container_choose.py compares every line with tests/choose_model.py).
#include "../gpu-lossless-compression_amd/csrc/choose_rule.h"

#include <stdio.h>
#include <vector>

using namespace glc;
typedef unsigned long long u64;

// a non-negative integer as 32-bit limbs, least significant first
struct Big {
    std::vector<uint32_t> d;
    explicit Big(u64 v) { d.push_back((uint32_t)v); d.push_back((uint32_t)(v >> 32)); }
    Big &mul(u64 v)                                            // schoolbook, one 32-bit half of v at a time
    {
        std::vector<uint32_t> r(d.size() + 2, 0u);
        const uint32_t h[2] = {(uint32_t)v, (uint32_t)(v >> 32)};
        for (size_t j = 0; j < 2; j++) {
            u64 carry = 0;
            for (size_t i = 0; i < d.size(); i++) {
                const u64 t = (u64)d[i] * h[j] + r[i + j] + carry;
                r[i + j] = (uint32_t)t;
                carry = t >> 32;
            }
            for (size_t i = d.size() + j; carry; i++) {
                const u64 t = (u64)r[i] + carry;
                r[i] = (uint32_t)t;
                carry = t >> 32;
            }
        }
        d = r;
        return *this;
    }
    bool ge(const Big &o) const
    {
        const size_t n = d.size() > o.d.size() ? d.size() : o.d.size();
        for (size_t i = n; i-- > 0;) {
            const uint32_t a = i < d.size() ? d[i] : 0u, b = i < o.d.size() ? o.d[i] : 0u;
            if (a != b) return a > b;
        }
        return true;
    }
};

static bool longhand(u64 L, u64 S2, u64 SR, u64 SC, u64 M)
{
    if (L < CHOOSE_MIN_LEN || SR == 0 || SC == 0 || M == 0) return false;
    return Big(CHOOSE_DEN).mul(S2).mul(M).mul(M - 1).ge(Big(CHOOSE_NUM).mul(SR).mul(SC));
}

static int failures = 0;
static void check(const char *name, u64 L, u64 S2, u64 SR, u64 SC, u64 M)
{
    const bool got = choose_bwt(L, S2, SR, SC, M), want = longhand(L, S2, SR, SC, M);
    if (name) printf("case %s %llu %llu %llu %llu %llu %d\n", name, L, S2, SR, SC, M, got ? 1 : 0);
    if (got != want) { printf("FAIL %s: %llu %llu %llu %llu %llu gives %d, long-hand %d\n", name ? name : "sweep", L, S2, SR, SC, M, got, want); failures++; }
}

int main()
{
    const u64 Lmax = 1ull << 20, Mmax = Lmax - 2, top = Mmax * (Mmax - 1);     // one cell holds every position: S2 = SR = SC = top
    check("one-value-2^20", Lmax, top, top, top, Mmax);
    check("top-s2-small-den", Lmax, top, 1, 1, Mmax);
    check("small-s2-top-den", Lmax, 1, top, top, Mmax);
    check("zero-s2", Lmax, 0, top, top, Mmax);
    check("all-zero", 0, 0, 0, 0, 0);
    check("all-zero-long", Lmax, 0, 0, 0, Mmax);
    check("sr-zero", 4096, 10, 0, 10, 4094);
    check("sc-zero", 4096, 10, 10, 0, 4094);
    check("short-2047", 2047, 2045ull * 2044, 2045ull * 2044, 2045ull * 1022, 2045);   // X = 2, one byte too short
    check("min-2048", 2048, 2046ull * 2045, 2046ull * 2045, 1023ull * 2045, 2046);     // X = 2
    // exactly on the threshold: 2 S2 M (M - 1) = 3 SR SC with M (M - 1) = 3 k and SR SC = 2 k S2
    {
        const u64 M = 4096, mm = M * (M - 1);                                   // 4096 * 4095 = 3 * 5591040
        const u64 S2 = 1000, SR = 2 * S2, SC = mm / 3;
        check("on-threshold", M + 2, S2, SR, SC, M);
        check("above-threshold", M + 2, S2 + 1, SR, SC, M);
        check("below-threshold", M + 2, S2, SR, SC + 1, M);
    }
    {
        const u64 SR = top, SC = 2 * Mmax, S2 = 3 * Mmax;                       // 2 S2 M (M - 1) = 6 M top = 3 SR SC, near 2^82
        check("on-threshold-2^20", Lmax, S2, SR, SC, Mmax);
        check("above-threshold-2^20", Lmax, S2 + 1, SR, SC, Mmax);
        check("below-threshold-2^20", Lmax, S2 - 1, SR, SC, Mmax);
    }
    u64 x = 0x9E3779B97F4A7C15ull;
    auto next = [&](u64 below) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % below; };
    for (int i = 0; i < 200000; i++) {
        const u64 M = 1 + next(Mmax), cap = M * (M - 1) + 1;
        check(nullptr, M + 2, next(cap), next(cap), next(cap), M);
    }
    if (failures) return 1;
    printf("choose_rule_check: ok\n");
    return 0;
}
