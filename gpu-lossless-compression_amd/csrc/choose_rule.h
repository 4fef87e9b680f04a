// choose_rule.h -- the rule of the container's CHOOSE codec (INTEGRATION.md 4b "choose"): whether a block goes to the BWT codec or
// to the order-0 codec, from the collision statistic of the bigram probe (choose.hip).  Plain C++, shared by the host side and
// the stand-alone checker tools/choose_rule_check.cpp: no GPU header needed.
//   A segment x of L bytes; for 2 <= p < L, ctx(p) = (31 x[p-2] + x[p-1]) & 255 and sym(p) = x[p].  N[a][b] counts the p with
//   ctx = a and sym = b, M = L - 2 (0 below two bytes) is their number, R[a] and C[b] are the row and column sums, and
//   S2 = sum N (N - 1), SR = sum R (R - 1), SC = sum C (C - 1).  X = S2 M (M - 1) / (SR SC) is the observed number of colliding
//   (context, symbol) pairs over what independence of symbol and context would give: 1 for i.i.d. bytes at any length.
//   A block is BWT exactly when L >= CHOOSE_MIN_LEN, SR > 0, SC > 0 and CHOOSE_DEN S2 M (M - 1) >= CHOOSE_NUM SR SC.
// With L <= 2^20 every sum is below 2^40 and both sides of the comparison below 2^83: 128-bit integers, no rounding anywhere.
#pragma once
#include <stdint.h>

namespace glc {

constexpr uint32_t CHOOSE_MIN_LEN = 2048;                    // shorter blocks are order-0 whatever they hold
constexpr uint32_t CHOOSE_NUM = 3, CHOOSE_DEN = 2;           // the threshold on X
constexpr uint32_t CHOOSE_STATS = 4;                         // a stats row: {S2, SR, SC, M}

inline bool choose_bwt(unsigned long long L, unsigned long long S2, unsigned long long SR, unsigned long long SC, unsigned long long M)
{
    if (L < CHOOSE_MIN_LEN || SR == 0 || SC == 0 || M == 0) return false;
    typedef unsigned __int128 u128;
    return (u128)CHOOSE_DEN * S2 * M * (M - 1) >= (u128)CHOOSE_NUM * SR * SC;
}
inline bool choose_bwt(unsigned long long L, const unsigned long long s[CHOOSE_STATS]) { return choose_bwt(L, s[0], s[1], s[2], s[3]); }

} // namespace glc
