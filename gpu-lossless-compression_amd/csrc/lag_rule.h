// lag_rule.h -- the integer pieces of the lag rule (INTEGRATION.md 4b "Filter: auto with lag") that lag_probe.hip, the host side
// and the stand-alone checker tools/filter_lag_rule_check.cpp share: which lag of the lagged, folded delta (lag.hip) a segment
// wants at each element size, and the walk that weighs those three against the seven candidates of filter_rule.h, which stays as
// it is.  Plain C++: no GPU header needed.
//   A segment's first P = L - L % 8 bytes; x_e[i] its elements of e = 2, 4, 8 bytes; f_{e,l}[i] the folded delta at lag
//   l = 1 .. 16 with runs of 2048 elements, run heads included: d = x[i] where i % 2048 < l, else x[i] - x[i - l] (mod 2^W,
//   W = 8 e); f = (d << 1) ^ (0 - (d >> (W - 1))).  That is what glcLagDeltaShuffleDevice(e, l, fold = 1) builds its planes from.
//     sums     S[e][l] = sum_i bitlen(f_{e,l}[i]), bitlen(0) = 0, bitlen(v) = floor(log2 v) + 1: 48 sums of 64 bits in the row
//              layout (log2 e - 1) * 16 + (l - 1).  With P <= 2^31 a sum is below 2^36.
//     winners  win_e = the l with the smallest S[e][l], ties to the smallest l (all zero, so P = 0 as well: 1)
//     planes   E_e[j][v] = elements whose f_{e,win_e}[i] has byte j equal to v: 14 rows of 256 counts, E_2 first
//     costs    three: filter_plane_cost summed over the planes of E_2, of E_4 and of E_8
//   The walk is filter_rule.h's over ten candidates: its seven in their order, then (2, win_2, fold), (4, win_4, fold) and
//   (8, win_8, fold); candidate i replaces the pick exactly when 33 cost[i] < 32 cost[pick].  Only the folded form is offered:
//   the unfolded delta at lag 1 is candidate 2, 4 or 6 already.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "filter_rule.h"

namespace glc {

constexpr uint32_t LAG_MAX = 16;                              // lags 1 .. 16 (lag.hip's LG_MAX_LAG)
constexpr uint32_t LAG_SUMS = 3 * LAG_MAX;                    // sums per probed segment
constexpr uint32_t LAG_ROWS = 14;                             // histograms per probed segment: 2 + 4 + 8
constexpr uint32_t LAG_ELEMS = 3;                             // element sizes 2, 4, 8: index k is elem 2 << k
constexpr uint32_t LAG_CANDS = FILTER_CANDS + LAG_ELEMS;      // the candidates of the walk

GLC_ANS_HD inline uint32_t lag_bitlen(unsigned long long v)
{
    uint32_t n = 0;
    if (v >> 32) { n += 32; v >>= 32; }
    if (v >> 16) { n += 16; v >>= 16; }
    if (v >> 8) { n += 8; v >>= 8; }
    if (v >> 4) { n += 4; v >>= 4; }
    if (v >> 2) { n += 2; v >>= 2; }
    if (v >> 1) { n += 1; v >>= 1; }
    return n + (uint32_t)v;
}
// the fold of a difference d of W = 8 elem bits (d below 2^W): its sign into bit 0
GLC_ANS_HD inline unsigned long long lag_fold(unsigned long long d, uint32_t elem)
{
    const uint32_t W = 8 * elem;
    const unsigned long long mask = W == 64 ? ~0ull : (1ull << W) - 1;
    return ((d << 1) ^ (0ull - (d >> (W - 1)))) & mask;
}
// the row of S[elem][lag] among a segment's 48 sums, and the first row of E_elem among its 14 histograms
GLC_ANS_HD inline uint32_t lag_sum_row(uint32_t elem, uint32_t lag) { return (elem == 2 ? 0u : elem == 4 ? 1u : 2u) * LAG_MAX + (lag - 1); }
GLC_ANS_HD inline uint32_t lag_plane_row(uint32_t elem) { return elem == 2 ? 0u : elem == 4 ? 2u : 6u; }
// a lag word as the plane probe uses it: whatever the word holds, a lag of 1 .. 16
GLC_ANS_HD inline uint32_t lag_clamp(uint32_t v) { return ((v - 1) & (LAG_MAX - 1)) + 1; }
// the winner of one element size from its sixteen sums
GLC_ANS_HD inline uint32_t lag_argmin(const unsigned long long S[LAG_MAX])
{
    uint32_t w = 0;
    for (uint32_t l = 1; l < LAG_MAX; l++)
        if (S[l] < S[w]) w = l;
    return w + 1;
}

// the 48 sums of the first len - len % 8 bytes of x, serially: for the checker
inline void lag_sums(const uint8_t *x, size_t len, unsigned long long S[LAG_SUMS])
{
    const size_t P = len - len % 8;
    for (uint32_t k = 0; k < LAG_ELEMS; k++) {
        const uint32_t e = 2u << k;
        const unsigned long long mask = e == 8 ? ~0ull : (1ull << (8 * e)) - 1;
        auto at = [&](size_t i) { unsigned long long v = 0; for (uint32_t b = 0; b < e; b++) v |= (unsigned long long)x[i * e + b] << (8 * b); return v; };
        for (uint32_t l = 1; l <= LAG_MAX; l++) {
            unsigned long long s = 0;
            for (size_t i = 0; i < P / e; i++) {
                const unsigned long long d = i % FILTER_RUN < l ? at(i) : (at(i) - at(i - l)) & mask;
                s += lag_bitlen(lag_fold(d, e));
            }
            S[lag_sum_row(e, l)] = s;
        }
    }
}

// a candidate of the walk: elem, the delta flag, and for the last three the lag (the fold is on); lags[k] = win of elem 2 << k
struct LagCand { uint8_t elem, delta, lag, fold; };
GLC_ANS_HD inline LagCand lag_cand(uint32_t i, const uint32_t lags[LAG_ELEMS])
{
    if (i < FILTER_CANDS) { const FilterCand f = filter_cand(i); return LagCand{f.elem, f.delta, 1, 0}; }
    const uint32_t k = i - FILTER_CANDS;
    return LagCand{(uint8_t)(2u << k), 1, (uint8_t)lags[k], 1};
}
// the margin walk over the ten costs: filter_rule.h's seven, then the three of the lag planes
inline uint32_t lag_pick(const unsigned long long cost[LAG_CANDS])
{
    uint32_t pick = 0;
    for (uint32_t i = 1; i < LAG_CANDS; i++)
        if (FILTER_MARGIN_NUM * cost[i] < FILTER_MARGIN_DEN * cost[pick]) pick = i;
    return pick;
}

} // namespace glc
