// grid_rule.h -- the integer pieces of the grid rule (INTEGRATION.md 4b "Filter: auto with grid") that grid_probe.hip, the host
// side and the stand-alone checker tools/filter_grid_rule_check.cpp share: which row width of the 2-D predictor (grid.hip) a
// segment wants at each element size, and the walk that weighs those three against the ten candidates of lag_rule.h, which stays
// as it is.  Plain C++: no GPU header needed.
//   A segment's first P = L - L % 8 bytes; x_e[i] its N = P / e elements of e = 2, 4, 8 bytes.  N < 1024: no candidate, width 0.
//   Else Wmax = min(65536, N / 2) and 32 tiles of 256 target elements at b_t = Wmax + floor(t (N - Wmax - 256) / 31), t = 0 .. 31
//   (on short segments tiles overlap; every target has its element Wmax back inside the segment).
//     sums     S_e[W] = sum over t, j < 256 of bitlen(fold(x_e[b_t + j] - x_e[b_t + j - W] mod 2^(8 e))) for W = 2 .. Wmax, with
//              lag_rule.h's fold and bitlen: the vertical difference alone, no bands, no run heads.  At most 8192 * 64 < 2^20.
//              A segment's row is 3 * 65537 words of 32 bits, S_e[W] at k * 65537 + W (k = log2 e - 1), 0xFFFFFFFF where W < 2
//              or W > Wmax.
//     winners  w_e = the W with the smallest S_e[W], ties to the smallest W; 0 where there is no candidate
//     planes   for every e with w_e != 0 the e byte planes of what glcGridDeltaShuffleDevice(e, w_e, fold = 1) builds from the
//              counted bytes (bands of 2048 ceil(w / 64) elements and run heads included): 14 rows of 256 counts in
//              lag_plane_row's layout; the rows of an e with w_e = 0 are zero
//     costs    three: filter_plane_cost summed over the planes of e; GRID_NO_COST where w_e = 0
//   The walk is lag_rule.h's over thirteen candidates: its ten in their order, then (2, w_2), (4, w_4) and (8, w_8), each the
//   grid filter with the fold; candidate i replaces the pick exactly when 33 cost[i] < 32 cost[pick].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "lag_rule.h"

namespace glc {

constexpr uint32_t GRID_MIN_ELEMS = 1024;                     // a segment with fewer elements has no grid candidate
constexpr uint32_t GRID_W_MIN = 2, GRID_W_MAX = 65536;        // grid.hip's widths
constexpr uint32_t GRID_TILES = 32, GRID_TILE = 256;          // the sample: 8192 targets per width
constexpr uint32_t GRID_SUM_ROW = GRID_W_MAX + 1;             // words of S_e: index W
constexpr uint32_t GRID_SUMS = LAG_ELEMS * GRID_SUM_ROW;      // words per probed segment
constexpr uint32_t GRID_NO_SUM = 0xFFFFFFFFu;
constexpr uint32_t GRID_CANDS = LAG_CANDS + LAG_ELEMS;        // the candidates of the walk
constexpr unsigned long long GRID_NO_COST = 1ull << 56;       // never picked, and 33 of it fit 64 bits

// a width word as the plane probe uses it: outside 2 .. 65536 there is no candidate
GLC_ANS_HD inline uint32_t grid_width_word(uint32_t v) { return v >= GRID_W_MIN && v <= GRID_W_MAX ? v : 0u; }
// the largest width of a segment of N elements (N >= GRID_MIN_ELEMS)
GLC_ANS_HD inline uint32_t grid_wmax(unsigned long long N) { return N / 2 < GRID_W_MAX ? (uint32_t)(N / 2) : GRID_W_MAX; }
// the first target of tile t
GLC_ANS_HD inline unsigned long long grid_tile_start(unsigned long long N, uint32_t wmax, uint32_t t)
{
    return wmax + (unsigned long long)t * (N - wmax - GRID_TILE) / (GRID_TILES - 1);
}
// what one (target, predecessor) pair of e-byte elements adds to a sum
GLC_ANS_HD inline uint32_t grid_pair_bits(unsigned long long x, unsigned long long p, uint32_t elem)
{
    const unsigned long long mask = elem == 8 ? ~0ull : (1ull << (8 * elem)) - 1;
    return lag_bitlen(lag_fold((x - p) & mask, elem));
}
// the winner among S[2 .. wmax] (S indexed by width)
GLC_ANS_HD inline uint32_t grid_argmin(const uint32_t *S, uint32_t wmax)
{
    uint32_t w = GRID_W_MIN;
    for (uint32_t i = GRID_W_MIN + 1; i <= wmax; i++)
        if (S[i] < S[w]) w = i;
    return w;
}

// the 3 * 65537 sums and the three winners of the first len - len % 8 bytes of x, serially: for the checker
inline void grid_sums(const uint8_t *x, size_t len, uint32_t *S, uint32_t widths[LAG_ELEMS])
{
    const size_t P = len - len % 8;
    for (uint32_t k = 0; k < LAG_ELEMS; k++) {
        const uint32_t e = 2u << k;
        uint32_t *row = S + (size_t)k * GRID_SUM_ROW;
        for (uint32_t w = 0; w < GRID_SUM_ROW; w++) row[w] = GRID_NO_SUM;
        widths[k] = 0;
        const unsigned long long N = P / e;
        if (N < GRID_MIN_ELEMS) continue;
        auto at = [&](unsigned long long i) { unsigned long long v = 0; for (uint32_t b = 0; b < e; b++) v |= (unsigned long long)x[i * e + b] << (8 * b); return v; };
        const uint32_t wmax = grid_wmax(N);
        for (uint32_t w = GRID_W_MIN; w <= wmax; w++) {
            uint32_t s = 0;
            for (uint32_t t = 0; t < GRID_TILES; t++) {
                const unsigned long long b = grid_tile_start(N, wmax, t);
                for (uint32_t j = 0; j < GRID_TILE; j++) s += grid_pair_bits(at(b + j), at(b + j - w), e);
            }
            row[w] = s;
        }
        widths[k] = grid_argmin(row, wmax);
    }
}

// a candidate of the walk: lag_rule.h's, and for the last three the grid filter at widths[k] with the fold (width 0 otherwise)
struct GridCand { uint8_t elem, delta, lag, fold; uint32_t width; };
GLC_ANS_HD inline GridCand grid_cand(uint32_t i, const uint32_t lags[LAG_ELEMS], const uint32_t widths[LAG_ELEMS])
{
    if (i < LAG_CANDS) { const LagCand c = lag_cand(i, lags); return GridCand{c.elem, c.delta, c.lag, c.fold, 0}; }
    const uint32_t k = i - LAG_CANDS;
    return GridCand{(uint8_t)(2u << k), 1, 1, 1, widths[k]};
}
// the margin walk over the thirteen costs
inline uint32_t grid_pick(const unsigned long long cost[GRID_CANDS])
{
    uint32_t pick = 0;
    for (uint32_t i = 1; i < GRID_CANDS; i++)
        if (FILTER_MARGIN_NUM * cost[i] < FILTER_MARGIN_DEN * cost[pick]) pick = i;
    return pick;
}

} // namespace glc
