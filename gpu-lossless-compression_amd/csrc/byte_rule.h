// byte_rule.h -- the integer pieces of the byte rule (INTEGRATION.md 4b "Filter: auto with bytes") that byte_probe.hip, the host
// side and the stand-alone checker tools/filter_byte_rule_check.cpp share: which lag and which row stride of the byte predictor
// (byte_delta.hip) a segment wants, and the walk that weighs its two candidates against the thirteen of grid_rule.h, which stays
// as it is, as lag_rule.h does.  Plain C++: no GPU header needed.
//   A segment's first P = L - L % 8 bytes x[i]; N = P.  N < 1024: no byte candidate, both costs GRID_NO_COST.  Else
//     lag sums     A[l] = sum over i < P of m((x[i] - p) mod 256) for l = 1 .. 16, p = x[i - l] where i mod 2048 >= l and 0 elsewhere
//                  (the run heads of byte_delta.hip), m(d) = d for d < 128 and 255 - d otherwise: the fold without its sign bit, a
//                  magnitude and not a bit length (four of them are one v_sad_u8).  Sixteen sums of 64 bits, A[l] at l - 1.
//                  The winner is the l with the smallest sum, ties to the smallest l.
//     stride sums  grid_rule.h's sample and statistic at element size 1: Wmax = min(65536, N / 2), 32 tiles of 256 targets at
//                  grid_tile_start(N, Wmax, t), S[W] = sum of bitlen(fold((x[i] - x[i - W]) mod 256)) for W = 17 .. Wmax -- 17 is one
//                  above the largest lag: a stride of 16 or less is a neighbour in the same row.  A row of 65537 words, S[W] at W,
//                  0xFFFFFFFF outside 17 .. Wmax.  The winner is the W with the smallest sum, ties to the smallest W.
//     planes       two rows of 256 counts: the histograms of what glcByteDeltaDevice(lag, 0) and glcByteDeltaDevice(lag, stride)
//                  write from the counted bytes, bands and run heads included
//     costs        filter_plane_cost of each row
//   The walk is grid_rule.h's over fifteen candidates: its thirteen in their order, then byte (lag, 0), then byte (lag, stride).
//   Among the first thirteen candidate i replaces the pick exactly when 33 cost[i] < 32 cost[pick].  A byte candidate replaces a
//   pick of one plane (candidate 0, or byte (lag, 0)) under the same margin, and a pick of two or more planes (an element size of
//   2, 4 or 8) exactly when cost[i] < cost[pick]: the margin is there because splitting into more planes never raises an empirical
//   entropy (filter_rule.h), and a byte candidate has fewer planes than such a pick, so that bias works against it, not for it.
//   Without this, two interleaved 8-bit channels stay with (2, delta), whose two planes are the byte predictor's output at lag 2
//   but for the borrows between the bytes: 0.7 % more by the costs, inside the margin.
//   Words read from device memory: a lag word is used as ((v - 1) & 15) + 1; a stride word outside 17 .. 65536 names no candidate
//   (its row is zero and its cost GRID_NO_COST).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "grid_rule.h"

namespace glc {

constexpr uint32_t BYTE_MIN_LEN = 1024;                       // a segment with fewer counted bytes has no byte candidate
constexpr uint32_t BYTE_LAGS = 16;                            // lags 1 .. 16 (byte_delta.hip's)
constexpr uint32_t BYTE_S_MIN = 17, BYTE_S_MAX = 65536;       // the strides the rule looks at
constexpr uint32_t BYTE_SUM_ROW = BYTE_S_MAX + 1;             // words of S: index W
constexpr uint32_t BYTE_RUN = 2048;                           // bytes between two run heads
constexpr uint32_t BYTE_ROWS = 2;                             // histograms per probed segment: (lag, 0), then (lag, stride)
constexpr uint32_t BYTE_CANDS = GRID_CANDS + BYTE_ROWS;       // the candidates of the walk

// what one (byte, predecessor) pair adds to a lag sum
GLC_ANS_HD inline uint32_t byte_mag(uint32_t x, uint32_t p)
{
    const uint32_t d = (x - p) & 0xFFu;
    return d < 128 ? d : 255u - d;
}
// a stride word as the plane probe uses it: outside 17 .. 65536 there is no candidate
GLC_ANS_HD inline uint32_t byte_stride_word(uint32_t v) { return v >= BYTE_S_MIN && v <= BYTE_S_MAX ? v : 0u; }
// the winner of the sixteen lag sums
GLC_ANS_HD inline uint32_t byte_lag_argmin(const unsigned long long A[BYTE_LAGS])
{
    uint32_t w = 0;
    for (uint32_t l = 1; l < BYTE_LAGS; l++)
        if (A[l] < A[w]) w = l;
    return w + 1;
}
// the winner among S[17 .. wmax] (S indexed by stride)
GLC_ANS_HD inline uint32_t byte_stride_argmin(const uint32_t *S, uint32_t wmax)
{
    uint32_t w = BYTE_S_MIN;
    for (uint32_t i = BYTE_S_MIN + 1; i <= wmax; i++)
        if (S[i] < S[w]) w = i;
    return w;
}

// the sixteen lag sums, the 65537 stride sums and the two winners {lag, stride} (stride 0: no candidate) of the first
// len - len % 8 bytes of x, serially: for the checker
inline void byte_sums(const uint8_t *x, size_t len, unsigned long long A[BYTE_LAGS], uint32_t *S, uint32_t win[2])
{
    const size_t P = len - len % 8;
    for (uint32_t l = 1; l <= BYTE_LAGS; l++) {
        unsigned long long s = 0;
        for (size_t i = 0; i < P; i++) s += byte_mag(x[i], i % BYTE_RUN >= l ? x[i - l] : 0u);
        A[l - 1] = s;
    }
    win[0] = byte_lag_argmin(A);
    win[1] = 0;
    for (uint32_t w = 0; w < BYTE_SUM_ROW; w++) S[w] = GRID_NO_SUM;
    if (P < BYTE_MIN_LEN) return;
    const uint32_t wmax = grid_wmax(P);
    for (uint32_t w = BYTE_S_MIN; w <= wmax; w++) {
        uint32_t s = 0;
        for (uint32_t t = 0; t < GRID_TILES; t++) {
            const unsigned long long b = grid_tile_start(P, wmax, t);
            for (uint32_t j = 0; j < GRID_TILE; j++) s += grid_pair_bits(x[b + j], x[b + j - w], 1);
        }
        S[w] = s;
    }
    win[1] = byte_stride_argmin(S, wmax);
}

// a candidate of the walk: grid_rule.h's, and for the last two the byte predictor (elem 1) at `lag` and at stride 0 or `stride`
// (in width)
GLC_ANS_HD inline GridCand byte_cand(uint32_t i, const uint32_t lags[LAG_ELEMS], const uint32_t widths[LAG_ELEMS], uint32_t lag, uint32_t stride)
{
    if (i < GRID_CANDS) return grid_cand(i, lags, widths);
    return GridCand{1, 1, (uint8_t)lag, 0, i == GRID_CANDS ? 0u : stride};
}
// the walk over the fifteen costs: grid_rule.h's over the first thirteen, then the two byte candidates -- under the margin against
// a pick of one plane, on the plain costs against a pick of more
inline uint32_t byte_pick(const unsigned long long cost[BYTE_CANDS])
{
    uint32_t pick = grid_pick(cost);
    for (uint32_t i = GRID_CANDS; i < BYTE_CANDS; i++) {
        const bool one_plane = pick == 0 || pick >= GRID_CANDS;
        if (one_plane ? FILTER_MARGIN_NUM * cost[i] < FILTER_MARGIN_DEN * cost[pick] : cost[i] < cost[pick]) pick = i;
    }
    return pick;
}

} // namespace glc
