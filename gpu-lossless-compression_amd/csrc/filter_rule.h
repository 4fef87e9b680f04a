// filter_rule.h -- the integer pieces of the filter rule (INTEGRATION.md 4b "filter: auto") that filter_probe.hip, the host side
// and the stand-alone checker tools/filter_rule_check.cpp share: the candidate filters in their fixed order, the planes of the
// filter probe that make up each candidate, the cost of a plane from its 256 byte counts and the margin walk that picks a
// candidate from the seven costs.  Plain C++: no GPU header needed.
//   A segment's first P = L - L % 8 bytes are probed into 22 histograms of 256 counts (FILTER_ROWS):
//     rows 0..7    A_k[v]    = positions p < P with p % 8 == k and x[p] == v
//     rows 8..9    D_2[j][v], rows 10..13 D_4[j][v], rows 14..21 D_8[j][v] = elements i < P / e whose delta d_e[i] has byte j equal
//                  to v; d_e[i] = x_e[i] where i % 2048 == 0, else x_e[i] - x_e[i-1] modulo 2^(8 e), elements little-endian
//   Plane j of candidate (e, 0) is the sum of the A_k with k = j modulo e; plane j of (e, 1) is D_e[j].
//   cost(plane) = sum_s H[s] * AUTO_COST[q(s)], q(s) = clamp(floor(H[s] * 4096 / N), 1, 4096) for H[s] > 0, N = sum H: the bits, in
//   1/256 bit, of the plane's bytes at their own frequencies rounded down to 12 bits.  A candidate's cost is the sum over its planes.
//   With P <= 2^31, H * 4096 < 2^44 and a candidate's cost is at most 2^31 * 3072 < 2^43: 64-bit integers, no rounding anywhere.
// The minimum of the costs alone is the wrong rule: splitting into more planes never raises an empirical entropy, so it would pick
// elem 8 on float32 and on text.  A later candidate must win by a margin: it replaces the pick when 33 cost < 32 cost[pick].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "auto_rule.h"

namespace glc {

constexpr uint32_t FILTER_CANDS = 7;
constexpr uint32_t FILTER_ROWS = 22;                         // histograms per probed segment
constexpr uint32_t FILTER_PLANES = 29;                       // 1 + 2 + 2 + 4 + 4 + 8 + 8 planes over the seven candidates
constexpr uint32_t FILTER_RUN = 2048;                        // elements between two delta restarts (glcDeltaShuffleDevice's)
constexpr uint32_t FILTER_MARGIN_NUM = 33, FILTER_MARGIN_DEN = 32;

struct FilterCand { uint8_t elem, delta; };
// the candidates in the order the walk visits them; (1, 0) is no filter
GLC_ANS_HD inline FilterCand filter_cand(uint32_t i)
{
    const uint8_t e[FILTER_CANDS] = {1, 2, 2, 4, 4, 8, 8}, d[FILTER_CANDS] = {0, 0, 1, 0, 1, 0, 1};
    return FilterCand{e[i], d[i]};
}
// the first of a candidate's planes in the list of all 29, candidate by candidate
GLC_ANS_HD inline uint32_t filter_first_plane(uint32_t cand)
{
    const uint8_t first[FILTER_CANDS + 1] = {0, 1, 3, 5, 9, 13, 21, 29};
    return first[cand];
}
// the first row of D_e among the probe's rows
GLC_ANS_HD inline uint32_t filter_delta_row(uint32_t elem) { return elem == 2 ? 8u : elem == 4 ? 10u : 14u; }

// plane `plane` (0 .. 28) as rows of the probe: its candidate, and the rows first, first + step, ... (count of them) whose sum it is
struct FilterPlane { uint32_t cand, first, step, count; };
GLC_ANS_HD inline FilterPlane filter_plane(uint32_t plane)
{
    uint32_t c = 0;
    while (plane >= filter_first_plane(c + 1)) c++;
    const FilterCand f = filter_cand(c);
    const uint32_t j = plane - filter_first_plane(c);
    if (f.delta) return FilterPlane{c, filter_delta_row(f.elem) + j, 1u, 1u};
    return FilterPlane{c, j, f.elem, 8u / f.elem};
}

// what symbol s adds to the cost of a plane of N bytes in all where it comes up h times (h <= N <= 2^31)
GLC_ANS_HD inline unsigned long long filter_symbol_cost(uint32_t h, unsigned long long N)
{
    if (h == 0) return 0ull;
    const unsigned long long q = (unsigned long long)h * ANS_M / N;
    return (unsigned long long)h * auto_cost(q < 1 ? 1u : (uint32_t)q);
}
// the cost of a plane from its 256 counts (all zero: 0)
GLC_ANS_HD inline unsigned long long filter_plane_cost(const uint32_t H[256])
{
    unsigned long long N = 0, sum = 0;
    for (uint32_t s = 0; s < 256; s++) N += H[s];
    for (uint32_t s = 0; s < 256; s++) sum += filter_symbol_cost(H[s], N);
    return sum;
}
// the seven costs of one segment from the 22 rows of its probe (rows[22 * 256]), serially: for the host and the checker
inline void filter_costs(const uint32_t *rows, unsigned long long cost[FILTER_CANDS])
{
    for (uint32_t c = 0; c < FILTER_CANDS; c++) cost[c] = 0;
    for (uint32_t p = 0; p < FILTER_PLANES; p++) {
        const FilterPlane pl = filter_plane(p);
        uint32_t H[256];
        for (uint32_t s = 0; s < 256; s++) {
            H[s] = 0;
            for (uint32_t k = 0; k < pl.count; k++) H[s] += rows[(size_t)(pl.first + k * pl.step) * 256 + s];
        }
        cost[pl.cand] += filter_plane_cost(H);
    }
}
// the margin walk: the index of the candidate a frame of these costs is filtered with
inline uint32_t filter_pick(const unsigned long long cost[FILTER_CANDS])
{
    uint32_t pick = 0;
    for (uint32_t i = 1; i < FILTER_CANDS; i++)
        if (FILTER_MARGIN_NUM * cost[i] < FILTER_MARGIN_DEN * cost[pick]) pick = i;
    return pick;
}

} // namespace glc
