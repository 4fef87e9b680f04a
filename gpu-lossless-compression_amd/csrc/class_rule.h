// class_rule.h -- the rule of the CHOOSE codec with filters (INTEGRATION.md 4b "choose with filters"): which class a block of a
// super-frame belongs to, from the filter probe's seven costs of the block (filter_rule.h), at level 5 the cost of the byte
// predictor at the block's best lag (byte_rule.h), and the bigram probe's stats row (choose_rule.h).  The writer cuts a frame
// wherever the class changes; the class never names a frame's filter -- the level's own probe chain over the whole run does.
// Plain C++, shared by the host side and the stand-alone checker tools/class_rule_check.cpp: no GPU header needed.
//   level   0: today's CHOOSE (version 3); 1: the order-0 frames take the auto mode (version 8); 2: and filter-auto (version 10);
//           3: and filter-lag (13); 4: and filter-grid (14); 5: and filter-byte (16)
//   A block of L bytes is
//     typed    when L >= CHOOSE_MIN_LEN, the level is 2 or more, and the walk over its costs picks a candidate other than (1, 0):
//              filter_pick() over the seven, and at level 5 an eighth candidate behind them, the byte predictor at (best lag, stride
//              0), under byte_rule.h's margin rule for a byte candidate (against a pick of one plane 33 cost < 32 cost[pick], against
//              a pick of more planes cost < cost[pick]).  Its element size e is the pick's: 2, 4 or 8, or 1 for the byte candidate;
//     BWT      when it is not typed and choose_bwt() says so;
//     order-0  otherwise, with e = 0.
//   The key of a block is CLASS_BWT or its e; every maximal run of blocks of one key is one frame.
#pragma once
#include <stdint.h>

#include "byte_rule.h"
#include "choose_rule.h"

namespace glc {

constexpr uint32_t CLASS_MAX_LEVEL = 5;
constexpr uint32_t CLASS_BWT = 0xFFu;                        // the key of a BWT block (the others: e = 0, 1, 2, 4, 8)
constexpr uint32_t CLASS_COSTS = FILTER_CANDS + 1;           // a block's cost row: filter_rule.h's seven, then byte (best lag, 0)

// the container version a level writes (0: CHOOSE's own version 3)
inline uint32_t class_version(uint32_t level)
{
    const uint32_t v[CLASS_MAX_LEVEL + 1] = {3, 8, 10, 13, 14, 16};
    return v[level <= CLASS_MAX_LEVEL ? level : 0];
}
// the element size of a typed block, 0 where the block is not typed.  cost[7] is read at level 5 alone
inline uint32_t class_typed(uint32_t level, unsigned long long L, const unsigned long long cost[CLASS_COSTS])
{
    if (level < 2 || L < CHOOSE_MIN_LEN) return 0;
    const uint32_t pick = filter_pick(cost);
    if (level >= 5) {
        const unsigned long long cb = cost[FILTER_CANDS];
        if (pick == 0 ? FILTER_MARGIN_NUM * cb < FILTER_MARGIN_DEN * cost[0] : cb < cost[pick]) return 1;
    }
    return pick ? filter_cand(pick).elem : 0u;
}
inline uint32_t class_key(uint32_t level, unsigned long long L, const unsigned long long cost[CLASS_COSTS], const unsigned long long stats[CHOOSE_STATS])
{
    const uint32_t e = class_typed(level, L, cost);
    if (e) return e;
    return choose_bwt(L, stats) ? CLASS_BWT : 0u;
}

} // namespace glc
