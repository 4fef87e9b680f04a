// dedup_rule.h -- which blocks of a version-9 frame a range read decodes ("dedup": range reads).  Host code,
// no device part; tools/dedup_rule_check.cpp holds it against a brute-force set under the host sanitizers.
// Blocks [first, last] of a frame of nb blocks are NEEDED: their bytes are asked for.  A needed block b of kind 6 may copy chunks
// from any block of [bwt_index[b], b], so the blocks of [bwt_index[b], b) in front of the range are needed AS SOURCES: decoded and
// joined, but not filled (a source chunk is a kept chunk, so a source-only block's own holes are never read) and not compared with
// their crc_raw (their holes stay unfilled; the needed block's crc_raw covers what was copied out of them).  Every such interval
// ends at a needed block, so their union in front of the range is one interval [lo, first): lo is the smallest bwt_index of a
// needed kind-6 block, or first.  The interval is wider than the exact set of source blocks, which only the ref lists give.
// A bwt_index above its block is what the field checks refuse; here it is ignored, so the result is in range whatever the tables
// hold.
#pragma once
#include <stdint.h>

namespace glc {

constexpr uint32_t DEDUP_KIND = 6;

constexpr uint8_t DEDUP_NEEDED = 1, DEDUP_SOURCE = 2;         // a block's mark: filled and compared with its crc_raw; decoded and joined only

// the first block to decode for the needed blocks [first, last], first <= last < nb
inline uint32_t dedup_first_block(const uint32_t *kind, const uint32_t *bwt_index, uint32_t nb, uint32_t first, uint32_t last)
{
    uint32_t lo = first;
    for (uint32_t b = first; b <= last && b < nb; b++)
        if (kind[b] == DEDUP_KIND && bwt_index[b] < lo) lo = bwt_index[b];
    return lo;
}

// The decoder's call.  mark[b] (nb entries) is DEDUP_NEEDED for the needed blocks -- any set, a filter's planes need several runs --
// and 0 elsewhere; every maximal run of needed blocks asks for its sources, and a block in front of a run that is not needed
// itself becomes DEDUP_SOURCE.  Returns the blocks decoded (marks other than 0): what glcContainerLastRangeStats counts.
inline uint32_t dedup_mark_sources(const uint32_t *kind, const uint32_t *bwt_index, uint32_t nb, uint8_t *mark)
{
    for (uint32_t a = 0; a < nb;) {
        if (mark[a] != DEDUP_NEEDED) { a++; continue; }
        uint32_t b = a;
        while (b + 1 < nb && mark[b + 1] == DEDUP_NEEDED) b++;
        for (uint32_t j = dedup_first_block(kind, bwt_index, nb, a, b); j < a; j++) if (!mark[j]) mark[j] = DEDUP_SOURCE;
        a = b + 1;
    }
    uint32_t decoded = 0;
    for (uint32_t b = 0; b < nb; b++) decoded += mark[b] != 0;
    return decoded;
}

} // namespace glc
