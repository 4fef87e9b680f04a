// grid_tile.h -- what the forward kernels of grid.hip and vol.hip share over lag_tile.h: the geometry of a raw LDS image of a
// tile and the element-wise select by a predicate on the element's place in its granule.
#pragma once
#include "lag_tile.h"

namespace glc {

constexpr uint32_t GD_FRONT = 4;                               // words in front of a raw image (a read starts up to 8 bytes early)
constexpr uint32_t GD_RAW_WORDS = GD_FRONT + 4 * SH_NGI;

// p with every element k zeroed for which keep(k) is false
template <uint32_t ELEM, class Keep>
__device__ __forceinline__ void gd_select(uint32_t (&p)[4], Keep keep)
{
#pragma unroll
    for (uint32_t m = 0; m < 4; m++) {
        if constexpr (ELEM == 2) p[m] &= (keep(2 * m) ? 0xFFFFu : 0u) | (keep(2 * m + 1) ? 0xFFFF0000u : 0u);
        else p[m] = keep(ELEM == 8 ? m / 2 : m) ? p[m] : 0u;
    }
}

} // namespace glc
