// shuffle_tile.h -- what the kernels of shuffle.hip and delta.hip share: the 16 KiB tile's geometry, the split of a byte run into
// a head, whole 16-byte granules and a tail, and the packing of 16 bytes into one store.
#pragma once
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t SH_TILE = 16384, SH_THREADS = 256;
constexpr uint32_t SH_BATCH_GRID = 2048;                       // batched form: 8 workgroups for each of 256 CUs
constexpr uint32_t SH_NGI = SH_TILE / 16 + 1;                  // granules that cover a 16 KiB range of any alignment
constexpr uint32_t SH_LDS_WORDS = 4 * SH_NGI + SH_NGI / 2 + 1 + 32;   // forward image with pads (ELEM = 2 pads most)

template <uint32_t ELEM> struct ShGeom {
    static constexpr uint32_t LG = ELEM == 2 ? 1 : (ELEM == 4 ? 2 : 3);
    static constexpr uint32_t TQ = SH_TILE / ELEM;             // elements per tile = bytes of a plane run
    static constexpr uint32_t NGP = TQ / 16 + 1;               // granules that cover a plane run
    static constexpr uint32_t PPW = ELEM > 4 ? ELEM / 4 : 1;   // planes per wave
    static constexpr uint32_t WPP = ELEM < 4 ? 4 / ELEM : 1;   // waves per plane
};

// a run of R bytes at address O: `head` bytes up to the first 16-byte boundary, nf whole granules, `tail` bytes
struct ShRun { uint32_t head, nf, tail; };
__device__ __forceinline__ ShRun sh_run(unsigned long long O, uint32_t R)
{
    ShRun r;
    r.head = min(R, (16u - (uint32_t)(O & 15)) & 15u);
    r.nf = (R - r.head) / 16;
    r.tail = (R - r.head) % 16;
    return r;
}

__device__ __forceinline__ uint4 sh_pack(const uint32_t (&b)[16])
{
    return make_uint4(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24),
                      b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24), b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24));
}

} // namespace glc
