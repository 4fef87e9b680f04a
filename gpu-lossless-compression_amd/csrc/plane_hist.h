// plane_hist.h -- the byte-plane counting step the plane probes share (lag_probe.hip's k_lp_planes, grid_probe.hip's k_gw_planes;
// k_fp_probe's scheme): a wave's 64 granules of 16 bytes into LDS histograms, with the uniform-value shortcut.
#pragma once
#include "glc_device.h"

namespace glc {

// the OR of x over the wave, in every lane's scalar (k_fp_probe's)
__device__ __forceinline__ uint32_t ph_wave_or(uint32_t x)
{
    x |= GLC_DPP(x, 0x111, 0xf);
    x |= GLC_DPP(x, 0x112, 0xf);
    x |= GLC_DPP(x, 0x114, 0xf);
    x |= GLC_DPP(x, 0x118, 0xf);
    x |= GLC_DPP(x, 0x142, 0xa);
    x |= GLC_DPP(x, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// one group of a pass: this lane's n (0, 8 or 16) bytes d into the histograms row0 .. row0 + e - 1 of H (rows PITCH words apart),
// byte k to row row0 + k % e.  whole (wave-uniform): every lane of the wave holds 16 bytes
template <uint32_t PITCH>
__device__ __forceinline__ void ph_group(uint32_t *H, const uint32_t (&d)[4], uint32_t n, bool whole, uint32_t row0, uint32_t e, uint32_t lane)
{
    if (whole) {                                               // every lane holds 16 bytes: are they the first lane's?
        uint32_t f[4];
        bool same = true;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            f[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[k]);
            same = same && d[k] == f[k];
        }
        if (__ballot(!same) == 0) {
            if (lane < 16) {
                const uint32_t w = lane < 4 ? f[0] : lane < 8 ? f[1] : lane < 12 ? f[2] : f[3];
                atomicAdd(&H[(row0 + (lane & (e - 1))) * PITCH + ((w >> (8 * (lane & 3))) & 0xFFu)], 64u);
            }
            return;
        }
        // the byte positions that hold one value in every lane (the high bytes of a small difference) cost one add of 64
        uint32_t var[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) var[k] = ph_wave_or(d[k] ^ f[k]);
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            uint32_t *row = H + (row0 + (k & (e - 1))) * PITCH;
            if ((var[k >> 2] >> (8 * (k & 3))) & 0xFFu) atomicAdd(&row[(d[k >> 2] >> (8 * (k & 3))) & 0xFFu], 1u);
            else if (lane == 0) atomicAdd(&row[(f[k >> 2] >> (8 * (k & 3))) & 0xFFu], 64u);
        }
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        if (k < n) atomicAdd(&H[(row0 + (k & (e - 1))) * PITCH + ((d[k >> 2] >> (8 * (k & 3))) & 0xFFu)], 1u);
}

} // namespace glc
