// lag_tile.h -- what the forward kernels of lag.hip and grid.hip share over shuffle_tile.h: element-wise arithmetic on 16-byte
// granules held as four dwords (masking by run-relative position, add / subtract, the fold), the read of 16 bytes at any byte
// of an LDS image, and the plane build from the padded image of a tile's differences.
#pragma once
#include "shuffle_tile.h"

namespace glc {

constexpr uint32_t LG_RUN = 2048;                              // elements between two restarts (delta.hip's DL_RUN)
constexpr uint32_t LG_IMG_WORDS = SH_TILE / 4 + SH_TILE / 32;  // padded image at s = 0 (ELEM = 2 pads most)

typedef unsigned short lg_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ lg_us2 lg_halves(uint32_t v) { return __builtin_bit_cast(lg_us2, v); }
__device__ __forceinline__ uint32_t lg_word(lg_us2 v) { return __builtin_bit_cast(uint32_t, v); }

// p with every element zeroed whose run-relative byte, gb + its offset in the granule, is below dist
template <uint32_t ELEM>
__device__ __forceinline__ void lg_mask(uint32_t (&p)[4], uint32_t gb, uint32_t dist)
{
#pragma unroll
    for (uint32_t m = 0; m < 4; m++) {
        if constexpr (ELEM == 2) p[m] &= (gb + 4 * m >= dist ? 0xFFFFu : 0u) | (gb + 4 * m + 2 >= dist ? 0xFFFF0000u : 0u);
        else p[m] = gb + (ELEM == 8 ? 8 * (m / 2) : 4 * m) >= dist ? p[m] : 0u;
    }
}

// c +- p, element by element
template <uint32_t ELEM, bool SUB>
__device__ __forceinline__ void lg_combine(uint32_t (&c)[4], const uint32_t (&p)[4])
{
    if constexpr (ELEM == 8) {
#pragma unroll
        for (uint32_t i = 0; i < 2; i++) {
            const unsigned long long a = c[2 * i] | ((unsigned long long)c[2 * i + 1] << 32), b = p[2 * i] | ((unsigned long long)p[2 * i + 1] << 32);
            const unsigned long long r = SUB ? a - b : a + b;
            c[2 * i] = (uint32_t)r; c[2 * i + 1] = (uint32_t)(r >> 32);
        }
    } else {
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) {
            if constexpr (ELEM == 4) c[m] = SUB ? c[m] - p[m] : c[m] + p[m];
            else c[m] = lg_word(SUB ? lg_halves(c[m]) - lg_halves(p[m]) : lg_halves(c[m]) + lg_halves(p[m]));
        }
    }
}

// the fold (fold = 0: nothing) and its inverse, element by element
template <uint32_t ELEM, bool INVERSE>
__device__ __forceinline__ void lg_fold(uint32_t (&d)[4], uint32_t fold)
{
    if constexpr (ELEM == 8) {
#pragma unroll
        for (uint32_t i = 0; i < 2; i++) {
            const unsigned long long v = d[2 * i] | ((unsigned long long)d[2 * i + 1] << 32);
            const unsigned long long r = INVERSE ? (v >> fold) ^ (0ull - (v & fold)) : (v << fold) ^ (0ull - ((v >> 63) & fold));
            d[2 * i] = (uint32_t)r; d[2 * i + 1] = (uint32_t)(r >> 32);
        }
    } else if constexpr (ELEM == 4) {
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) d[m] = INVERSE ? (d[m] >> fold) ^ (0u - (d[m] & fold)) : (d[m] << fold) ^ (0u - ((d[m] >> 31) & fold));
    } else {
        const lg_us2 f = {(unsigned short)fold, (unsigned short)fold}, z = {0, 0}, s = {15, 15};
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) {
            const lg_us2 v = lg_halves(d[m]);
            d[m] = lg_word(INVERSE ? (v >> f) ^ (z - (v & f)) : (v << f) ^ (z - ((v >> s) & f)));
        }
    }
}

// the 16 bytes at byte b (b >= -4 * front of the caller's slack) of an LDS image whose byte 0 is at words: five aligned dwords
__device__ __forceinline__ void lg_read16(const uint32_t *words, int b, uint32_t (&o)[4])
{
    const uint32_t *p = words + (b >> 2);
    const uint32_t sb = (uint32_t)b & 3;
    uint32_t w[5];
#pragma unroll
    for (int m = 0; m < 5; m++) w[m] = p[m];
#pragma unroll
    for (int m = 0; m < 4; m++) o[m] = __builtin_amdgcn_alignbyte(w[m + 1], w[m], sb);
}

// granule g of a tile's differences into the padded image: one pad dword behind every 16 << LG bytes
template <uint32_t ELEM>
__device__ __forceinline__ void lg_img_store(uint32_t *img, uint32_t g, const uint32_t (&c)[4])
{
    uint32_t *dst = img + 4 * g + (g >> ShGeom<ELEM>::LG);
    dst[0] = c[0]; dst[1] = c[1]; dst[2] = c[2]; dst[3] = c[3];
}

// the planes of elements [i0, i0 + cnt) from the padded image, as delta.hip's forward tile: byte B = ELEM e + j lies at
// B + 4 * (B >> SH); plane j of the output starts at out + j q; tid, lane, wave: the caller's, the wave uniform (read at the tile's start)
template <uint32_t ELEM>
__device__ __forceinline__ void lg_planes(const uint32_t *img, uint8_t *out, unsigned long long q, unsigned long long i0, uint32_t cnt,
                                          uint32_t tid, uint32_t lane, uint32_t wave)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t SH = 4 + G::LG;                         // log2 of the bytes between two pad dwords
    const uint8_t *ldsb = reinterpret_cast<const uint8_t *>(img);
#pragma unroll
    for (uint32_t pp = 0; pp < G::PPW; pp++) {
        const uint32_t j = G::WPP > 1 ? wave % ELEM : wave + 4 * pp;
        const uint32_t sub = G::WPP > 1 ? wave / ELEM : 0;
        const unsigned long long O = (unsigned long long)(uintptr_t)out + j * q + i0;
        const ShRun r = sh_run(O, cnt);
        const uint32_t c = j + ELEM * r.head;
        const uint32_t ru = c & ((16u << G::LG) - 1);
        uint4 *dst = reinterpret_cast<uint4 *>(out + (j * q + i0 + r.head));
        for (uint32_t h = sub * 64 + lane; h < r.nf; h += 64 * G::WPP) {
            const uint32_t B0 = c + ((16 * h) << G::LG);
            const uint32_t P0 = B0 + 4 * (B0 >> SH);
            uint32_t b[16];
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) b[k] = ldsb[P0 + ELEM * k + 4 * ((ru + ELEM * k) >> SH)];
            dst[h] = sh_pack(b);
        }
    }
    {
        const uint32_t j = tid >> 5, x = tid & 31;
        if (j < ELEM) {
            const unsigned long long O = (unsigned long long)(uintptr_t)out + j * q + i0;
            const ShRun r = sh_run(O, cnt);
            const bool is_head = x < 16;
            const uint32_t y = x & 15;
            if (y < (is_head ? r.head : r.tail)) {
                const uint32_t e = is_head ? y : r.head + 16 * r.nf + y;
                const uint32_t B = j + ELEM * e;
                out[j * q + i0 + e] = ldsb[B + 4 * (B >> SH)];
            }
        }
    }
}

} // namespace glc
