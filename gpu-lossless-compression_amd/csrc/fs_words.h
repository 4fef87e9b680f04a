// fs_words.h -- what the two fast suffix sorters share on the device: the layout of a suffix word and suffix comparison
// in the text.  bwt_bucket.hip (arithmetic-code bucket sorter) and bwt_sample.hip (string sample sort) include it.
#pragma once
#include "glc_internal.h"                                    // FS_LCP_CAP, SS_TOL_CAP

namespace glc {

// one word per suffix = [top 36 bits of its arithmetic code | suffix index : 20 | T[i-1] : 8]; the code: bwt_bucket.hip, top
#ifndef GLC_FS_DEPTH
#define GLC_FS_DEPTH 8
#endif
constexpr int      FS_DEPTH  = GLC_FS_DEPTH;        // symbols the arithmetic code of a suffix is made of (bwt_bucket.hip, top)
#ifndef GLC_SS_DEPTH
#define GLC_SS_DEPTH GLC_FS_DEPTH
#endif
constexpr int      SS_DEPTH  = GLC_SS_DEPTH;        // ... in the sample sorter's own words (k_ss_sample's samples and k_ss_part must agree; the tiers need not)
static_assert(FS_DEPTH >= 2 && FS_DEPTH <= 8 && SS_DEPTH >= 2 && SS_DEPTH <= 8, "a thread's 8 codes take their symbols from its 16 staged bytes");
constexpr uint64_t FS_LOW_MASK = (1ull << 28) - 1;  // [index : 20 | bwt : 8]

// ---------------------------------------------------------------------------
// suffix comparison in the text (runs of equal codes; the sample tier's splitters)
// ---------------------------------------------------------------------------
// (FS_LCP_CAP, glc_internal.h: a longer common prefix flags the block as deep)

// 8 bytes at any address as a big-endian number: ONE unaligned 8-byte load (global memory takes any alignment on
// gfx9+; built from aligned dwords it is three scattered loads per lane, and the gathers of the refinement
// rounds are bound by the number of addresses the texture path takes per clock)
__device__ __forceinline__ uint64_t fs_load_be64(const uint8_t *p)
{
    uint64_t x;
    __builtin_memcpy(&x, p, 8);
    return __builtin_bswap64(x);
}

// 16 bytes at any address as two big-endian numbers: ONE unaligned 16-byte load
__device__ __forceinline__ void fs_load_be128(const uint8_t *p, uint64_t &hi, uint64_t &lo)
{
    uint64_t x[2];
    __builtin_memcpy(x, p, 16);
    hi = __builtin_bswap64(x[0]);
    lo = __builtin_bswap64(x[1]);
}

// suffix a < suffix b ?  (a != b; the shorter of two suffixes that agree to the end of one is the smaller)
// tol (the sample sorter's second form, for blocks with repeats deeper than its cap: see ss_build): two suffixes that
// agree in their first SS_TOL_CAP + 8 bytes are ordered by their POSITIONS -- a total order that every comparison of the
// pass agrees on, and a (SS_TOL_CAP)-order of the suffixes, which is all the prefix-doubling rounds behind it need.
template <bool W16 = false>
__device__ __forceinline__ bool fs_suffix_less(const uint8_t *T, uint32_t n, uint32_t a, uint32_t b, bool *deep, uint32_t k = 0,
                                               bool tol = false)
{
    for (;;) {
        const uint32_t m = max(a, b) + k;
#ifndef GLC_TOL_STEP8
        if (W16 && m + 20 <= n) {                              // (every tolerant comparison starts at k = 0 or 16: all of them end their ties at k = 144)
#else
        if (W16 && !tol && m + 20 <= n) {
#endif
            const uint64_t va = fs_load_be64(T + a + k), vb = fs_load_be64(T + b + k);
            const uint64_t va2 = fs_load_be64(T + a + k + 8), vb2 = fs_load_be64(T + b + k + 8);
            if (va != vb) return va < vb;
            if (va2 != vb2) return va2 < vb2;
            k += 16;
        } else if (m + 12 <= n) {
            const uint64_t va = fs_load_be64(T + a + k), vb = fs_load_be64(T + b + k);
            if (va != vb) return va < vb;
            k += 8;
        } else {
            if (a + k >= n || b + k >= n) return a > b;        // one (or both: called with k > 0) ended: the shorter suffix is the smaller
            const uint32_t ca = T[a + k], cb = T[b + k];
            if (ca != cb) return ca < cb;
            k++;
        }
        if (tol && k > SS_TOL_CAP) { *deep = true; return a < b; }   // (*deep: "agreed up to the cap" -- a tie, not a give-up, for these callers)
        if (k > FS_LCP_CAP) { *deep = true; return false; }
    }
}

} // namespace glc
