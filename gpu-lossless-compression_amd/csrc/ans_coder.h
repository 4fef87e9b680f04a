// ans_coder.h -- the constants and the integer pieces of the rANS mode (record kind 5, format version 7)
// that ans.hip, the host side and the stand-alone checker tools/ans_div_check.cpp share.  Plain C++: no GPU header needed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GLC_ANS_HD __host__ __device__
#else
#define GLC_ANS_HD
#endif

namespace glc {

constexpr uint32_t ANS_PROB_BITS = 12, ANS_M = 1u << ANS_PROB_BITS;   // probabilities are 12-bit: the q of a block sum to 4096
constexpr uint32_t ANS_L = 1u << 16;                                  // a state's lower bound; units are 16 bits
constexpr uint32_t ANS_CHUNK = 32768, ANS_LANES = 64;                 // a chunk: 64 interleaved lanes, 512 steps
constexpr uint32_t ANS_MAX_LEN = 1u << 20, ANS_MAX_CHUNKS = ANS_MAX_LEN / ANS_CHUNK;

GLC_ANS_HD inline uint32_t ans_chunks(uint32_t len) { return (len + ANS_CHUNK - 1) / ANS_CHUNK; }
// the largest record of a segment of len bytes, in words: every symbol emits at most one unit
GLC_ANS_HD inline unsigned long long ans_bound_words(uint32_t len)
{
    return (unsigned long long)ans_chunks(len) * (1 + ANS_LANES) + (len + 1ull) / 2 + ans_chunks(len);
}

// floor(x / f) for 1 <= f <= 4096 and any 32-bit x by multiply-high and shifts (Granlund and Montgomery, "Division by invariant
// integers using multiplication", fig. 4.1 with N = 32): l = ceil(log2 f), m = floor(2^32 (2^l - f) / f) + 1,
// t = mulhi(m, x), quotient = (t + ((x - t) >> min(l, 1))) >> max(l - 1, 0).  Exact: no float, no correction step.
struct AnsDiv { uint32_t m, l; };
GLC_ANS_HD inline AnsDiv ans_div_make(uint32_t f)
{
    uint32_t l = 0;
    while ((1u << l) < f) l++;
    return {(uint32_t)((((uint64_t)1 << 32) * ((1u << l) - f)) / f) + 1u, l};
}
GLC_ANS_HD inline uint32_t ans_div(uint32_t x, uint32_t m, uint32_t l)
{
    const uint32_t t = (uint32_t)(((uint64_t)m * x) >> 32);
    return (t + ((x - t) >> (l ? 1u : 0u))) >> (l ? l - 1u : 0u);
}

// a symbol's entry of a block's table: f = q[s] (0 .. 4096), c = cum[s], and the l of its divisor
GLC_ANS_HD inline uint32_t ans_pack(uint32_t f, uint32_t c, uint32_t l) { return f | (c << 13) | (l << 25); }
GLC_ANS_HD inline uint32_t ans_f(uint32_t w) { return w & 0x1FFFu; }
GLC_ANS_HD inline uint32_t ans_c(uint32_t w) { return (w >> 13) & 0xFFFu; }
GLC_ANS_HD inline uint32_t ans_l(uint32_t w) { return w >> 25; }

// one encoder step of a lane whose state has been renormalised (x < f * 2^20)
GLC_ANS_HD inline uint32_t ans_put(uint32_t x, uint32_t w, uint32_t m)
{
    const uint32_t f = ans_f(w), d = ans_div(x, m, ans_l(w));
    return (d << ANS_PROB_BITS) + (x - d * f) + ans_c(w);
}

} // namespace glc
