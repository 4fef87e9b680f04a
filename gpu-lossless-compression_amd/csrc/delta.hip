// delta.hip -- the delta mode of the container's typed-data filter (format version 4): the byte-plane shuffle
// of shuffle.hip applied to the differences of neighbouring elements, and its inverse, each fused into one kernel so that a
// segment is still read once and written once.  With x[i] element i of a segment as a little-endian unsigned integer of ELEM
// = 2, 4 or 8 bytes and RUN = 2048 elements:
//   forward   d[i] = x[i] where i mod RUN == 0, else x[i] - x[i - 1] (mod 2^(8 ELEM)); out[j q + i] = byte j of d[i]
//   inverse   the planes gathered back into d; x[i] = the sum of d[RUN * (i / RUN)] .. d[i]
// over the q = len / ELEM whole elements, the last len % ELEM bytes copied in place.
//
// The delta restarts every RUN elements and the 16 KiB tile of the shuffle holds 4, 2 or 1 whole runs, so a tile needs nothing
// from outside itself in either direction: no workgroup waits for another, there is no flag, look-back or atomic anywhere.
//
// Forward, one tile: the address-aligned 16-byte granules that cover the tile's input go to LDS as they are (the raw image,
// one global_load_dwordx4 and one ds_write_b128 per lane and granule).  Then every lane takes element-aligned granules of the
// tile -- tile bytes [16 g, 16 g + 16), at raw byte s + 16 g where s is the input's misalignment -- as the aligned dwords that
// cover them and the element in front, funnel-shifted by s mod 4 bytes (v_alignbyte), subtracts, and stores the differences
// into a second image with the pad dwords of shuffle.hip's forward image at s = 0.  Planes are built from that image exactly
// as there: 16 byte reads and one 16-byte store per output granule, heads and tails of the plane runs as bytes.
// Inverse, one tile: the ELEM plane runs go to ELEM regions of LDS as in shuffle.hip.  Lane t of the workgroup takes the
// element-aligned granules t, t + 256, t + 512, t + 768: 16 byte reads reassemble 16 / ELEM differences, which the lane sums
// serially; an inclusive scan over the wave (six DPP steps; 64-bit adds are add / add-with-carry pairs) and the totals
// of the waves in front -- 16 words of LDS, one barrier for all four passes -- give the sum in front of the lane within its
// run.  A pass of the workgroup covers 4096 bytes, that is one run, half a run or a quarter of one: the carry from pass to
// pass is dropped where a run starts.  The elements go to a flat image of the tile, from which output granules are cut at the
// output's own alignment (five dword reads and four v_alignbyte each) and stored as 16 bytes; head and tail as bytes.
// Loads touch only aligned granules that hold a byte of the caller's buffers, stores exactly the bytes of the segment.
//
// LDS: forward 34848 bytes (raw image 16416, padded image 18432), inverse 33024 bytes: four workgroups per CU each, against
// eight of the plain shuffle, whose kernels are untouched.  Single segment, one workgroup per tile, 64-bit offsets.
#include "shuffle_tile.h"

namespace glc {

constexpr uint32_t DL_RUN = 2048;                              // elements between two restarts of the delta
constexpr uint32_t DL_PASSES = SH_TILE / 16 / SH_THREADS;      // element-aligned granules of a tile per lane
constexpr uint32_t DL_RAW_WORDS = 4 + 4 * SH_NGI;              // raw image: 4 words in front so that granule 0 may read "before" it
constexpr uint32_t DL_IMG_WORDS = SH_TILE / 4 + SH_TILE / 32;  // padded image at s = 0 (ELEM = 2 pads most)
constexpr uint32_t DL_FLAT_WORDS = SH_TILE / 4 + 4;            // inverse: the tile's elements, one granule of slack behind
constexpr uint32_t DL_REGION_WORDS = SH_TILE / 4 + 4 * 8;      // inverse: ELEM plane regions of 16 NGP bytes
static_assert(DL_PASSES == 4, "four passes of 256 lanes cover a tile");

// the 16 / ELEM elements of a granule, c[0..3], minus their predecessors; p = the two dwords in front of c[0]
template <uint32_t ELEM>
__device__ __forceinline__ uint4 dl_differences(const uint32_t (&c)[4], uint32_t p0, uint32_t p1, bool first)
{
    if constexpr (ELEM == 4) {
        return make_uint4(c[0] - (first ? 0u : p1), c[1] - c[0], c[2] - c[1], c[3] - c[2]);
    } else if constexpr (ELEM == 8) {
        const unsigned long long a = c[0] | ((unsigned long long)c[1] << 32), b = c[2] | ((unsigned long long)c[3] << 32);
        const unsigned long long pv = first ? 0ull : (p0 | ((unsigned long long)p1 << 32));
        const unsigned long long da = a - pv, db = b - a;
        return make_uint4((uint32_t)da, (uint32_t)(da >> 32), (uint32_t)db, (uint32_t)(db >> 32));
    } else {
        uint32_t d[4], pv = first ? 0u : p1 >> 16;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t lo = c[i] & 0xFFFFu, hi = c[i] >> 16;
            d[i] = ((lo - pv) & 0xFFFFu) | ((hi - lo) << 16);
            pv = hi;
        }
        return make_uint4(d[0], d[1], d[2], d[3]);
    }
}

// ---------------------------------------------------------------------------
// forward: elements [i0, i0 + cnt) of a segment whose q whole elements start at `in`; i0 is a multiple of RUN
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__device__ __forceinline__ void dl_tile_forward(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t *raw, uint32_t *img)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t SH = 4 + G::LG;                         // log2 of the bytes between two pad dwords
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long A = (unsigned long long)(uintptr_t)in + i0 * ELEM, A0 = A & ~15ull;
    const uint32_t s = (uint32_t)(A - A0);
    const uint32_t ng = (s + cnt * ELEM + 15) / 16;            // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS)
        reinterpret_cast<uint4 *>(raw + 4)[g] = *reinterpret_cast<const uint4 *>(in + ((long long)(i0 * ELEM) - (long long)s) + 16ull * g);
    __syncthreads();
    // tile bytes [16 g, 16 g + 16) are raw bytes s + 16 g ..: dwords (s + 16 g) / 4 - 2 .. + 4, shifted down by s mod 4 bytes
    const uint32_t nge = (cnt * ELEM + 15) / 16, sb = s & 3;   // nge <= 1024
    for (uint32_t g = tid; g < nge; g += SH_THREADS) {
        const uint32_t *p = raw + 4 + ((s + 16 * g) >> 2);
        uint32_t w[7], c[4];
#pragma unroll
        for (int m = 0; m < 7; m++) w[m] = (ELEM == 8 || m > 0) ? p[m - 2] : 0u;
        const uint32_t p0 = ELEM == 8 ? __builtin_amdgcn_alignbyte(w[1], w[0], sb) : 0u;
        const uint32_t p1 = __builtin_amdgcn_alignbyte(w[2], w[1], sb);
#pragma unroll
        for (int m = 0; m < 4; m++) c[m] = __builtin_amdgcn_alignbyte(w[m + 3], w[m + 2], sb);
        const uint4 d = dl_differences<ELEM>(c, p0, p1, (g & (DL_RUN * ELEM / 16 - 1)) == 0);
        uint32_t *dst = img + 4 * g + (g >> G::LG);
        dst[0] = d.x; dst[1] = d.y; dst[2] = d.z; dst[3] = d.w;
    }
    __syncthreads();
    // planes from the padded image, as shuffle.hip's forward tile at s = 0: byte B = ELEM e + j lies at B + 4 * (B >> SH)
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

// ---------------------------------------------------------------------------
// inverse: plane j of the input starts at in + j q; elements [i0, i0 + cnt) go to out + i0 ELEM
// ---------------------------------------------------------------------------
template <uint32_t ELEM> struct DlAcc { using T = uint32_t; };
template <> struct DlAcc<8> { using T = unsigned long long; };

// inclusive sum over the wave in six DPP steps: within rows of 16 lanes by shifts of 1, 2, 4 and 8 (lanes without a source add
// 0), then lane 15 of rows 0 and 2 into rows 1 and 3, then lane 31 into the upper half.  VALU only; a 64-bit value moves as
// its two dwords and is added as one (add / add-with-carry).
template <uint32_t CTRL, uint32_t ROWS>
__device__ __forceinline__ uint32_t dl_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, false);
}
template <uint32_t CTRL, uint32_t ROWS>
__device__ __forceinline__ unsigned long long dl_dpp(unsigned long long v)
{
    return dl_dpp<CTRL, ROWS>((uint32_t)v) | ((unsigned long long)dl_dpp<CTRL, ROWS>((uint32_t)(v >> 32)) << 32);
}
template <class A>
__device__ __forceinline__ A dl_wave_inclusive(A v)
{
    v += dl_dpp<0x111, 0xF>(v);                                // row_shr:1
    v += dl_dpp<0x112, 0xF>(v);                                // row_shr:2
    v += dl_dpp<0x114, 0xF>(v);                                // row_shr:4
    v += dl_dpp<0x118, 0xF>(v);                                // row_shr:8
    v += dl_dpp<0x142, 0xA>(v);                                // row_bcast:15 into rows 1 and 3
    v += dl_dpp<0x143, 0xC>(v);                                // row_bcast:31 into rows 2 and 3
    return v;
}

template <uint32_t ELEM>
__device__ __forceinline__ void dl_tile_inverse(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t *reg, uint32_t *flat, typename DlAcc<ELEM>::T *wt)
{
    using G = ShGeom<ELEM>;
    using Acc = typename DlAcc<ELEM>::T;
    constexpr uint32_t E = 16 / ELEM;                          // elements of a granule
    constexpr uint32_t PPR = ELEM / 2;                         // passes of the workgroup that make one run
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *regb = reinterpret_cast<const uint8_t *>(reg);
    const unsigned long long I = (unsigned long long)(uintptr_t)in + i0;      // plane 0's run
    for (uint32_t t = tid; t < ELEM * G::NGP; t += SH_THREADS) {
        const uint32_t j = t / G::NGP, g = t - j * G::NGP;
        const unsigned long long A = I + j * q, A0 = A & ~15ull;
        if (g < ((uint32_t)(A - A0) + cnt + 15) / 16)
            reinterpret_cast<uint4 *>(reg)[t] = *reinterpret_cast<const uint4 *>(in + ((long long)(i0 + j * q) - (long long)(A - A0)) + 16ull * g);
    }
    __syncthreads();
    auto plane_base = [&](uint32_t j) { return 16 * G::NGP * j + (((uint32_t)I + j * (uint32_t)q) & 15u); };
    // v[k]: the lane's granule of pass k, summed within the lane; ex[k]: the sum of the lanes in front within the wave
    Acc v[DL_PASSES][E], ex[DL_PASSES];
#pragma unroll
    for (uint32_t k = 0; k < DL_PASSES; k++) {
        const uint32_t e0 = (tid + SH_THREADS * k) * E;        // the granule's first element within the tile
        uint32_t b[16];
#pragma unroll
        for (uint32_t m = 0; m < 16; m++) b[m] = regb[e0 + plane_base(m & (ELEM - 1)) + (m >> G::LG)];
#pragma unroll
        for (uint32_t i = 0; i < E; i++) {
            Acc x = 0;
#pragma unroll
            for (uint32_t m = 0; m < ELEM; m++) x |= (Acc)b[ELEM * i + m] << (8 * m);
            v[k][i] = i ? v[k][i - 1] + x : x;
        }
        const Acc incl = dl_wave_inclusive<Acc>(v[k][E - 1]);
        ex[k] = incl - v[k][E - 1];
        if (lane == 63) wt[4 * k + wave] = incl;
    }
    __syncthreads();
    Acc run = 0;
#pragma unroll
    for (uint32_t k = 0; k < DL_PASSES; k++) {
        if (k % PPR == 0) run = 0;                             // (a run starts with this pass)
        Acc carry = run + ex[k];
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            const Acc t = wt[4 * k + w];
            if (w < wave) carry += t;
            run += t;
        }
        uint32_t o[4];
        if constexpr (ELEM == 8) {
#pragma unroll
            for (uint32_t i = 0; i < 2; i++) { const Acc x = v[k][i] + carry; o[2 * i] = (uint32_t)x; o[2 * i + 1] = (uint32_t)(x >> 32); }
        } else if constexpr (ELEM == 4) {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) o[i] = v[k][i] + carry;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) o[i] = ((v[k][2 * i] + carry) & 0xFFFFu) | ((v[k][2 * i + 1] + carry) << 16);
        }
        reinterpret_cast<uint4 *>(flat)[tid + SH_THREADS * k] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    const uint8_t *flatb = reinterpret_cast<const uint8_t *>(flat);
    const unsigned long long O = (unsigned long long)(uintptr_t)out + i0 * ELEM;
    const ShRun r = sh_run(O, cnt * ELEM);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (i0 * ELEM + r.head));
    const uint32_t hb = r.head & 3;
    for (uint32_t h = tid; h < r.nf; h += SH_THREADS) {        // tile bytes [head + 16 h, + 16): five dwords, shifted by head mod 4
        const uint32_t *p = flat + ((r.head + 16 * h) >> 2);
        uint32_t w[5];
#pragma unroll
        for (int m = 0; m < 5; m++) w[m] = p[m];
        dst[h] = make_uint4(__builtin_amdgcn_alignbyte(w[1], w[0], hb), __builtin_amdgcn_alignbyte(w[2], w[1], hb),
                            __builtin_amdgcn_alignbyte(w[3], w[2], hb), __builtin_amdgcn_alignbyte(w[4], w[3], hb));
    }
    if (tid < 32) {
        const bool is_head = tid < 16;
        const uint32_t y = tid & 15;
        if (y < (is_head ? r.head : r.tail)) {
            const uint32_t p = is_head ? y : r.head + 16 * r.nf + y;
            out[i0 * ELEM + p] = flatb[p];
        }
    }
}

template <uint32_t ELEM, bool INVERSE>
__global__ __launch_bounds__(SH_THREADS) void k_delta_shuffle(const uint8_t *in, uint8_t *out, unsigned long long len)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t WORDS_A = INVERSE ? DL_REGION_WORDS : DL_RAW_WORDS, WORDS_B = INVERSE ? DL_FLAT_WORDS : DL_IMG_WORDS;
    __shared__ __attribute__((aligned(16))) uint32_t ldsA[WORDS_A];
    __shared__ __attribute__((aligned(16))) uint32_t ldsB[WORDS_B];
    __shared__ typename DlAcc<ELEM>::T wt[INVERSE ? 4 * DL_PASSES : 1];
    static_assert(DL_REGION_WORDS * 4 >= 16 * G::NGP * ELEM, "inverse regions fit");
    static_assert(G::TQ % DL_RUN == 0 && (DL_RUN * ELEM) % (16 * SH_THREADS) == 0, "runs, tiles and passes nest");
    const unsigned long long q = len / ELEM, nt = q ? (q + G::TQ - 1) / G::TQ : 1;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, q - i0);
        if (cnt) {
            if constexpr (INVERSE) dl_tile_inverse<ELEM>(in, out, q, i0, cnt, ldsA, ldsB, wt);
            else dl_tile_forward<ELEM>(in, out, q, i0, cnt, ldsA, ldsB);
        }
        if (t + 1 == nt && threadIdx.x < (uint32_t)(len - q * ELEM)) out[q * ELEM + threadIdx.x] = in[q * ELEM + threadIdx.x];
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

template <uint32_t ELEM>
static hipError_t dl_launch(hipStream_t st, bool inverse, uint32_t grid, const uint8_t *in, uint8_t *out, unsigned long long len)
{
    if (inverse) hipLaunchKernelGGL((k_delta_shuffle<ELEM, true>), dim3(grid), dim3(SH_THREADS), 0, st, in, out, len);
    else hipLaunchKernelGGL((k_delta_shuffle<ELEM, false>), dim3(grid), dim3(SH_THREADS), 0, st, in, out, len);
    return hipGetLastError();
}

hipError_t delta_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, bool inverse)
{
    if (len == 0) return hipSuccess;
    const unsigned long long tq = SH_TILE / elem, q = len / elem, nt = q ? (q + tq - 1) / tq : 1;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(nt, 1u << 24);     // (one workgroup per tile up to 256 GiB)
    switch (elem) {
    case 2: return dl_launch<2>(st, inverse, grid, in, out, len);
    case 4: return dl_launch<4>(st, inverse, grid, in, out, len);
    case 8: return dl_launch<8>(st, inverse, grid, in, out, len);
    default: return hipErrorInvalidValue;
    }
}

// the range form of the inverse (see k_unshuffle_range): `first` is a multiple of RUN, so every tile still starts a run, and
// the sums of a tile never depended on anything in front of it
template <uint32_t ELEM>
__global__ __launch_bounds__(SH_THREADS) void k_undelta_unshuffle_range(const uint8_t *in, uint8_t *out, unsigned long long q,
                                                                        unsigned long long first, unsigned long long count)
{
    using G = ShGeom<ELEM>;
    __shared__ __attribute__((aligned(16))) uint32_t reg[DL_REGION_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t flat[DL_FLAT_WORDS];
    __shared__ typename DlAcc<ELEM>::T wt[4 * DL_PASSES];
    uint8_t *base = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out) - first * ELEM);
    const unsigned long long nt = (count + G::TQ - 1) / G::TQ;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = first + t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, first + count - i0);
        dl_tile_inverse<ELEM>(in, base, q, i0, cnt, reg, flat, wt);
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

hipError_t undelta_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                          unsigned long long first, unsigned long long count)
{
    if (count == 0) return hipSuccess;
    if (first % DL_RUN) return hipErrorInvalidValue;
    const unsigned long long tq = SH_TILE / elem, nt = (count + tq - 1) / tq;
    const dim3 grid((uint32_t)std::min<unsigned long long>(nt, 1u << 24)), block(SH_THREADS);
    switch (elem) {
    case 2: hipLaunchKernelGGL(k_undelta_unshuffle_range<2>, grid, block, 0, st, in, out, q, first, count); break;
    case 4: hipLaunchKernelGGL(k_undelta_unshuffle_range<4>, grid, block, 0, st, in, out, q, first, count); break;
    case 8: hipLaunchKernelGGL(k_undelta_unshuffle_range<8>, grid, block, 0, st, in, out, q, first, count); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace glc
