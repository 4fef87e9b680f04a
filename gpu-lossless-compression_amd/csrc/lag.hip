// lag.hip -- the lagged, folded delta of the container's typed-data filter (INTEGRATION.md 4b "Delta: lag and fold", format
// version 11): delta.hip's fused delta + shuffle with the predecessor LAG elements back instead of one, for interleaved channels,
// and the difference's sign optionally folded into bit 0 (zigzag), so that the upper planes of a small difference of either sign
// are zero.  With x[i] element i of a segment as a little-endian unsigned integer of ELEM = 2, 4 or 8 bytes, W = 8 ELEM,
// RUN = 2048 elements, 1 <= LAG <= 16 and r = i mod RUN:
//   forward   d[i] = x[i] where r < LAG, else x[i] - x[i - LAG] (mod 2^W); f[i] = d[i], or with the fold
//             (d[i] << 1) ^ (0 - (d[i] >> (W - 1))); out[j q + i] = byte j of f[i]
//   inverse   the planes gathered back into f; d = (f >> 1) ^ (0 - (f & 1)); x[i] = d[i] + d[i - LAG] + d[i - 2 LAG] + ... down to
//             the member of the chain with r < LAG
// over the q = len / ELEM whole elements, the last len % ELEM bytes copied in place.  (LAG, fold) = (1, 0) is delta.hip's
// transform; the host entries below hand that setting to delta.hip's kernels, which stay as they are.
//
// The geometry is delta.hip's: one workgroup of 256 lanes per 16 KiB tile, a tile holds whole runs, so nothing in front of a
// tile is ever read and no workgroup waits for another; aligned 16-byte granule loads at any alignment of the buffers; the
// plane build with its head / body / tail stores; single segment, 64-bit offsets.  The element-wise arithmetic on granules, the
// LDS read at any byte and the plane build are lag_tile.h's, which grid.hip's forward shares.
//
// Forward, one tile: the raw image as in delta.hip, with 32 words in front of it: the predecessors of a granule are the 16 bytes
// LAG ELEM <= 128 bytes in front of it, taken like the granule itself as five aligned dwords and v_alignbyte.  An element with
// r < LAG -- run-relative byte below LAG ELEM -- subtracts 0 instead (what was read for it is the previous run's tail or the
// slack, never global memory in front of the tile).  The fold is a shift and an xor per element, on dword pairs for ELEM 8 and
// on packed halves for ELEM 2.  The differences go to the padded image, from which the planes are built as in delta.hip.
// Inverse, one tile: the plane regions as in delta.hip; every lane reassembles its four granules, undoes the fold and keeps them
// in registers.  The sums down the columns of a run (rows of LAG elements) are a Kogge-Stone scan over the flat image of the
// tile at element strides LAG, 2 LAG, 4 LAG, ... below RUN (7 to 11 rounds): a round adds to every granule the 16 bytes
// stride * ELEM bytes in front of it, element by element where the run-relative byte is at least that distance, so a chain
// never leaves its run and the short last row of a run (RUN % LAG != 0) needs no case of its own.  The rounds go from one LDS
// image to the other (the plane regions' space is the second image once the granules are in registers): one read, one write
// and one barrier each.  Where the distance is a multiple of 16 bytes the read is one ds_read_b128 and the mask is the whole
// granule's; the first rounds of small lags take five dwords and v_alignbyte.  Output granules are cut from the last image as in
// delta.hip.
//
// LDS: forward 34960 bytes (raw image 16528, padded image 18432), inverse 32928 bytes: four workgroups per CU each.
#include "lag_tile.h"

namespace glc {

constexpr uint32_t LG_MAX_LAG = 16;
constexpr uint32_t LG_PASSES = SH_TILE / 16 / SH_THREADS;      // element-aligned granules of a tile per lane
constexpr uint32_t LG_RAW_FRONT = LG_MAX_LAG * 8 / 4;          // forward: words in front of the raw image, the longest way back
constexpr uint32_t LG_RAW_WORDS = LG_RAW_FRONT + 4 * SH_NGI;
constexpr uint32_t LG_REGION_WORDS = SH_TILE / 4 + 4 * 8;      // inverse: ELEM plane regions of 16 NGP bytes; then the second image
constexpr uint32_t LG_FRONT = 4;                               // inverse: words in front of an image (a masked read may start 15 bytes early)
constexpr uint32_t LG_FLAT_WORDS = LG_FRONT + SH_TILE / 4 + 4; // and one granule of slack behind it for the output cut
static_assert(LG_PASSES == 4, "four passes of 256 lanes cover a tile");
static_assert(LG_REGION_WORDS >= LG_FLAT_WORDS, "the regions' space holds an image");

// ---------------------------------------------------------------------------
// forward: elements [i0, i0 + cnt) of a segment whose q whole elements start at `in`; i0 is a multiple of RUN
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__device__ __forceinline__ void lg_tile_forward(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t lag, uint32_t fold, uint32_t *raw, uint32_t *img)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long A = (unsigned long long)(uintptr_t)in + i0 * ELEM, A0 = A & ~15ull;
    const uint32_t s = (uint32_t)(A - A0);
    const uint32_t ng = (s + cnt * ELEM + 15) / 16;            // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS)
        reinterpret_cast<uint4 *>(raw + LG_RAW_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + ((long long)(i0 * ELEM) - (long long)s) + 16ull * g);
    __syncthreads();
    // tile bytes [16 g, 16 g + 16) are raw bytes s + 16 g ..; their predecessors lie dist bytes in front of them
    const uint32_t nge = (cnt * ELEM + 15) / 16, dist = lag * ELEM;   // nge <= 1024, dist <= 4 * LG_RAW_FRONT
    for (uint32_t g = tid; g < nge; g += SH_THREADS) {
        uint32_t c[4], p[4];
        lg_read16(raw + LG_RAW_FRONT, (int)(s + 16 * g), c);
        lg_read16(raw + LG_RAW_FRONT, (int)(s + 16 * g) - (int)dist, p);
        lg_mask<ELEM>(p, (16 * g) & (LG_RUN * ELEM - 1), dist);
        lg_combine<ELEM, true>(c, p);
        lg_fold<ELEM, false>(c, fold);
        lg_img_store<ELEM>(img, g, c);
    }
    __syncthreads();
    lg_planes<ELEM>(img, out, q, i0, cnt, tid, lane, wave);
}

// ---------------------------------------------------------------------------
// inverse: plane j of the input starts at in + j q; elements [i0, i0 + cnt) go to out + i0 ELEM
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__device__ __forceinline__ void lg_tile_inverse(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t lag, uint32_t fold, uint32_t *reg, uint32_t *flat)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t E = 16 / ELEM;                          // elements of a granule
    const uint32_t tid = threadIdx.x;
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
    // v[k]: the lane's granule tid + 256 k, unfolded; it stays in registers through the rounds
    uint32_t v[LG_PASSES][4];
    uint32_t *cur = flat + LG_FRONT, *nxt = reg + LG_FRONT;
#pragma unroll
    for (uint32_t k = 0; k < LG_PASSES; k++) {
        const uint32_t e0 = (tid + SH_THREADS * k) * E;        // the granule's first element within the tile
        uint32_t b[16];
#pragma unroll
        for (uint32_t m = 0; m < 16; m++) b[m] = regb[e0 + plane_base(m & (ELEM - 1)) + (m >> G::LG)];
#pragma unroll
        for (uint32_t m = 0; m < 4; m++) v[k][m] = b[4 * m] | (b[4 * m + 1] << 8) | (b[4 * m + 2] << 16) | (b[4 * m + 3] << 24);
        lg_fold<ELEM, true>(v[k], fold);
        reinterpret_cast<uint4 *>(cur)[tid + SH_THREADS * k] = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
    }
    __syncthreads();                                           // (the regions are free from here on)
    for (uint32_t st = lag; st < LG_RUN; st <<= 1) {
        const uint32_t dist = st * ELEM;
#pragma unroll
        for (uint32_t k = 0; k < LG_PASSES; k++) {
            const uint32_t g = tid + SH_THREADS * k, gb = (16 * g) & (LG_RUN * ELEM - 1);
            if (gb + 16 > dist) {                              // (else every element of the granule is within `st` of its run's start)
                uint32_t p[4];
                if ((dist & 15) == 0) {
                    const uint4 t = reinterpret_cast<const uint4 *>(cur)[g - dist / 16];
                    p[0] = t.x; p[1] = t.y; p[2] = t.z; p[3] = t.w;
                } else {
                    lg_read16(cur, (int)(16 * g) - (int)dist, p);
                    lg_mask<ELEM>(p, gb, dist);
                }
                lg_combine<ELEM, false>(v[k], p);
            }
            reinterpret_cast<uint4 *>(nxt)[g] = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
        }
        __syncthreads();
        uint32_t *t = cur; cur = nxt; nxt = t;
    }
    const uint8_t *flatb = reinterpret_cast<const uint8_t *>(cur);
    const unsigned long long O = (unsigned long long)(uintptr_t)out + i0 * ELEM;
    const ShRun r = sh_run(O, cnt * ELEM);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (i0 * ELEM + r.head));
    for (uint32_t h = tid; h < r.nf; h += SH_THREADS) {        // tile bytes [head + 16 h, + 16)
        uint32_t o[4];
        lg_read16(cur, (int)(r.head + 16 * h), o);
        dst[h] = make_uint4(o[0], o[1], o[2], o[3]);
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
__global__ __launch_bounds__(SH_THREADS) void k_lag_shuffle(const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t lag, uint32_t fold)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t WORDS_A = INVERSE ? LG_REGION_WORDS : LG_RAW_WORDS, WORDS_B = INVERSE ? LG_FLAT_WORDS : LG_IMG_WORDS;
    __shared__ __attribute__((aligned(16))) uint32_t ldsA[WORDS_A];
    __shared__ __attribute__((aligned(16))) uint32_t ldsB[WORDS_B];
    static_assert(LG_REGION_WORDS * 4 >= 16 * G::NGP * ELEM, "inverse regions fit");
    static_assert(G::TQ % LG_RUN == 0, "a tile holds whole runs");
    const unsigned long long q = len / ELEM, nt = q ? (q + G::TQ - 1) / G::TQ : 1;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, q - i0);
        if (cnt) {
            if constexpr (INVERSE) lg_tile_inverse<ELEM>(in, out, q, i0, cnt, lag, fold, ldsA, ldsB);
            else lg_tile_forward<ELEM>(in, out, q, i0, cnt, lag, fold, ldsA, ldsB);
        }
        if (t + 1 == nt && threadIdx.x < (uint32_t)(len - q * ELEM)) out[q * ELEM + threadIdx.x] = in[q * ELEM + threadIdx.x];
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

template <uint32_t ELEM>
static hipError_t lg_launch(hipStream_t st, bool inverse, uint32_t grid, const uint8_t *in, uint8_t *out, unsigned long long len,
                            uint32_t lag, uint32_t fold)
{
    if (inverse) hipLaunchKernelGGL((k_lag_shuffle<ELEM, true>), dim3(grid), dim3(SH_THREADS), 0, st, in, out, len, lag, fold);
    else hipLaunchKernelGGL((k_lag_shuffle<ELEM, false>), dim3(grid), dim3(SH_THREADS), 0, st, in, out, len, lag, fold);
    return hipGetLastError();
}

hipError_t lag_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, uint32_t lag,
                              uint32_t fold, bool inverse)
{
    if (lag < 1 || lag > LG_MAX_LAG || fold > 1) return hipErrorInvalidValue;
    if (lag == 1 && !fold) return delta_shuffle_device(st, in, out, len, elem, inverse);      // (the plain delta keeps its kernels)
    if (len == 0) return hipSuccess;
    const unsigned long long tq = SH_TILE / elem, q = len / elem, nt = q ? (q + tq - 1) / tq : 1;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(nt, 1u << 24);     // (one workgroup per tile up to 256 GiB)
    switch (elem) {
    case 2: return lg_launch<2>(st, inverse, grid, in, out, len, lag, fold);
    case 4: return lg_launch<4>(st, inverse, grid, in, out, len, lag, fold);
    case 8: return lg_launch<8>(st, inverse, grid, in, out, len, lag, fold);
    default: return hipErrorInvalidValue;
    }
}

// the range form of the inverse (see k_undelta_unshuffle_range): `first` is a multiple of RUN, so every tile still starts a run
template <uint32_t ELEM>
__global__ __launch_bounds__(SH_THREADS) void k_unlag_unshuffle_range(const uint8_t *in, uint8_t *out, unsigned long long q,
                                                                      unsigned long long first, unsigned long long count, uint32_t lag,
                                                                      uint32_t fold)
{
    using G = ShGeom<ELEM>;
    __shared__ __attribute__((aligned(16))) uint32_t reg[LG_REGION_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t flat[LG_FLAT_WORDS];
    uint8_t *base = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out) - first * ELEM);
    const unsigned long long nt = (count + G::TQ - 1) / G::TQ;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = first + t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, first + count - i0);
        lg_tile_inverse<ELEM>(in, base, q, i0, cnt, lag, fold, reg, flat);
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

hipError_t unlag_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                        uint32_t lag, uint32_t fold, unsigned long long first, unsigned long long count)
{
    if (lag < 1 || lag > LG_MAX_LAG || fold > 1) return hipErrorInvalidValue;
    if (lag == 1 && !fold) return undelta_unshuffle_range_device(st, in, out, q, elem, first, count);
    if (count == 0) return hipSuccess;
    if (first % LG_RUN) return hipErrorInvalidValue;
    const unsigned long long tq = SH_TILE / elem, nt = (count + tq - 1) / tq;
    const dim3 grid((uint32_t)std::min<unsigned long long>(nt, 1u << 24)), block(SH_THREADS);
    switch (elem) {
    case 2: hipLaunchKernelGGL(k_unlag_unshuffle_range<2>, grid, block, 0, st, in, out, q, first, count, lag, fold); break;
    case 4: hipLaunchKernelGGL(k_unlag_unshuffle_range<4>, grid, block, 0, st, in, out, q, first, count, lag, fold); break;
    case 8: hipLaunchKernelGGL(k_unlag_unshuffle_range<8>, grid, block, 0, st, in, out, q, first, count, lag, fold); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace glc
