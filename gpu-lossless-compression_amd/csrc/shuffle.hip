// shuffle.hip -- the byte-plane shuffle filter of the BWT container (format version 2): for elements of
// ELEM = 2, 4 or 8 bytes, out[j * q + i] = in[i * ELEM + j] over the q whole elements of a segment, the last len % ELEM
// bytes copied in place; and its inverse.  A bandwidth kernel: one read and one write per byte, both as 16 bytes per lane.
//
// A workgroup of four waves takes a tile of 16 KiB of element bytes (TQ = 16384 / ELEM elements) through LDS:
//   forward   the tile's input, one contiguous range of any byte alignment, is read as the address-aligned 16-byte granules
//             that cover it (one global_load_dwordx4 per lane and granule, consecutive lanes consecutive granules) and
//             stored to LDS; then every lane builds whole 16-byte granules of one plane's output run -- 16 LDS byte reads,
//             ELEM bytes apart in the tile image -- and writes each with one 16-byte store, consecutive lanes consecutive
//             granules of the same plane, so a wave's store covers 1 KiB of one plane;
//   inverse   the ELEM plane runs of the tile are read the same way into ELEM regions of LDS, and every lane builds whole
//             granules of the tile's single output run.
// Runs start at arbitrary byte addresses (plane starts j * q are what they are): the up to 15 bytes in front of a run's first
// aligned granule and the up to 15 behind its last are peeled off and written as bytes by one pass of the workgroup; the
// body never is.  An aligned granule that holds one byte of a buffer lies in that byte's page, so the covering loads touch
// no page the caller did not pass; stores write exactly the bytes of the segment.
//
// LDS banks.  Forward: lane l reads byte c + ELEM * (16 l + k) of the tile image in step k, a lane stride of 16 * ELEM bytes
// -- 2 banks for all 32 lanes of a group if the image were stored flat.  The image is stored with one pad dword behind every
// ELEM granules, which makes the lane stride 4 * ELEM + 1 dwords: odd, so conflict-free.  The pad a lane's byte needs is
// B / (16 * ELEM) dwords and B mod (16 * ELEM) is the same in every lane of a plane, so the per-step offset is a scalar.
// Inverse: lanes read 16 / ELEM consecutive bytes of one plane region per step: consecutive dwords (2-way for ELEM = 2).
//
// Work is dealt out as a list of tiles over all segments of a call: workgroup w takes tiles w, w + grid, ...; every
// workgroup walks the segment lengths itself (scalar loads; O(count) per workgroup).  The single-segment form launches one
// workgroup per tile, the batched form (lengths on the device only) a fixed grid.  Offsets are 64-bit throughout.
#include "shuffle_tile.h"

namespace glc {

// ---------------------------------------------------------------------------
// forward: elements [i0, i0 + cnt) of a segment whose q whole elements start at `in`; plane j of the output starts at out + j q
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__device__ __forceinline__ void sh_tile_forward(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t *lds)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t SH = 4 + G::LG;                         // log2 of the bytes between two pad dwords
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *ldsb = reinterpret_cast<const uint8_t *>(lds);
    const unsigned long long A = (unsigned long long)(uintptr_t)in + i0 * ELEM, A0 = A & ~15ull;
    const uint32_t s = (uint32_t)(A - A0);
    const uint32_t ng = (s + cnt * ELEM + 15) / 16;            // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + ((long long)(i0 * ELEM) - (long long)s) + 16ull * g);
        uint32_t *d = lds + 4 * g + (g >> G::LG);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    // byte B of the tile image (B = s + ELEM * e + j for element e, plane j) lies at B + 4 * (B >> SH) of the padded image
#pragma unroll
    for (uint32_t pp = 0; pp < G::PPW; pp++) {
        const uint32_t j = G::WPP > 1 ? wave % ELEM : wave + 4 * pp;
        const uint32_t sub = G::WPP > 1 ? wave / ELEM : 0;
        const unsigned long long O = (unsigned long long)(uintptr_t)out + j * q + i0;
        const ShRun r = sh_run(O, cnt);
        const uint32_t c = s + j + ELEM * r.head;              // image byte of the first whole granule's first element
        const uint32_t ru = c & ((16u << G::LG) - 1);          // = B mod (16 ELEM) of every granule's first byte
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
    // heads and tails of the ELEM runs: up to 30 bytes each, one pass
    {
        const uint32_t j = tid >> 5, x = tid & 31;
        if (j < ELEM) {
            const unsigned long long O = (unsigned long long)(uintptr_t)out + j * q + i0;
            const ShRun r = sh_run(O, cnt);
            const bool is_head = x < 16;
            const uint32_t y = x & 15;
            if (y < (is_head ? r.head : r.tail)) {
                const uint32_t e = is_head ? y : r.head + 16 * r.nf + y;
                const uint32_t B = s + j + ELEM * e;
                out[j * q + i0 + e] = ldsb[B + 4 * (B >> SH)];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// inverse: plane j of the input starts at in + j q; elements [i0, i0 + cnt) go to out + i0 ELEM
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__device__ __forceinline__ void sh_tile_inverse(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t *lds)
{
    using G = ShGeom<ELEM>;
    const uint32_t tid = threadIdx.x;
    const uint8_t *ldsb = reinterpret_cast<const uint8_t *>(lds);
    const unsigned long long I = (unsigned long long)(uintptr_t)in + i0;      // plane 0's run
    for (uint32_t t = tid; t < ELEM * G::NGP; t += SH_THREADS) {
        const uint32_t j = t / G::NGP, g = t - j * G::NGP;
        const unsigned long long A = I + j * q, A0 = A & ~15ull;
        if (g < ((uint32_t)(A - A0) + cnt + 15) / 16)
            reinterpret_cast<uint4 *>(lds)[t] = *reinterpret_cast<const uint4 *>(in + ((long long)(i0 + j * q) - (long long)(A - A0)) + 16ull * g);
    }
    __syncthreads();
    const unsigned long long O = (unsigned long long)(uintptr_t)out + i0 * ELEM;
    const ShRun r = sh_run(O, cnt * ELEM);
    // output byte p of the run is plane p mod ELEM, element p / ELEM: region 16 NGP j, then the run's own misalignment
    auto plane_base = [&](uint32_t j) { return 16 * G::NGP * j + (((uint32_t)I + j * (uint32_t)q) & 15u); };
    uint4 *dst = reinterpret_cast<uint4 *>(out + (i0 * ELEM + r.head));
    const uint32_t rb = r.head & (ELEM - 1);                   // = p mod ELEM of every whole granule's first byte
    for (uint32_t h = tid; h < r.nf; h += SH_THREADS) {
        const uint32_t e0 = (r.head + 16 * h) >> G::LG;
        uint32_t b[16];
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) b[k] = ldsb[e0 + plane_base((rb + k) & (ELEM - 1)) + ((rb + k) >> G::LG)];
        dst[h] = sh_pack(b);
    }
    if (tid < 32) {
        const bool is_head = tid < 16;
        const uint32_t y = tid & 15;
        if (y < (is_head ? r.head : r.tail)) {
            const uint32_t p = is_head ? y : r.head + 16 * r.nf + y;
            out[i0 * ELEM + p] = ldsb[plane_base(p & (ELEM - 1)) + (p >> G::LG)];
        }
    }
}

// tiles of a segment of L bytes: one at least where there is a byte (its last tile copies the len % ELEM bytes)
template <uint32_t ELEM>
__device__ __forceinline__ unsigned long long sh_tiles(unsigned long long L)
{
    const unsigned long long q = L / ELEM, t = (q + ShGeom<ELEM>::TQ - 1) / ShGeom<ELEM>::TQ;
    return L == 0 ? 0 : (t ? t : 1);
}

// off == nullptr: one segment of one_len bytes at the bases
template <uint32_t ELEM, bool INVERSE>
__global__ __launch_bounds__(SH_THREADS) void k_shuffle(const uint8_t *inBase, uint8_t *outBase,
                                                        const unsigned long long *__restrict__ off,
                                                        const unsigned long long *__restrict__ len, uint32_t count,
                                                        unsigned long long one_len)
{
    using G = ShGeom<ELEM>;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SH_LDS_WORDS];
    static_assert(SH_LDS_WORDS * 4 >= 16 * G::NGP * ELEM + 16, "inverse regions fit");
    unsigned long long run = 0, next = blockIdx.x;
    for (uint32_t sg = 0; sg < count; sg++) {
        const unsigned long long L = off ? len[sg] : one_len, o = off ? off[sg] : 0;
        const unsigned long long nt = sh_tiles<ELEM>(L);
        const unsigned long long q = L / ELEM;
        const uint8_t *in = inBase + o;
        uint8_t *out = outBase + o;
        for (; next < run + nt; next += gridDim.x) {
            const unsigned long long i0 = (next - run) * G::TQ;
            const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, q - i0);
            if (cnt) {
                if (INVERSE) sh_tile_inverse<ELEM>(in, out, q, i0, cnt, lds);
                else sh_tile_forward<ELEM>(in, out, q, i0, cnt, lds);
            }
            if (next + 1 == run + nt && threadIdx.x < (uint32_t)(L - q * ELEM)) out[q * ELEM + threadIdx.x] = in[q * ELEM + threadIdx.x];
            __syncthreads();                                   // (the next tile of this workgroup reuses the LDS image)
        }
        run += nt;
    }
}

template <uint32_t ELEM>
static hipError_t sh_launch(hipStream_t st, bool inverse, uint32_t grid, const uint8_t *in, uint8_t *out,
                            const unsigned long long *d_off, const unsigned long long *d_len, uint32_t count, unsigned long long one_len)
{
    if (inverse) hipLaunchKernelGGL((k_shuffle<ELEM, true>), dim3(grid), dim3(SH_THREADS), 0, st, in, out, d_off, d_len, count, one_len);
    else hipLaunchKernelGGL((k_shuffle<ELEM, false>), dim3(grid), dim3(SH_THREADS), 0, st, in, out, d_off, d_len, count, one_len);
    return hipGetLastError();
}

static hipError_t sh_dispatch(hipStream_t st, bool inverse, uint32_t elem, uint32_t grid, const uint8_t *in, uint8_t *out,
                              const unsigned long long *d_off, const unsigned long long *d_len, uint32_t count, unsigned long long one_len)
{
    switch (elem) {
    case 2: return sh_launch<2>(st, inverse, grid, in, out, d_off, d_len, count, one_len);
    case 4: return sh_launch<4>(st, inverse, grid, in, out, d_off, d_len, count, one_len);
    case 8: return sh_launch<8>(st, inverse, grid, in, out, d_off, d_len, count, one_len);
    default: return hipErrorInvalidValue;
    }
}

hipError_t shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, bool inverse)
{
    if (len == 0) return hipSuccess;
    const unsigned long long tq = SH_TILE / elem, q = len / elem, nt = q ? (q + tq - 1) / tq : 1;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(nt, 1u << 24);     // (one workgroup per tile up to 256 GiB)
    return sh_dispatch(st, inverse, elem, grid, in, out, nullptr, nullptr, 1, len);
}

// ---------------------------------------------------------------------------
// the range form of the inverse: elements [first, first + count) of a segment with plane stride q, to out[0 .. count ELEM).
// The inverse tile takes any i0 (a plane run starts where it starts), so tile t is simply elements first + t TQ ..; it
// addresses its output as base + i0 ELEM, which makes the base out - first ELEM.  Nothing of the tile function changes: the
// loads are the aligned granules that cover the ELEM plane runs of the tile, the stores exactly the tile's output bytes.
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__global__ __launch_bounds__(SH_THREADS) void k_unshuffle_range(const uint8_t *in, uint8_t *out, unsigned long long q,
                                                                unsigned long long first, unsigned long long count)
{
    using G = ShGeom<ELEM>;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SH_LDS_WORDS];
    uint8_t *base = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out) - first * ELEM);
    const unsigned long long nt = (count + G::TQ - 1) / G::TQ;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = first + t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, first + count - i0);
        sh_tile_inverse<ELEM>(in, base, q, i0, cnt, lds);
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS image)
    }
}

hipError_t unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                  unsigned long long first, unsigned long long count)
{
    if (count == 0) return hipSuccess;
    const unsigned long long tq = SH_TILE / elem, nt = (count + tq - 1) / tq;
    const dim3 grid((uint32_t)std::min<unsigned long long>(nt, 1u << 24)), block(SH_THREADS);
    switch (elem) {
    case 2: hipLaunchKernelGGL(k_unshuffle_range<2>, grid, block, 0, st, in, out, q, first, count); break;
    case 4: hipLaunchKernelGGL(k_unshuffle_range<4>, grid, block, 0, st, in, out, q, first, count); break;
    case 8: hipLaunchKernelGGL(k_unshuffle_range<8>, grid, block, 0, st, in, out, q, first, count); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t shuffle_segments(hipStream_t st, const uint8_t *inBase, uint8_t *outBase, const unsigned long long *d_off,
                            const unsigned long long *d_len, uint32_t count, uint32_t elem, bool inverse)
{
    if (count == 0) return hipSuccess;
    return sh_dispatch(st, inverse, elem, SH_BATCH_GRID, inBase, outBase, d_off, d_len, count, 0);
}

} // namespace glc
