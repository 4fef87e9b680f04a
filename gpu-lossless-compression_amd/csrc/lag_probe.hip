// lag_probe.hip -- the lag probe (INTEGRATION.md 4b "Filter: auto with lag"; the sums, the winners, the planes and the costs are
// defined in lag_rule.h): which lag of the lagged, folded delta (lag.hip) a segment wants at each element size, and what its
// planes would cost, from two reads of it.  gfx950 / wave64.
//   k_lp_sums    the 48 sums S[e][l] of a segment.  The span geometry is k_fp_probe's: a workgroup of 256 lanes owns a span of
//                the segment, a multiple of 16 KiB, so that every restart of every element size (2048 elements: 4, 8 and 16 KiB)
//                is found from the offset alone and nothing in front of a span is read.  A span goes through LDS a 16 KiB tile
//                at a time, with 128 bytes in front of it -- sixteen elements of 8 bytes, the longest way back, as in lag.hip.
//                A lane takes 16-byte granules: the granule and the 128 bytes in front of it come into 36 registers, and every
//                one of the 32 distinct distances l * e is a fixed register (for an odd lag of 2-byte elements a v_alignbyte of
//                two), so the 224 (element, lag) pairs of a granule are a subtract, the fold, a count of leading zeros and an
//                add each.  An element whose run-relative index is below l takes no predecessor: the window's bytes in front
//                of the granule's run are zeroed, first for 8-byte elements, then for 4, then for 2 -- the runs nest, so the
//                zeroing does.  What was read there is the slack or the previous run, never memory in front of the segment.
//                48 accumulators of 32 bits a lane (a lane's share of the largest span, 2 MiB, is 2^16 bits a sum); they leave
//                by a wave reduction, LDS, and one 64-bit global atomic per (workgroup, sum).  16-byte loads where the
//                segment's address allows, a byte path where it does not.
//   k_lp_argmin  the three winners of a segment from its sums, so that the host is not involved between the two probes.
//   k_lp_planes  the 14 histograms of a segment for three lags read from device memory, each used as ((v - 1) & 15) + 1: a bad
//                word cannot take the kernel out of its tile.  The tiles are k_lp_sums'; the predecessors of a granule are the
//                16 bytes lag * e bytes in front of it (lag_tile.h's read, mask, subtract and fold).  The LDS counter copies
//                and the uniform shortcut are k_fp_probe's: a wave whose lanes hold one value at a byte position adds 64 once
//                -- the upper planes of a good lag are almost all zero, so without it every lane lands on one counter.
//   k_lp_cost    the three costs of a segment from its 14 rows: one wave per plane, as k_fp_cost.  The grid probe
//                (grid_probe.hip) runs it over its own rows, with the width words that say which element sizes have a candidate.
// Any segment length up to 2^31, any byte alignment; only the first L - L % 8 bytes are counted.
#include "container_internal.h"
#include "glc_device.h"
#include "grid_rule.h"
#include "lag_rule.h"
#include "lag_tile.h"
#include "plane_hist.h"

namespace glc {

constexpr uint32_t LP_THREADS = 256, LP_PASS = 1024, LP_TILE = 16384;
constexpr uint32_t LP_FRONT = LAG_MAX * 8 / 4;                 // words in front of a tile's image: the longest way back
constexpr uint32_t LP_RAW_WORDS = LP_FRONT + LP_TILE / 4;
constexpr uint32_t LP_WINDOW = LP_FRONT + 4;                   // a granule and what lies in front of it, in dwords
constexpr uint32_t LP_MIN_SPAN = 4 * LP_TILE, LP_MAX_SPANS = 1024;
constexpr uint32_t LP_COPIES = 2, LP_PITCH = 257, LP_COPY_WORDS = LAG_ROWS * LP_PITCH;
constexpr uint32_t LP_PLANE_WAVES = 8;
static_assert(LP_TILE % (FILTER_RUN * 8) == 0 && FILTER_RUN == LG_RUN, "a tile holds whole runs of every element size");

__device__ __forceinline__ uint32_t lp_len(const unsigned long long *len, uint32_t i, uint32_t max_len)
{
    const unsigned long long l = len[i];
    return (l > max_len ? max_len : (uint32_t)l) & ~7u;
}

// eight bytes at p as two dwords
__device__ __forceinline__ uint2 lp_load8(const uint8_t *p, bool aligned)
{
    if (aligned) return *reinterpret_cast<const uint2 *>(p);
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint2(w[0], w[1]);
}

// bytes [t, t + n) of the segment at `in` (n a multiple of 8, at most a tile) to the image behind the front words of raw
__device__ __forceinline__ void lp_stage(const uint8_t *in, bool al, uint32_t t, uint32_t n, uint32_t *raw)
{
    for (uint32_t o = 16 * threadIdx.x; o < n; o += 16 * LP_THREADS) {
        uint32_t *dst = raw + LP_FRONT + o / 4;
        if (al && n - o >= 16) {
            *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(in + t + o);
        } else {
            const uint2 q = lp_load8(in + t + o, al);
            dst[0] = q.x; dst[1] = q.y;
            if (n - o >= 16) { const uint2 r = lp_load8(in + t + o + 8, al); dst[2] = r.x; dst[3] = r.y; }
        }
    }
}

// the window's dwords [FIRST, LP_FRONT) that lie in front of the run of ELEM-byte elements the granule at tile byte o is in: zero
template <uint32_t ELEM, uint32_t FIRST>
__device__ __forceinline__ void lp_zero_front(uint32_t (&w)[LP_WINDOW], uint32_t o)
{
    const uint32_t rb = o & (FILTER_RUN * ELEM - 1);           // the granule's run-relative byte, a multiple of 16
    const uint32_t z = rb < 4 * LP_FRONT ? (4 * LP_FRONT - rb) / 4 : 0u;
#pragma unroll
    for (uint32_t i = FIRST; i < LP_FRONT; i++) w[i] = i >= z ? w[i] : 0u;
}

// what the granule in w[LP_FRONT ..] (HALF: its first eight bytes) adds to the 48 sums
template <bool HALF>
__device__ __forceinline__ void lp_granule(uint32_t (&w)[LP_WINDOW], uint32_t o, uint32_t (&acc)[LAG_SUMS])
{
    constexpr uint32_t C = LP_FRONT, ND = HALF ? 2 : 4;        // the granule's first dword; its dwords that count
    lp_zero_front<8, 0>(w, o);
#pragma unroll
    for (uint32_t l = 1; l <= LAG_MAX; l++) {
#pragma unroll
        for (uint32_t m = 0; m < ND; m += 2) {
            const unsigned long long x = w[C + m] | ((unsigned long long)w[C + m + 1] << 32);
            const unsigned long long p = w[C + m - 2 * l] | ((unsigned long long)w[C + m + 1 - 2 * l] << 32);
            const unsigned long long d = x - p, f = (d << 1) ^ (0ull - (d >> 63));
            acc[2 * LAG_MAX + l - 1] += 64u - (uint32_t)__clzll((long long)f);
        }
    }
    lp_zero_front<4, LP_FRONT - 4 * LAG_MAX / 4>(w, o);
#pragma unroll
    for (uint32_t l = 1; l <= LAG_MAX; l++) {
#pragma unroll
        for (uint32_t m = 0; m < ND; m++) {
            const uint32_t d = w[C + m] - w[C + m - l], f = (d << 1) ^ (0u - (d >> 31));
            acc[LAG_MAX + l - 1] += 32u - (uint32_t)__clz((int)f);
        }
    }
    lp_zero_front<2, LP_FRONT - 2 * LAG_MAX / 4>(w, o);
    const lg_us2 one = {1, 1}, z = {0, 0}, s = {15, 15};
#pragma unroll
    for (uint32_t l = 1; l <= LAG_MAX; l++) {
#pragma unroll
        for (uint32_t m = 0; m < ND; m++) {
            // the two elements l back: a dword where l is even, else the halves of two
            const uint32_t p = l % 2 == 0 ? w[C + m - l / 2] : __builtin_amdgcn_alignbyte(w[C + m - (l - 1) / 2], w[C + m - (l + 1) / 2], 2);
            const lg_us2 d = lg_halves(w[C + m]) - lg_halves(p);
            const uint32_t f = lg_word((d << one) ^ (z - (d >> s)));
            acc[l - 1] += (32u - (uint32_t)__clz((int)(f & 0xFFFFu))) + (32u - (uint32_t)__clz((int)(f >> 16)));
        }
    }
}

__global__ __launch_bounds__(LP_THREADS) void k_lp_sums(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                        const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                        uint32_t span, unsigned long long *__restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) uint32_t raw[LP_RAW_WORDS];
    __shared__ uint32_t s_red[LP_THREADS / 64][LAG_SUMS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t P = lp_len(data_len, b, max_len);
    const unsigned long long s0 = (unsigned long long)blockIdx.y * span;
    if (s0 >= P) return;
    const uint32_t t0 = (uint32_t)s0, t1 = P - t0 > span ? t0 + span : P;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    if (tid < LP_FRONT) raw[tid] = 0;                          // (every tile starts a run of every element size: never a predecessor)
    uint32_t acc[LAG_SUMS];
#pragma unroll
    for (uint32_t i = 0; i < LAG_SUMS; i++) acc[i] = 0;
    for (uint32_t t = t0; t < t1; t += LP_TILE) {
        const uint32_t n = min(LP_TILE, t1 - t);               // a multiple of 8
        __syncthreads();                                       // (the tile before has been read)
        lp_stage(in, al, t, n, raw);
        __syncthreads();
        for (uint32_t o = 16 * tid; o < n; o += 16 * LP_THREADS) {
            uint32_t w[LP_WINDOW];
            const uint4 *src = reinterpret_cast<const uint4 *>(raw + o / 4);      // 128 bytes in front of the granule
#pragma unroll
            for (uint32_t k = 0; k < LP_WINDOW / 4; k++) {
                const uint4 q = src[k];
                w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
            }
            if (n - o >= 16) lp_granule<false>(w, o, acc);
            else lp_granule<true>(w, o, acc);
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < LAG_SUMS; i++) {
        const uint32_t v = wave_sum(acc[i]);
        if (lane == 0) s_red[wave][i] = v;
    }
    __syncthreads();
    if (tid < LAG_SUMS) {
        unsigned long long v = 0;
#pragma unroll
        for (uint32_t k = 0; k < LP_THREADS / 64; k++) v += s_red[k][tid];
        if (v) atomicAdd(&sums[(size_t)b * LAG_SUMS + tid], v);
    }
}

__global__ __launch_bounds__(64) void k_lp_argmin(const unsigned long long *__restrict__ sums, uint32_t count, uint32_t *__restrict__ lags)
{
    const uint32_t b = blockIdx.x;
    if (b >= count || threadIdx.x >= LAG_ELEMS) return;
    lags[(size_t)b * LAG_ELEMS + threadIdx.x] = lag_argmin(sums + (size_t)b * LAG_SUMS + threadIdx.x * LAG_MAX);
}

// the folded differences of the granule at tile byte o, its predecessors `lag` elements back
template <uint32_t ELEM>
__device__ __forceinline__ void lp_folded(const uint32_t *raw, uint32_t o, uint32_t lag, const uint32_t (&c)[4], uint32_t (&f)[4])
{
    uint32_t p[4];
    const uint32_t dist = lag * ELEM;                          // <= 4 * LP_FRONT
    lg_read16(raw + LP_FRONT, (int)o - (int)dist, p);
    lg_mask<ELEM>(p, o & (LG_RUN * ELEM - 1), dist);
#pragma unroll
    for (uint32_t m = 0; m < 4; m++) f[m] = c[m];
    lg_combine<ELEM, true>(f, p);
    lg_fold<ELEM, false>(f, 1);
}

__global__ __launch_bounds__(LP_THREADS) void k_lp_planes(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                          const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                          uint32_t span, const uint32_t *__restrict__ lags, uint32_t *__restrict__ planes)
{
    __shared__ __attribute__((aligned(16))) uint32_t raw[LP_RAW_WORDS];
    __shared__ uint32_t s_h[LP_COPIES * LP_COPY_WORDS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t P = lp_len(data_len, b, max_len);
    const unsigned long long s0 = (unsigned long long)blockIdx.y * span;
    if (s0 >= P) return;
    const uint32_t t0 = (uint32_t)s0, t1 = P - t0 > span ? t0 + span : P;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const uint32_t l2 = lag_clamp(lags[(size_t)b * LAG_ELEMS]), l4 = lag_clamp(lags[(size_t)b * LAG_ELEMS + 1]),
                   l8 = lag_clamp(lags[(size_t)b * LAG_ELEMS + 2]);
    if (tid < LP_FRONT) raw[tid] = 0;
    for (uint32_t i = tid; i < LP_COPIES * LP_COPY_WORDS; i += LP_THREADS) s_h[i] = 0;
    uint32_t *H = s_h + (tid & (LP_COPIES - 1)) * LP_COPY_WORDS;
    for (uint32_t t = t0; t < t1; t += LP_TILE) {
        const uint32_t n = min(LP_TILE, t1 - t);               // a multiple of 8
        __syncthreads();                                       // (the tile before has been read; the counters are zero)
        lp_stage(in, al, t, n, raw);
        __syncthreads();
        for (uint32_t o0 = wave * LP_PASS; o0 < n; o0 += 4 * LP_PASS) {
            const uint32_t o = o0 + 16 * lane;                 // o + 16 <= LP_TILE
            const uint32_t nn = o < n ? min(16u, n - o) : 0u;  // 0, 8 or 16
            const bool whole = n - o0 >= LP_PASS;              // wave-uniform
            uint32_t c[4] = {0, 0, 0, 0}, f2[4] = {0, 0, 0, 0}, f4[4] = {0, 0, 0, 0}, f8[4] = {0, 0, 0, 0};
            if (nn) {
                const uint4 q = *reinterpret_cast<const uint4 *>(raw + LP_FRONT + o / 4);
                c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
                lp_folded<2>(raw, o, l2, c, f2);
                lp_folded<4>(raw, o, l4, c, f4);
                lp_folded<8>(raw, o, l8, c, f8);
            }
            ph_group<LP_PITCH>(H, f2, nn, whole, lag_plane_row(2), 2, lane);
            ph_group<LP_PITCH>(H, f4, nn, whole, lag_plane_row(4), 4, lane);
            ph_group<LP_PITCH>(H, f8, nn, whole, lag_plane_row(8), 8, lane);
        }
    }
    __syncthreads();
    uint32_t *out = planes + (size_t)b * LAG_ROWS * 256;
    for (uint32_t i = tid; i < LAG_ROWS * 256; i += LP_THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < LP_COPIES; k++) c += s_h[k * LP_COPY_WORDS + (i >> 8) * LP_PITCH + (i & 255u)];
        if (c) atomicAdd(&out[i], c);
    }
}

__device__ __forceinline__ unsigned long long lp_wave_sum64(unsigned long long x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += (unsigned long long)__shfl_xor((long long)x, m, 64);
    return x;
}

// widths: null, or (the grid rule's use, grid_rule.h) three width words a segment: an element size whose word names no width has
// no candidate, and its cost is GRID_NO_COST
__global__ __launch_bounds__(LP_PLANE_WAVES * 64) void k_lp_cost(const uint32_t *__restrict__ planes, uint32_t count,
                                                                 const uint32_t *__restrict__ widths, unsigned long long *__restrict__ costs)
{
    __shared__ unsigned long long s_plane[LAG_ROWS];
    const uint32_t b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (b >= count) return;
    const uint32_t *rows = planes + (size_t)b * LAG_ROWS * 256;
    for (uint32_t pl = wave; pl < LAG_ROWS; pl += LP_PLANE_WAVES) {
        const uint4 q = *reinterpret_cast<const uint4 *>(rows + (size_t)pl * 256 + 4 * lane);
        const uint32_t h[4] = {q.x, q.y, q.z, q.w};
        const unsigned long long N = lp_wave_sum64((unsigned long long)h[0] + h[1] + h[2] + h[3]);
        unsigned long long c = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) c += filter_symbol_cost(h[k], N);
        c = lp_wave_sum64(c);
        if (lane == 0) s_plane[pl] = c;
    }
    __syncthreads();
    if (threadIdx.x < LAG_ELEMS) {
        const uint32_t e = 2u << threadIdx.x;
        unsigned long long c = 0;
        for (uint32_t j = 0; j < e; j++) c += s_plane[lag_plane_row(e) + j];
        if (widths && !grid_width_word(widths[(size_t)b * LAG_ELEMS + threadIdx.x])) c = GRID_NO_COST;
        costs[(size_t)b * LAG_ELEMS + threadIdx.x] = c;
    }
}

// spans: multiples of 16 KiB, at least LP_MIN_SPAN, at most LP_MAX_SPANS of them a segment
static dim3 lp_grid(uint32_t count, uint32_t max_len, uint32_t *span)
{
    const unsigned long long tiles = ((unsigned long long)max_len + LP_TILE - 1) / LP_TILE;
    unsigned long long per = (tiles + LP_MAX_SPANS - 1) / LP_MAX_SPANS;
    if (per < LP_MIN_SPAN / LP_TILE) per = LP_MIN_SPAN / LP_TILE;
    *span = (uint32_t)(per * LP_TILE);
    return dim3(count, (uint32_t)((tiles + per - 1) / per));
}

hipError_t lag_probe_sums(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                          uint32_t count, uint32_t max_len, unsigned long long *sums, uint32_t *lags)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)count * LAG_SUMS * 8, st);
    if (e != hipSuccess) return e;
    if (max_len >= 8) {
        uint32_t span;
        const dim3 grid = lp_grid(count, max_len, &span);
        hipLaunchKernelGGL(k_lp_sums, grid, dim3(LP_THREADS), 0, st, data, data_off, data_len, max_len, span, sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_lp_argmin, dim3(count), dim3(64), 0, st, sums, count, lags);
    return hipGetLastError();
}

hipError_t lag_probe_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                            uint32_t count, uint32_t max_len, const uint32_t *lags, uint32_t *planes, unsigned long long *costs)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(planes, 0, (size_t)count * LAG_ROWS * 1024, st);
    if (e != hipSuccess) return e;
    if (max_len >= 8) {
        uint32_t span;
        const dim3 grid = lp_grid(count, max_len, &span);
        hipLaunchKernelGGL(k_lp_planes, grid, dim3(LP_THREADS), 0, st, data, data_off, data_len, max_len, span, lags, planes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return lag_probe_cost(st, planes, count, nullptr, costs);
}

hipError_t lag_probe_cost(hipStream_t st, const uint32_t *planes, uint32_t count, const uint32_t *widths, unsigned long long *costs)
{
    hipLaunchKernelGGL(k_lp_cost, dim3(count), dim3(LP_PLANE_WAVES * 64), 0, st, planes, count, widths, costs);
    return hipGetLastError();
}

} // namespace glc
