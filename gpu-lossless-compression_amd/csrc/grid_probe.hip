// grid_probe.hip -- the grid probe (INTEGRATION.md 4b "Filter: auto with grid"; the sample, the sums, the winners, the planes and
// the costs are defined in grid_rule.h): which row width of the 2-D predictor (grid.hip) a segment wants at each element size, and
// what its planes would cost.  gfx950 / wave64.
//   k_gw_init    a segment's 3 * 65537 sums: 0 where a width is a candidate (2 .. Wmax of an element size with 1024 elements or
//                more), 0xFFFFFFFF everywhere else, so that callers zero nothing.
//   k_gw_sums    the sums, one instance for the elements of 2 and 4 bytes and one for those of 8.  One workgroup of 256 lanes per (segment, element size, tile of 256 targets, chunk of 4096 widths).  The
//                tile's targets and the 4096 + 255 history elements the chunk's widths reach lie in LDS, 2-byte elements widened
//                to dwords.  A lane owns 16 consecutive widths and walks the targets 16 at a time: the 31 history elements those
//                256 (target, width) pairs meet are a register window, of which 15 stay from the step before, so an LDS element
//                read serves 16 pairs.  The target of a step is the same for every lane (an LDS broadcast).  History position p
//                lies at p + p / 16: lanes 16 elements apart read 17 words (64-bit elements: 17 double words) apart, which no
//                two lanes of a wave share a bank for.  Per pair: subtract, (2-byte elements: sign-extend,) fold, count leading
//                zeros, add -- the sum of the bit lengths is 256 * width less the sum of the leading zeros.  A lane's 16 sums leave
//                with one 32-bit global atomic add each: integer adds commute, so the result does not depend on scheduling.  The
//                elements are read one by one at any alignment of the segment; nothing in front of or behind a segment is read.
//   k_gw_argmin  one workgroup per (segment, element size): the width with the smallest sum, ties to the smallest width, 0 where
//                there is no candidate, to device memory, so that the host is not involved between the two probes.
//   k_gw_planes  one instance per element size: the byte-plane histograms of what the grid forward at (e, w_e, fold) builds, w_e
//                read from device memory (a word outside 2 .. 65536 names no width: the instance does nothing, and the word is
//                never a distance).  grid.hip's geometry unchanged -- 16 KiB tiles of whole runs, lag_tile.h's two raw images and
//                granule arithmetic -- with plane_hist.h's counting (two LDS counter copies, the uniform-value shortcut: the upper
//                planes of a good width are almost all zero) in place of the plane build.
//   The costs are k_lp_cost's (lag_probe.hip) over these 14 rows, GRID_NO_COST where the width word names no width.
// Any segment length up to 2^31, any byte alignment; only the first L - L % 8 bytes are counted.
#include "container_internal.h"
#include "glc_device.h"
#include "grid_rule.h"
#include "lag_tile.h"
#include "plane_hist.h"

#include <type_traits>

namespace glc {

constexpr uint32_t GW_THREADS = 256;
constexpr uint32_t GW_OWN = 16;                                // consecutive widths a lane owns; targets a step
constexpr uint32_t GW_CHUNK = GW_THREADS * GW_OWN;             // widths a workgroup
constexpr uint32_t GW_CHUNKS = (GRID_W_MAX - GRID_W_MIN + GW_CHUNK) / GW_CHUNK;       // 16
constexpr uint32_t GW_HIST = GW_CHUNK + GRID_TILE - 1;         // history elements a workgroup reaches
constexpr uint32_t GW_HIST_WORDS = GW_HIST + GW_HIST / GW_OWN + 1;
constexpr uint32_t GW_WINDOW = 2 * GW_OWN - 1;
constexpr uint32_t GW_COPIES = 2, GW_PITCH = 257;
constexpr uint32_t GW_ARGMIN_THREADS = 1024;                   // (a lane walks 64 sums: the walk is bound by their latency)
constexpr uint32_t GW_PLANE_BLOCKS = 1024;                     // workgroups a segment's tiles are dealt to
static_assert(GRID_TILE % GW_OWN == 0 && GW_CHUNKS * GW_CHUNK >= GRID_W_MAX - GRID_W_MIN + 1, "the chunks cover every width");

__device__ __forceinline__ uint32_t gw_len(const unsigned long long *len, uint32_t i, uint32_t max_len)
{
    const unsigned long long l = len[i];
    return (l > max_len ? max_len : (uint32_t)l) & ~7u;
}

__global__ __launch_bounds__(GW_THREADS) void k_gw_init(const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                        uint32_t *__restrict__ sums)
{
    const uint32_t b = blockIdx.x, k = blockIdx.y;
    const uint32_t N = gw_len(data_len, b, max_len) >> (k + 1);
    const uint32_t wmax = N < GRID_MIN_ELEMS ? 0u : grid_wmax(N);
    uint32_t *row = sums + (size_t)b * GRID_SUMS + (size_t)k * GRID_SUM_ROW;
    for (uint32_t w = threadIdx.x; w < GRID_SUM_ROW; w += GW_THREADS) row[w] = w >= GRID_W_MIN && w <= wmax ? 0u : GRID_NO_SUM;
}

// element i of the segment at `in`; al: the segment's address is a multiple of ELEM
template <uint32_t ELEM, class T>
__device__ __forceinline__ T gw_load(const uint8_t *in, unsigned long long i, bool al)
{
    const uint8_t *p = in + i * ELEM;
    if (al) {
        if constexpr (ELEM == 2) return *reinterpret_cast<const uint16_t *>(p);
        else return *reinterpret_cast<const T *>(p);
    }
    T v = 0;
#pragma unroll
    for (uint32_t k = 0; k < ELEM; k++) v |= (T)p[k] << (8 * k);
    return v;
}

// the leading zeros of the folded difference x - p: width of T less its bit length
template <uint32_t ELEM, class T>
__device__ __forceinline__ uint32_t gw_pair_clz(T x, T p)
{
    if constexpr (ELEM == 8) {
        const unsigned long long d = x - p, f = (d << 1) ^ (0ull - (d >> 63));
        return (uint32_t)__clzll((long long)f);
    } else {
        int d = (int)(x - p);
        if constexpr (ELEM == 2) d = (int)((uint32_t)d << 16) >> 16;               // (the difference modulo 2^16, its sign spread)
        const uint32_t f = ((uint32_t)d << 1) ^ (uint32_t)(d >> 31);
        return (uint32_t)__clz((int)f);
    }
}

// widths wlo .. wlo + GW_CHUNK - 1 (those up to wmax) against the tile of 256 targets at element bt of the N-element segment
template <uint32_t ELEM>
__device__ __forceinline__ void gw_sums_tile(const uint8_t *in, uint32_t wmax, unsigned long long bt, uint32_t wlo, uint32_t *row,
                                             unsigned long long *lds)
{
    using T = typename std::conditional<ELEM == 8, unsigned long long, uint32_t>::type;
    constexpr uint32_t BITS = ELEM == 8 ? 64 : 32;             // the width the zeros are counted in
    T *hist = reinterpret_cast<T *>(lds), *tgt = hist + GW_HIST_WORDS;
    const uint32_t tid = threadIdx.x;
    const bool al = (reinterpret_cast<uintptr_t>(in) & (ELEM - 1)) == 0;
    // history position p is element hb + p; the pair (target j, width W) meets position j + GW_CHUNK - 1 - (W - wlo).  Positions
    // in front of the segment belong to widths above wmax alone, which are not written
    const long long hb = (long long)bt - (long long)wlo - (long long)(GW_CHUNK - 1);
    for (uint32_t p = tid; p < GW_HIST; p += GW_THREADS) {
        const long long i = hb + (long long)p;
        hist[p + p / GW_OWN] = i >= 0 ? gw_load<ELEM, T>(in, (unsigned long long)i, al) : (T)0;
    }
    tgt[tid] = gw_load<ELEM, T>(in, bt + tid, al);
    __syncthreads();
    // this lane's widths: wlo + GW_OWN tid + r; target jb + s meets window element s - r + GW_OWN - 1 of the window at position q0 + jb
    const uint32_t q0 = GW_CHUNK - GW_OWN * (tid + 1);
    uint32_t acc[GW_OWN];
    T win[GW_WINDOW];
#pragma unroll
    for (uint32_t r = 0; r < GW_OWN; r++) acc[r] = 0;
    const T *h = hist + q0 + q0 / GW_OWN;
#pragma unroll
    for (uint32_t i = 0; i < GW_OWN - 1; i++) win[i] = h[i];
#pragma unroll 1
    for (uint32_t jb = 0; jb < GRID_TILE; jb += GW_OWN) {
        T x[GW_OWN];
#pragma unroll
        for (uint32_t s = 0; s < GW_OWN; s++) x[s] = tgt[jb + s];
#pragma unroll
        for (uint32_t i = GW_OWN - 1; i < GW_WINDOW; i++) win[i] = h[i + i / GW_OWN];
#pragma unroll
        for (uint32_t s = 0; s < GW_OWN; s++) {
#pragma unroll
            for (uint32_t r = 0; r < GW_OWN; r++) acc[r] += gw_pair_clz<ELEM, T>(x[s], win[s - r + GW_OWN - 1]);
        }
#pragma unroll
        for (uint32_t i = 0; i < GW_OWN - 1; i++) win[i] = win[i + GW_OWN];
        h += GW_OWN + 1;
    }
#pragma unroll
    for (uint32_t r = 0; r < GW_OWN; r++) {
        const uint32_t W = wlo + GW_OWN * tid + r;
        if (W <= wmax) atomicAdd(&row[W], BITS * GRID_TILE - acc[r]);
    }
}

// grid: (segments, element sizes x 32 tiles x 16 chunks); WIDE: the 64-bit elements, else those of 2 and 4 bytes
template <bool WIDE>
__global__ __launch_bounds__(GW_THREADS) void k_gw_sums(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                        const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                        uint32_t *__restrict__ sums)
{
    __shared__ unsigned long long lds[(GW_HIST_WORDS + GRID_TILE) / (WIDE ? 1 : 2) + 1];
    const uint32_t b = blockIdx.x, y = blockIdx.y;
    const uint32_t k = WIDE ? 2 : y / (GRID_TILES * GW_CHUNKS), t = y / GW_CHUNKS % GRID_TILES, c = y % GW_CHUNKS;
    const uint32_t N = gw_len(data_len, b, max_len) >> (k + 1);
    if (N < GRID_MIN_ELEMS) return;
    const uint32_t wmax = grid_wmax(N), wlo = GRID_W_MIN + c * GW_CHUNK;
    if (wlo > wmax) return;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const unsigned long long bt = grid_tile_start(N, wmax, t);
    uint32_t *row = sums + (size_t)b * GRID_SUMS + (size_t)k * GRID_SUM_ROW;
    if constexpr (WIDE) gw_sums_tile<8>(in, wmax, bt, wlo, row, lds);
    else if (k == 0) gw_sums_tile<2>(in, wmax, bt, wlo, row, lds);
    else gw_sums_tile<4>(in, wmax, bt, wlo, row, lds);
}

// grid: (segments, 3)
__global__ __launch_bounds__(GW_ARGMIN_THREADS) void k_gw_argmin(const uint32_t *__restrict__ sums, const unsigned long long *__restrict__ data_len,
                                                          uint32_t max_len, uint32_t *__restrict__ widths)
{
    __shared__ unsigned long long s_key[GW_ARGMIN_THREADS];
    const uint32_t b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const uint32_t N = gw_len(data_len, b, max_len) >> (k + 1);
    if (N < GRID_MIN_ELEMS) {
        if (tid == 0) widths[(size_t)b * LAG_ELEMS + k] = 0;
        return;
    }
    const uint32_t wmax = grid_wmax(N);
    const uint32_t *row = sums + (size_t)b * GRID_SUMS + (size_t)k * GRID_SUM_ROW;
    unsigned long long key = ~0ull;                            // (sum, width): the smallest key is the winner
#pragma unroll 8
    for (uint32_t w = GRID_W_MIN + tid; w <= wmax; w += GW_ARGMIN_THREADS) {
        const unsigned long long v = (unsigned long long)row[w] << 32 | w;
        key = v < key ? v : key;
    }
    s_key[tid] = key;
    __syncthreads();
    for (uint32_t m = GW_ARGMIN_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) s_key[tid] = s_key[tid + m] < s_key[tid] ? s_key[tid + m] : s_key[tid];
        __syncthreads();
    }
    if (tid == 0) widths[(size_t)b * LAG_ELEMS + k] = (uint32_t)s_key[0];
}

// ---------------------------------------------------------------------------
// the two-image tile of grid.hip's forward, restated for the plane probe (grid.hip keeps its own text, so that its kernels keep
// their machine code): a tile's own bytes and the bytes one row (wb bytes) in front of them, each image at its own alignment
// ---------------------------------------------------------------------------
constexpr uint32_t GW_FRONT = 4;                               // words in front of a raw image (a read starts up to 8 bytes early)
constexpr uint32_t GW_RAW_WORDS = GW_FRONT + 4 * SH_NGI;

// p with every element k zeroed for which keep(k) is false
template <uint32_t ELEM, class Keep>
__device__ __forceinline__ void gw_select(uint32_t (&p)[4], Keep keep)
{
#pragma unroll
    for (uint32_t m = 0; m < 4; m++) {
        if constexpr (ELEM == 2) p[m] &= (keep(2 * m) ? 0xFFFFu : 0u) | (keep(2 * m + 1) ? 0xFFFF0000u : 0u);
        else p[m] = keep(ELEM == 8 ? m / 2 : m) ? p[m] : 0u;
    }
}

// the nbytes (<= SH_TILE) at byte a0 of the segment at `in` into raw, the nbytes wb in front of them into above, as aligned
// 16-byte granules; s, sb: where the first byte of each lies in its image.  No granule wholly in front of the segment is read
__device__ __forceinline__ void gw_stage(const uint8_t *in, unsigned long long a0, unsigned long long wb, uint32_t nbytes, uint32_t *raw,
                                         uint32_t *above, uint32_t &s, uint32_t &sb)
{
    const uint32_t tid = threadIdx.x;
    const long long a = (long long)a0, ab = a - (long long)wb;                     // the tile's and the row above's byte in the segment
    s = (uint32_t)(((unsigned long long)(uintptr_t)in + (unsigned long long)a) & 15);
    sb = (uint32_t)(((unsigned long long)(uintptr_t)in + (unsigned long long)ab) & 15);
    const uint32_t ng = (s + nbytes + 15) / 16, ngb = (sb + nbytes + 15) / 16;     // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS)
        reinterpret_cast<uint4 *>(raw + GW_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + (a - (long long)s) + 16ll * g);
    for (uint32_t g = tid; g < ngb; g += SH_THREADS) {
        const long long off = ab - (long long)sb + 16ll * g;   // the aligned granule's first byte in the segment
        if (off > -16) reinterpret_cast<uint4 *>(above + GW_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + off);
    }
}

// the folded differences of granule g of the tile.  c: the granule, p: the 16 bytes one element back; ca, pa: the same of the row
// above.  rt: the band-relative index of the tile's first element, r: of the granule's (the period P is a multiple of 16 / ELEM,
// so a granule never leaves its band)
template <uint32_t ELEM>
__device__ __forceinline__ void gw_granule(const uint32_t *raw, const uint32_t *above, uint32_t s, uint32_t sb, uint32_t g, uint32_t rt,
                                           uint32_t W, uint32_t P, uint32_t fold, uint32_t (&c)[4])
{
    constexpr uint32_t E = 16 / ELEM;                          // elements of a granule
    uint32_t p[4], ca[4], pa[4];
    lg_read16(raw + GW_FRONT, (int)(s + 16 * g), c);
    lg_read16(raw + GW_FRONT, (int)(s + 16 * g) - (int)ELEM, p);
    lg_read16(above + GW_FRONT, (int)(sb + 16 * g), ca);
    lg_read16(above + GW_FRONT, (int)(sb + 16 * g) - (int)ELEM, pa);
    const uint32_t r = (rt + g * E) % P;
    gw_select<ELEM>(ca, [&](uint32_t k) { return r + k >= W; });
    gw_select<ELEM>(pa, [&](uint32_t k) { return r + k > W; });      // (element i - 1 has a row above; at r + k = 0 a run starts)
    lg_combine<ELEM, true>(c, ca);
    lg_combine<ELEM, true>(p, pa);
    lg_mask<ELEM>(p, (16 * g) & (LG_RUN * ELEM - 1), ELEM);
    lg_combine<ELEM, true>(c, p);
    lg_fold<ELEM, false>(c, fold);
}

// grid: (segments, up to GW_PLANE_BLOCKS)
template <uint32_t ELEM>
__global__ __launch_bounds__(SH_THREADS) void k_gw_planes(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                          const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                          const uint32_t *__restrict__ widths, uint32_t *__restrict__ planes)
{
    using G = ShGeom<ELEM>;
    constexpr uint32_t E = 16 / ELEM, K = ELEM == 2 ? 0 : ELEM == 4 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) uint32_t raw[GW_RAW_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t above[GW_RAW_WORDS];
    __shared__ uint32_t s_h[GW_COPIES * ELEM * GW_PITCH];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t W = grid_width_word(widths[(size_t)b * LAG_ELEMS + K]);
    const uint32_t q = gw_len(data_len, b, max_len) / ELEM;
    const uint32_t nt = (q + G::TQ - 1) / G::TQ;
    if (!W || blockIdx.y >= nt) return;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const uint32_t P = ct_grid_period(W);
    for (uint32_t i = tid; i < GW_COPIES * ELEM * GW_PITCH; i += SH_THREADS) s_h[i] = 0;
    uint32_t *H = s_h + (tid & (GW_COPIES - 1)) * ELEM * GW_PITCH;
    for (uint32_t t = blockIdx.y; t < nt; t += gridDim.y) {
        const uint32_t i0 = t * G::TQ, cnt = min(G::TQ, q - i0), nbytes = cnt * ELEM;      // nbytes: a multiple of 8
        __syncthreads();                                       // (the tile before has been read; the counters are zero)
        uint32_t s, sb;
        gw_stage(in, (unsigned long long)i0 * ELEM, (unsigned long long)W * ELEM, nbytes, raw, above, s, sb);
        __syncthreads();
        const uint32_t nge = (nbytes + 15) / 16, rt = i0 % P;
        for (uint32_t g0 = wave * 64; g0 < nge; g0 += SH_THREADS) {
            const uint32_t g = g0 + lane;
            const uint32_t n = g < nge ? min(16u, nbytes - 16 * g) : 0u;           // 0, 8 or 16
            const bool whole = nbytes - 16 * g0 >= 1024;       // wave-uniform
            uint32_t c[4] = {0, 0, 0, 0};
            if (n) gw_granule<ELEM>(raw, above, s, sb, g, rt, W, P, 1, c);
            ph_group<GW_PITCH>(H, c, n, whole, 0, ELEM, lane);
        }
    }
    __syncthreads();
    uint32_t *out = planes + (size_t)b * LAG_ROWS * 256 + lag_plane_row(ELEM) * 256;
    for (uint32_t i = tid; i < ELEM * 256; i += SH_THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < GW_COPIES; k++) c += s_h[k * ELEM * GW_PITCH + (i >> 8) * GW_PITCH + (i & 255u)];
        if (c) atomicAdd(&out[i], c);
    }
}

hipError_t grid_probe_sums(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                           uint32_t count, uint32_t max_len, uint32_t *sums, uint32_t *widths)
{
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gw_init, dim3(count, LAG_ELEMS), dim3(GW_THREADS), 0, st, data_len, max_len, sums);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (max_len >= 2 * GRID_MIN_ELEMS) {
        hipLaunchKernelGGL(k_gw_sums<false>, dim3(count, 2 * GRID_TILES * GW_CHUNKS), dim3(GW_THREADS), 0, st, data, data_off, data_len,
                           max_len, sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_gw_sums<true>, dim3(count, GRID_TILES * GW_CHUNKS), dim3(GW_THREADS), 0, st, data, data_off, data_len,
                           max_len, sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_gw_argmin, dim3(count, LAG_ELEMS), dim3(GW_ARGMIN_THREADS), 0, st, sums, data_len, max_len, widths);
    return hipGetLastError();
}

template <uint32_t ELEM>
static hipError_t gw_launch_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                                   uint32_t count, uint32_t max_len, const uint32_t *widths, uint32_t *planes)
{
    const uint32_t nt = (uint32_t)(((unsigned long long)max_len + SH_TILE - 1) / SH_TILE);
    hipLaunchKernelGGL(k_gw_planes<ELEM>, dim3(count, std::min(nt, GW_PLANE_BLOCKS)), dim3(SH_THREADS), 0, st, data, data_off, data_len,
                       max_len, widths, planes);
    return hipGetLastError();
}

hipError_t grid_probe_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                             uint32_t count, uint32_t max_len, const uint32_t *widths, uint32_t *planes, unsigned long long *costs)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(planes, 0, (size_t)count * LAG_ROWS * 1024, st);
    if (e != hipSuccess) return e;
    if (max_len >= 8) {
        if ((e = gw_launch_planes<2>(st, data, data_off, data_len, count, max_len, widths, planes)) != hipSuccess) return e;
        if ((e = gw_launch_planes<4>(st, data, data_off, data_len, count, max_len, widths, planes)) != hipSuccess) return e;
        if ((e = gw_launch_planes<8>(st, data, data_off, data_len, count, max_len, widths, planes)) != hipSuccess) return e;
    }
    return lag_probe_cost(st, planes, count, widths, costs);
}

} // namespace glc
