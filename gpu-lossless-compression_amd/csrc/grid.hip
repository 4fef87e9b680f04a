// grid.hip -- the 2-D (row-stride) predictor of the container's typed-data filter (INTEGRATION.md 4b "Delta: grid", format version
// 12): the delta + shuffle of lag.hip at lag 1 over the differences to the element one ROW above, for row-major gridded data
// (images, detector frames, slices of simulation fields, rasters).  With x[i] element i of a segment as a little-endian unsigned
// integer of ELEM = 2, 4 or 8 bytes, arithmetic modulo 2^(8 ELEM), RUN = 2048 elements, the row width 2 <= W <= 65536 elements and
// the period P = 2048 ceil(W / 64) (a band, about 32 rows, a multiple of RUN):
//   forward   v[i] = x[i] where i mod P < W, else x[i] - x[i - W]; d[i] = v[i] where i mod RUN == 0, else v[i] - v[i - 1];
//             f[i] = d[i], or with the fold (d[i] << 1) ^ (0 - (d[i] >> (8 ELEM - 1))); out[j q + i] = byte j of f[i]
//   inverse   lag.hip's inverse at (1, fold) gives v; then x[i] = v[i] + x[i - W] for i mod P >= W, up every band
// over the q = len / ELEM whole elements, the last len % ELEM bytes copied in place.  The rule is linear in i: a frame needs no row
// alignment, the "left" element of a row's first is the end of the row above.  Bands are independent and runs nest inside bands.
//
// Forward, one pass, lag.hip's geometry (one workgroup of 256 lanes per 16 KiB tile of whole runs, aligned 16-byte granule loads at
// any alignment of the buffers, lag_tile.h's plane build): a tile takes two raw images, its own bytes and the bytes W ELEM in
// front of them, each at its own alignment; no granule that lies wholly in front of the segment is read (its elements have
// i < W, so i mod P < W: they subtract 0).  Every lane takes for its granule the 16 bytes and the 16 bytes one element back from
// both images (five aligned dwords and v_alignbyte each), subtracts the row above where the band-relative index says so -- for the
// element one back where ITS index says so -- and goes on as lag.hip's forward at lag 1.
// Inverse: two kernels.  lag.hip's (or at fold 0 delta.hip's) inverse writes v to the output; k_grid_vsum then works in place on
// the output: per band one lane owns a column slice and walks the band's rows (up to ceil(P / W)) adding the row above, lanes of
// a wave on adjacent columns, so every row access is contiguous across the wave.  Fast path: 16-byte accesses, where W ELEM and
// the output address are multiples of 16; general path: element-sized accesses at any alignment.  Plain vector loads and stores;
// the first W elements of a band are never written.
//
// LDS: forward 51264 bytes (two raw images of 16416, padded image 18432): three workgroups per CU; k_grid_vsum none.
#include "grid_tile.h"

namespace glc {

constexpr uint32_t GD_VSUM_ROWS = 4;                           // rows k_grid_vsum has in flight per lane

// ---------------------------------------------------------------------------
// forward: elements [i0, i0 + cnt) of a segment whose q whole elements start at `in`; i0 is a multiple of RUN
// ---------------------------------------------------------------------------
template <uint32_t ELEM>
__device__ __forceinline__ void gd_tile_forward(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t W, uint32_t P, uint32_t fold, uint32_t *raw, uint32_t *above,
                                                uint32_t *img)
{
    constexpr uint32_t E = 16 / ELEM;                          // elements of a granule
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long a = (long long)(i0 * ELEM), ab = a - (long long)W * ELEM;       // the tile's and the row above's byte in the segment
    const uint32_t s = (uint32_t)(((unsigned long long)(uintptr_t)in + (unsigned long long)a) & 15);
    const uint32_t sb = (uint32_t)(((unsigned long long)(uintptr_t)in + (unsigned long long)ab) & 15);
    const uint32_t ng = (s + cnt * ELEM + 15) / 16, ngb = (sb + cnt * ELEM + 15) / 16;     // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS)
        reinterpret_cast<uint4 *>(raw + GD_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + (a - (long long)s) + 16ll * g);
    for (uint32_t g = tid; g < ngb; g += SH_THREADS) {
        const long long off = ab - (long long)sb + 16ll * g;   // the aligned granule's first byte in the segment
        if (off > -16) reinterpret_cast<uint4 *>(above + GD_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + off);
    }
    __syncthreads();
    const uint32_t nge = (cnt * ELEM + 15) / 16;               // <= 1024
    const uint32_t rt = (uint32_t)(i0 % P);                    // the tile's first element within its band
    for (uint32_t g = tid; g < nge; g += SH_THREADS) {
        // c: the granule, p: the 16 bytes one element back; ca, pa: the same of the row above.  r: the band-relative index of the
        // granule's first element (P is a multiple of E, so a granule never leaves its band)
        uint32_t c[4], p[4], ca[4], pa[4];
        lg_read16(raw + GD_FRONT, (int)(s + 16 * g), c);
        lg_read16(raw + GD_FRONT, (int)(s + 16 * g) - (int)ELEM, p);
        lg_read16(above + GD_FRONT, (int)(sb + 16 * g), ca);
        lg_read16(above + GD_FRONT, (int)(sb + 16 * g) - (int)ELEM, pa);
        const uint32_t r = (rt + g * E) % P;
        gd_select<ELEM>(ca, [&](uint32_t k) { return r + k >= W; });
        gd_select<ELEM>(pa, [&](uint32_t k) { return r + k > W; });      // (element i - 1 has a row above; at r + k = 0 a run starts)
        lg_combine<ELEM, true>(c, ca);
        lg_combine<ELEM, true>(p, pa);
        lg_mask<ELEM>(p, (16 * g) & (LG_RUN * ELEM - 1), ELEM);
        lg_combine<ELEM, true>(c, p);
        lg_fold<ELEM, false>(c, fold);
        lg_img_store<ELEM>(img, g, c);
    }
    __syncthreads();
    lg_planes<ELEM>(img, out, q, i0, cnt, tid, lane, wave);
}

template <uint32_t ELEM>
__global__ __launch_bounds__(SH_THREADS) void k_grid_forward(const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t W, uint32_t P,
                                                             uint32_t fold)
{
    using G = ShGeom<ELEM>;
    __shared__ __attribute__((aligned(16))) uint32_t raw[GD_RAW_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t above[GD_RAW_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t img[LG_IMG_WORDS];
    static_assert(G::TQ % LG_RUN == 0, "a tile holds whole runs");
    const unsigned long long q = len / ELEM, nt = q ? (q + G::TQ - 1) / G::TQ : 1;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, q - i0);
        if (cnt) gd_tile_forward<ELEM>(in, out, q, i0, cnt, W, P, fold, raw, above, img);
        if (t + 1 == nt && threadIdx.x < (uint32_t)(len - q * ELEM)) out[q * ELEM + threadIdx.x] = in[q * ELEM + threadIdx.x];
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

// ---------------------------------------------------------------------------
// the sums up the bands: `count` elements of v at `out`, element 0 the first of a band, become x in place
// ---------------------------------------------------------------------------
template <class T> struct alignas(16) GdVec { T v[16 / sizeof(T)]; };

// what a lane holds of a row: 16 aligned bytes (FAST) or one element at any alignment
template <class T, bool FAST> struct GdSlice;
template <class T> struct GdSlice<T, true> {
    static constexpr uint32_t N = 16 / sizeof(T);
    GdVec<T> x;
    __device__ __forceinline__ void load(const uint8_t *p) { x = *reinterpret_cast<const GdVec<T> *>(p); }
    __device__ __forceinline__ void store(uint8_t *p) const { *reinterpret_cast<GdVec<T> *>(p) = x; }
    __device__ __forceinline__ void add(const GdSlice &o)
    {
#pragma unroll
        for (uint32_t k = 0; k < N; k++) x.v[k] = (T)(x.v[k] + o.x.v[k]);
    }
};
template <class T> struct GdSlice<T, false> {
    static constexpr uint32_t N = 1;
    T x;
    __device__ __forceinline__ void load(const uint8_t *p) { __builtin_memcpy(&x, p, sizeof(T)); }
    __device__ __forceinline__ void store(uint8_t *p) const { __builtin_memcpy(p, &x, sizeof(T)); }
    __device__ __forceinline__ void add(const GdSlice &o) { x = (T)(x + o.x); }
};

template <class T, bool FAST>
__global__ __launch_bounds__(SH_THREADS) void k_grid_vsum(uint8_t *out, unsigned long long count, uint32_t W, uint32_t P)
{
    using S = GdSlice<T, FAST>;
    constexpr uint32_t N = S::N;                               // elements of a lane's slice
    const uint32_t slices = W / N;                             // (FAST: W is a multiple of N)
    const unsigned long long units = (count + P - 1) / P * slices;
    for (unsigned long long u = blockIdx.x * (unsigned long long)SH_THREADS + threadIdx.x; u < units; u += gridDim.x * (unsigned long long)SH_THREADS) {
        const unsigned long long band = u / slices;
        const uint32_t c = (uint32_t)(u - band * slices) * N;                       // the slice's first column
        const uint32_t n = (uint32_t)min((unsigned long long)P, count - band * P);  // elements of this band
        uint8_t *base = out + band * P * sizeof(T);
        if (c + N > n) continue;                               // (row 0 ends in front of or inside the slice: nothing below it)
        S acc;
        acc.load(base + (size_t)c * sizeof(T));
        uint32_t e = c + W;
        while (e + N <= n) {                                   // rows whose slice lies whole in the band, GD_VSUM_ROWS loads ahead
            S r[GD_VSUM_ROWS];
#pragma unroll
            for (uint32_t j = 0; j < GD_VSUM_ROWS; j++)
                if (e + j * W + N <= n) r[j].load(base + (size_t)(e + j * W) * sizeof(T));
#pragma unroll
            for (uint32_t j = 0; j < GD_VSUM_ROWS; j++)
                if (e + j * W + N <= n) { acc.add(r[j]); acc.store(base + (size_t)(e + j * W) * sizeof(T)); }
            e += GD_VSUM_ROWS * W;
        }
        if constexpr (FAST) {                                  // the band's last row may end inside the slice: element by element
            const uint32_t ep = c + (n - 1 - c) / W * W;       // the slice's place in the last row that reaches column c
            if (ep > c && ep + N > n) {
#pragma unroll
                for (uint32_t k = 0; k < N; k++)
                    if (ep + k < n) {
                        T *p = reinterpret_cast<T *>(base) + ep + k;
                        *p = (T)(*p + acc.x.v[k]);
                    }
            }
        }
    }
}

template <uint32_t ELEM>
static hipError_t gd_launch_forward(hipStream_t st, uint32_t grid, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t W,
                                    uint32_t fold)
{
    hipLaunchKernelGGL(k_grid_forward<ELEM>, dim3(grid), dim3(SH_THREADS), 0, st, in, out, len, W, ct_grid_period(W), fold);
    return hipGetLastError();
}

template <class T>
static hipError_t gd_launch_vsum(hipStream_t st, uint8_t *out, unsigned long long count, uint32_t W, uint32_t P)
{
    const bool fast = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (W * sizeof(T)) % 16 == 0;
    const unsigned long long units = (count + P - 1) / P * (fast ? W / (16 / sizeof(T)) : W);
    const dim3 grid((uint32_t)std::min<unsigned long long>((units + SH_THREADS - 1) / SH_THREADS, 1u << 20)), block(SH_THREADS);
    if (fast) hipLaunchKernelGGL((k_grid_vsum<T, true>), grid, block, 0, st, out, count, W, P);
    else hipLaunchKernelGGL((k_grid_vsum<T, false>), grid, block, 0, st, out, count, W, P);
    return hipGetLastError();
}

// v -> x over `count` elements at `out`, the first of them the first of a band: every element at P-relative place W or beyond
// gains the element W places back.  vol.hip runs the same walk up its slabs, with (S, Q) for (W, P): the kernel's indices within a
// band are 32-bit and stay below P + GD_VSUM_ROWS * W, which holds at Q <= 2^28 + 2^21 and S <= 2^24
hipError_t grid_vsum_device(hipStream_t st, uint8_t *out, unsigned long long count, uint32_t elem, uint32_t W, uint32_t P)
{
    if (count <= W) return hipSuccess;                         // (one row: nothing above anything)
    switch (elem) {
    case 2: return gd_launch_vsum<uint16_t>(st, out, count, W, P);
    case 4: return gd_launch_vsum<uint32_t>(st, out, count, W, P);
    case 8: return gd_launch_vsum<unsigned long long>(st, out, count, W, P);
    default: return hipErrorInvalidValue;
    }
}

hipError_t grid_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, uint32_t width,
                               uint32_t fold, bool inverse)
{
    if (!shuffle_elem_ok(elem) || !ct_grid_width_ok(width) || fold > 1) return hipErrorInvalidValue;
    if (len == 0) return hipSuccess;
    if (inverse) {
        const hipError_t e = lag_shuffle_device(st, in, out, len, elem, 1, fold, true);
        return e != hipSuccess ? e : grid_vsum_device(st, out, len / elem, elem, width, ct_grid_period(width));
    }
    const unsigned long long tq = SH_TILE / elem, q = len / elem, nt = q ? (q + tq - 1) / tq : 1;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(nt, 1u << 24);     // (one workgroup per tile up to 256 GiB)
    switch (elem) {
    case 2: return gd_launch_forward<2>(st, grid, in, out, len, width, fold);
    case 4: return gd_launch_forward<4>(st, grid, in, out, len, width, fold);
    default: return gd_launch_forward<8>(st, grid, in, out, len, width, fold);
    }
}

// the range form of the inverse: `first` is a multiple of P, so out[0] is the first element of a band
hipError_t ungrid_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                         uint32_t width, uint32_t fold, unsigned long long first, unsigned long long count)
{
    if (!shuffle_elem_ok(elem) || !ct_grid_width_ok(width) || fold > 1) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (first % ct_grid_period(width)) return hipErrorInvalidValue;
    const hipError_t e = unlag_unshuffle_range_device(st, in, out, q, elem, 1, fold, first, count);
    return e != hipSuccess ? e : grid_vsum_device(st, out, count, elem, width, ct_grid_period(width));
}

} // namespace glc
