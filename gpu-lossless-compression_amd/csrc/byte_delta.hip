// byte_delta.hip -- the byte predictor of the container for 8-bit sample data (INTEGRATION.md 4b "Delta: bytes", format version 15):
// greyscale, RGB and RGBA images, masks and label maps, 8-bit depth or detector frames, u8 audio.  With x the bytes of a segment of
// any length, arithmetic modulo 256, RUN = 2048, the lag 1 <= LAG <= 16 (the channel count), the row stride S = 0 (none) or
// 2 <= S <= 65536 bytes (channels * width) and the period P = 2048 ceil(S / 64) (a band of at least 32 rows, a multiple of RUN):
//   forward   v[i] = x[i] where S == 0 or i mod P < S, else x[i] - x[i - S]; d[i] = v[i] where i mod RUN < LAG, else v[i] - v[i - LAG];
//             out[i] = d[i]: same length, same positions, no planes and no tail
//   inverse   v[i] = d[i] + d[i - LAG] + d[i - 2 LAG] + ... down to the member of the chain with i mod RUN < LAG; then
//             x[i] = v[i] + x[i - S] for i mod P >= S, up every band
// The rule is linear in i: a segment needs no row alignment.  Runs nest in bands, bands and runs are independent, and S < LAG is
// legal (the two differences commute).  There is no fold: for one-byte elements it permutes the byte values, which an order-0
// coder cannot see.
//
// The geometry is lag.hip's and grid.hip's: one workgroup of 256 lanes per 16 KiB tile of whole runs, aligned 16-byte granule
// loads at any alignment of the buffers, nothing in front of the segment is ever read, 64-bit offsets, a single segment.
// Arithmetic is on four packed bytes per dword (SWAR, bd_sub4 / bd_add4: six instructions a dword each; two v_pk_*_u16 halves
// would take twelve with their splits and joins).
// Forward, one pass: a tile takes its own bytes and, with a stride, the bytes S in front of them as two raw LDS images, each at
// its own alignment; no granule that lies wholly in front of the segment is read (its bytes have i < S: they subtract 0).  Every
// lane takes for an OUTPUT-aligned granule the four neighbourhoods (0, -LAG, -S, -S - LAG) with lg_read16, masks them byte by
// byte -- the row above where the band-relative index is at least S, for the byte LAG back where it is at least S + LAG, the lag
// term where the run-relative index is at least LAG -- subtracts and stores 16 bytes; the head and tail bytes of the tile's output
// run go byte by byte.
// Inverse, two kernels.  k_bd_scan: lag.hip's Kogge-Stone scan over the flat image of the tile at byte distances LAG, 2 LAG, 4 LAG,
// ... below RUN (7 to 11 rounds) between two LDS images, one read, one write and one barrier a
// round, the byte mask of a run's first granules without a branch; its range form takes bytes
// [first, first + count) with first a multiple of RUN (of P with a stride).  k_bd_vsum then works in place on the output: per band
// one lane owns 16 columns and walks the band's rows adding the row above, lanes of a wave on adjacent columns, with 16-byte
// accesses at whatever alignment the row has (S is usually odd: 3 * 427); only the last S mod 16 columns of a row and a band's
// ragged last row go byte by byte.  Plain vector loads and stores.
//
// LDS: forward 16416 bytes without a stride (eight workgroups per CU, the wave limit) and 32832 with one (four); k_bd_scan 32832
// (four); k_bd_vsum none.
#include "lag_tile.h"

namespace glc {

constexpr uint32_t BD_FRONT = 4;                               // words in front of an image (a read starts up to 16 bytes early)
constexpr uint32_t BD_IMG_WORDS = BD_FRONT + 4 * SH_NGI;       // a 16 KiB range at any alignment; as a flat image, with a granule of slack
constexpr uint32_t BD_PASSES = SH_TILE / 16 / SH_THREADS;      // tile-aligned granules of a tile per lane
constexpr uint32_t BD_VSUM_ROWS = 4;                           // rows k_bd_vsum has in flight per lane
constexpr uint32_t BD_H = 0x80808080u;
static_assert(BD_PASSES == 4, "four passes of 256 lanes cover a tile");
static_assert(SH_TILE % LG_RUN == 0, "a tile holds whole runs");

// a - b and a + b on four packed bytes
__device__ __forceinline__ uint32_t bd_sub4(uint32_t a, uint32_t b) { return ((a | BD_H) - (b & ~BD_H)) ^ ((a ^ ~b) & BD_H); }
__device__ __forceinline__ uint32_t bd_add4(uint32_t a, uint32_t b) { return ((a & ~BD_H) + (b & ~BD_H)) ^ ((a ^ b) & BD_H); }

// the byte mask of a granule whose byte k has the index (r + k) mod M: 0xFF where that index is at least T (r < M, 16 <= M)
__device__ __forceinline__ void bd_keep(uint32_t r, uint32_t M, uint32_t T, uint32_t (&m)[4])
{
    const bool inside = r + 15 < M;
    const uint32_t all = inside && r >= T ? ~0u : 0u;
    m[0] = m[1] = m[2] = m[3] = all;
    if (all || (inside && r + 15 < T)) return;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t i = r + k >= M ? r + k - M : r + k;
        m[k >> 2] |= i >= T ? 0xFFu << (8 * (k & 3)) : 0u;
    }
}

// the byte mask of a granule that is 0xFF in every byte k >= t (t <= 0: all of them)
__device__ __forceinline__ void bd_from(int t, uint32_t (&m)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) m[j] = (uint32_t)(0xFFFFFFFFull << (8 * min(max(t - 4 * j, 0), 4)));
}

// ---------------------------------------------------------------------------
// forward: bytes [a, a + cnt) of the segment at `in`; a is a multiple of RUN
// ---------------------------------------------------------------------------
template <bool STRIDED>
__device__ __forceinline__ void bd_tile_forward(const uint8_t *in, uint8_t *out, unsigned long long a, uint32_t cnt, uint32_t lag,
                                                uint32_t stride, uint32_t P, uint32_t *raw, uint32_t *above)
{
    const uint32_t tid = threadIdx.x;
    const long long ab = (long long)a - (long long)stride;     // the byte above the tile's first (below 0: in front of the segment)
    const uint32_t s = (uint32_t)(((unsigned long long)(uintptr_t)in + a) & 15);
    const uint32_t sb = (uint32_t)(((unsigned long long)(uintptr_t)in + (unsigned long long)ab) & 15);
    const uint32_t ng = (s + cnt + 15) / 16;                   // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS)
        reinterpret_cast<uint4 *>(raw + BD_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + ((long long)a - (long long)s) + 16ll * g);
    if constexpr (STRIDED) {
        const uint32_t ngb = (sb + cnt + 15) / 16;
        for (uint32_t g = tid; g < ngb; g += SH_THREADS) {
            const long long off = ab - (long long)sb + 16ll * g;   // the aligned granule's first byte in the segment
            if (off > -16) reinterpret_cast<uint4 *>(above + BD_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + off);
        }
    }
    __syncthreads();
    const uint32_t rt = STRIDED ? (uint32_t)(a % P) : 0u;      // the tile's first byte within its band
    const ShRun run = sh_run((unsigned long long)(uintptr_t)out + a, cnt);
    uint4 *dst = reinterpret_cast<uint4 *>(out + (a + run.head));
    for (uint32_t h = tid; h < run.nf; h += SH_THREADS) {
        // c: the granule, p: the 16 bytes LAG back; ca, pa: the same of the row above
        const uint32_t o = run.head + 16 * h;                  // the granule's first byte within the tile
        uint32_t c[4], p[4], m[4];
        lg_read16(raw + BD_FRONT, (int)(s + o), c);
        lg_read16(raw + BD_FRONT, (int)(s + o) - (int)lag, p);
        if constexpr (STRIDED) {
            uint32_t ca[4], pa[4];
            const uint32_t r = (rt + o) % P;
            lg_read16(above + BD_FRONT, (int)(sb + o), ca);
            lg_read16(above + BD_FRONT, (int)(sb + o) - (int)lag, pa);
            bd_keep(r, P, stride, m);
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) c[k] = bd_sub4(c[k], ca[k] & m[k]);
            bd_keep(r, P, stride + lag, m);                    // (byte i - LAG has a row above; where it is in another run it is not used)
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) p[k] = bd_sub4(p[k], pa[k] & m[k]);
        }
        bd_keep(o & (LG_RUN - 1), LG_RUN, lag, m);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) c[k] = bd_sub4(c[k], p[k] & m[k]);
        dst[h] = make_uint4(c[0], c[1], c[2], c[3]);
    }
    if (tid < 32) {                                            // the head and the tail of the tile's output run
        const bool is_head = tid < 16;
        const uint32_t y = tid & 15;
        if (y < (is_head ? run.head : run.tail)) {
            const uint8_t *rawb = reinterpret_cast<const uint8_t *>(raw + BD_FRONT), *aboveb = reinterpret_cast<const uint8_t *>(above + BD_FRONT);
            const uint32_t o = is_head ? y : run.head + 16 * run.nf + y, rr = o & (LG_RUN - 1);
            const uint32_t r = STRIDED ? (rt + o) % P : 0u;
            uint32_t v = rawb[s + o];
            if (STRIDED && r >= stride) v -= aboveb[sb + o];
            if (rr >= lag) {
                uint32_t u = rawb[s + o - lag];
                if (STRIDED && r >= stride + lag) u -= aboveb[sb + o - lag];
                v -= u;
            }
            out[a + o] = (uint8_t)v;
        }
    }
}

template <bool STRIDED>
__global__ __launch_bounds__(SH_THREADS) void k_bd_forward(const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t lag, uint32_t stride,
                                                           uint32_t P)
{
    __shared__ __attribute__((aligned(16))) uint32_t raw[BD_IMG_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t above[STRIDED ? BD_IMG_WORDS : 4];
    const unsigned long long nt = (len + SH_TILE - 1) / SH_TILE;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long a = t * SH_TILE;
        bd_tile_forward<STRIDED>(in, out, a, (uint32_t)min((unsigned long long)SH_TILE, len - a), lag, stride, P, raw, above);
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

// ---------------------------------------------------------------------------
// inverse (a): the sums down the chains of a tile's runs: cnt bytes of d at src become v at dst; src is the first byte of a run
// ---------------------------------------------------------------------------
__device__ __forceinline__ void bd_tile_scan(const uint8_t *src, uint8_t *dst, uint32_t cnt, uint32_t lag, uint32_t *imgA, uint32_t *imgB)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t s = (uint32_t)((unsigned long long)(uintptr_t)src & 15);
    const uint32_t ng = (s + cnt + 15) / 16;                   // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS)
        reinterpret_cast<uint4 *>(imgA + BD_FRONT)[g] = *reinterpret_cast<const uint4 *>(src - s + 16ull * g);
    __syncthreads();
    // v[k]: the lane's tile-aligned granule tid + 256 k; it stays in registers through the rounds
    uint32_t v[BD_PASSES][4];
    uint32_t *cur = imgB + BD_FRONT, *nxt = imgA + BD_FRONT;
#pragma unroll
    for (uint32_t k = 0; k < BD_PASSES; k++) {
        const uint32_t g = tid + SH_THREADS * k;
        lg_read16(imgA + BD_FRONT, (int)(s + 16 * g), v[k]);
        reinterpret_cast<uint4 *>(cur)[g] = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
    }
    __syncthreads();                                           // (the raw image is free from here on: it is the second flat image)
    for (uint32_t st = lag; st < LG_RUN; st <<= 1) {
#pragma unroll
        for (uint32_t k = 0; k < BD_PASSES; k++) {
            const uint32_t g = tid + SH_THREADS * k, gb = (16 * g) & (LG_RUN - 1);
            if (gb + 16 > st) {                                // (else every byte of the granule is within `st` of its run's start)
                uint32_t p[4];
                if ((st & 15) == 0) {
                    const uint4 t = reinterpret_cast<const uint4 *>(cur)[g - st / 16];
                    p[0] = t.x; p[1] = t.y; p[2] = t.z; p[3] = t.w;
                } else {
                    uint32_t m[4];
                    lg_read16(cur, (int)(16 * g) - (int)st, p);
                    bd_from((int)st - (int)gb, m);
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) p[j] &= m[j];
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) v[k][j] = bd_add4(v[k][j], p[j]);
            }
            reinterpret_cast<uint4 *>(nxt)[g] = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
        }
        __syncthreads();
        uint32_t *t = cur; cur = nxt; nxt = t;
    }
    const uint8_t *flatb = reinterpret_cast<const uint8_t *>(cur);
    const ShRun r = sh_run((unsigned long long)(uintptr_t)dst, cnt);
    uint4 *d16 = reinterpret_cast<uint4 *>(dst + r.head);
    for (uint32_t h = tid; h < r.nf; h += SH_THREADS) {        // tile bytes [head + 16 h, + 16)
        uint32_t o[4];
        lg_read16(cur, (int)(r.head + 16 * h), o);
        d16[h] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if (tid < 32) {
        const bool is_head = tid < 16;
        const uint32_t y = tid & 15;
        if (y < (is_head ? r.head : r.tail)) {
            const uint32_t p = is_head ? y : r.head + 16 * r.nf + y;
            dst[p] = flatb[p];
        }
    }
}

// bytes [first, first + count) of the segment at `in` go to out[0 .. count); first is a multiple of RUN (the whole segment: 0, len)
__global__ __launch_bounds__(SH_THREADS) void k_bd_scan(const uint8_t *in, uint8_t *out, unsigned long long first, unsigned long long count,
                                                        uint32_t lag)
{
    __shared__ __attribute__((aligned(16))) uint32_t imgA[BD_IMG_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t imgB[BD_IMG_WORDS];
    const unsigned long long nt = (count + SH_TILE - 1) / SH_TILE;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long a = t * SH_TILE;
        bd_tile_scan(in + (first + a), out + a, (uint32_t)min((unsigned long long)SH_TILE, count - a), lag, imgA, imgB);
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

// ---------------------------------------------------------------------------
// inverse (b): the sums up the bands: `count` bytes of v at `out`, byte 0 the first of a band, become x in place
// ---------------------------------------------------------------------------
struct BdVec { uint32_t w[4]; };
__device__ __forceinline__ BdVec bd_load16(const uint8_t *p) { BdVec x; __builtin_memcpy(&x, p, 16); return x; }
__device__ __forceinline__ void bd_store16(uint8_t *p, const BdVec &x) { __builtin_memcpy(p, &x, 16); }

__global__ __launch_bounds__(SH_THREADS) void k_bd_vsum(uint8_t *out, unsigned long long count, uint32_t stride, uint32_t P)
{
    const uint32_t slices = (stride + 15) / 16;
    const unsigned long long units = (count + P - 1) / P * slices;
    for (unsigned long long u = blockIdx.x * (unsigned long long)SH_THREADS + threadIdx.x; u < units; u += gridDim.x * (unsigned long long)SH_THREADS) {
        const unsigned long long band = u / slices;
        const uint32_t c = (uint32_t)(u - band * slices) * 16;                      // the slice's first column
        const uint32_t n = (uint32_t)min((unsigned long long)P, count - band * P);  // bytes of this band
        const uint32_t w = min(16u, stride - c);                                    // its columns
        uint8_t *base = out + band * P;
        if (c + stride >= n) continue;                         // (nothing below row 0 in these columns)
        if (w == 16) {
            BdVec acc = bd_load16(base + c);
            uint32_t e = c + stride;
            while (e + 16 <= n) {                              // rows whose slice lies whole in the band, BD_VSUM_ROWS loads ahead
                BdVec r[BD_VSUM_ROWS];
#pragma unroll
                for (uint32_t j = 0; j < BD_VSUM_ROWS; j++)
                    if (e + j * stride + 16 <= n) r[j] = bd_load16(base + (e + j * stride));
#pragma unroll
                for (uint32_t j = 0; j < BD_VSUM_ROWS; j++)
                    if (e + j * stride + 16 <= n) {
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++) acc.w[k] = bd_add4(acc.w[k], r[j].w[k]);
                        bd_store16(base + (e + j * stride), acc);
                    }
                e += BD_VSUM_ROWS * stride;
            }
            const uint32_t ep = c + (n - 1 - c) / stride * stride;   // the slice's place in the last row that reaches column c
            if (ep + 16 > n) {                                 // the band's last row ends inside the slice: byte by byte
#pragma unroll
                for (uint32_t k = 0; k < 16; k++)
                    if (ep + k < n) base[ep + k] = (uint8_t)(base[ep + k] + (acc.w[k >> 2] >> (8 * (k & 3))));
            }
        } else {                                               // the last stride mod 16 columns of every row
            for (uint32_t k = 0; k < w; k++) {
                uint32_t acc = base[c + k];
                for (uint32_t e = c + k + stride; e < n; e += stride) {
                    acc += base[e];
                    base[e] = (uint8_t)acc;
                }
            }
        }
    }
}

// v -> x over `count` bytes at `out`, the first of them the first of a band
static hipError_t bd_vsum_device(hipStream_t st, uint8_t *out, unsigned long long count, uint32_t stride)
{
    if (stride == 0 || count <= stride) return hipSuccess;     // (no stride, or one row: nothing above anything)
    const uint32_t P = ct_grid_period(stride);
    const unsigned long long units = (count + P - 1) / P * ((stride + 15) / 16);
    const dim3 grid((uint32_t)std::min<unsigned long long>((units + SH_THREADS - 1) / SH_THREADS, 1u << 20)), block(SH_THREADS);
    hipLaunchKernelGGL(k_bd_vsum, grid, block, 0, st, out, count, stride, P);
    return hipGetLastError();
}

static hipError_t bd_scan_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long first, unsigned long long count, uint32_t lag)
{
    const unsigned long long nt = (count + SH_TILE - 1) / SH_TILE;
    const dim3 grid((uint32_t)std::min<unsigned long long>(nt, 1u << 24)), block(SH_THREADS);   // (one workgroup per tile up to 256 GiB)
    hipLaunchKernelGGL(k_bd_scan, grid, block, 0, st, in, out, first, count, lag);
    return hipGetLastError();
}

hipError_t byte_delta_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t lag, uint32_t stride, bool inverse)
{
    if (!ct_byte_lag_ok(lag) || !ct_byte_stride_ok(stride)) return hipErrorInvalidValue;
    if (len == 0) return hipSuccess;
    if (inverse) {
        const hipError_t e = bd_scan_device(st, in, out, 0, len, lag);
        return e != hipSuccess ? e : bd_vsum_device(st, out, len, stride);
    }
    const unsigned long long nt = (len + SH_TILE - 1) / SH_TILE;
    const dim3 grid((uint32_t)std::min<unsigned long long>(nt, 1u << 24)), block(SH_THREADS);
    if (stride) hipLaunchKernelGGL(k_bd_forward<true>, grid, block, 0, st, in, out, len, lag, stride, ct_grid_period(stride));
    else hipLaunchKernelGGL(k_bd_forward<false>, grid, block, 0, st, in, out, len, lag, 0u, (uint32_t)LG_RUN);
    return hipGetLastError();
}

// the range form of the inverse: `first` is a multiple of RUN, with a stride of P, so out[0] is the first byte of a run or a band
hipError_t unbyte_delta_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t lag, uint32_t stride,
                                     unsigned long long first, unsigned long long count)
{
    if (!ct_byte_lag_ok(lag) || !ct_byte_stride_ok(stride) || first > len || count > len - first) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (first % ct_byte_step(stride)) return hipErrorInvalidValue;
    const hipError_t e = bd_scan_device(st, in, out, first, count, lag);
    return e != hipSuccess ? e : bd_vsum_device(st, out, count, stride);
}

} // namespace glc
