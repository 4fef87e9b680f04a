// byte_probe.hip -- the byte probe (INTEGRATION.md 4b "Filter: auto with bytes"; the sums, the winners, the planes and the costs are
// defined in byte_rule.h): which lag and which row stride of the byte predictor (byte_delta.hip) a segment wants, and what its two
// outputs would cost.  gfx950 / wave64.
//   k_bp_lags     the 16 lag sums A[l] of a segment.  The span geometry is k_lp_sums': a workgroup of 256 lanes owns a span of the
//                 segment, a multiple of 16 KiB, so every run head (2048 bytes) is found from the offset alone and nothing in front
//                 of a span is read.  A span goes through LDS a 16 KiB tile at a time with 16 bytes in front of it.  A lane takes
//                 16-byte granules: the granule and the 16 bytes in front of it are 8 registers, every lag a fixed v_alignbyte of
//                 that window.  Per lag and dword: the SWAR subtract of byte_delta.hip, the sign mask, an xor (a byte d >= 128
//                 becomes 255 - d) and v_sad_u8 against zero into one of 16 accumulators.  The window's bytes in front of a run
//                 head are zeroed in place (a granule never straddles one).  32-bit accumulators (a lane's share of the largest
//                 span, 2 MiB, is below 2^20 a sum); they leave by a wave reduction, LDS, and one 64-bit atomic per (workgroup, sum).
//   k_bp_init     a segment's 65537 stride sums: 0 where a stride is a candidate (17 .. Wmax, 1024 counted bytes or more),
//                 0xFFFFFFFF everywhere else.
//   k_bp_strides  the stride sums: k_gw_sums' 32-bit form (grid_probe.hip) restated for bytes, widened to dwords as its 2-byte
//                 elements are -- one workgroup per (segment, tile of 256 targets, chunk of 4096 strides), a lane owns 16
//                 consecutive strides, the history in a register window, LDS position p at p + p / 16.
//   k_bp_argmin   one workgroup per segment: the lag and the stride with the smallest sums (ties to the smallest; stride 0 where
//                 there is no candidate) to device memory, so that the host is not involved between the two probes.
//   k_bp_planes   both histograms from one read: byte_delta.hip's forward tile (two raw LDS images, the second `stride` back,
//                 each at its own alignment) builds the (lag, 0) output and the (lag, stride) output of a granule, and
//                 plane_hist.h counts both (two LDS counter copies, the uniform-value shortcut).  The lag word is used as
//                 ((v - 1) & 15) + 1; a stride word outside 17 .. 65536 names no stride: row 1 stays zero, and the word is never a
//                 distance.
//   k_bp_cost     the two costs of a segment from its two rows: one wave per row, k_lp_cost's code.
// Any segment length up to 2^31, any byte alignment; only the first L - L % 8 bytes are counted.
#include "container_internal.h"
#include "glc_device.h"
#include "byte_rule.h"
#include "lag_tile.h"
#include "plane_hist.h"

namespace glc {

constexpr uint32_t BP_THREADS = 256, BP_TILE = 16384;
constexpr uint32_t BP_FRONT = 4;                               // words in front of a tile's image: the longest way back
constexpr uint32_t BP_RAW_WORDS = BP_FRONT + BP_TILE / 4;
constexpr uint32_t BP_MIN_SPAN = 4 * BP_TILE, BP_MAX_SPANS = 1024;
constexpr uint32_t BP_H = 0x80808080u;
// the stride sums: k_gw_sums' geometry
constexpr uint32_t BP_OWN = 16;                                // consecutive strides a lane owns; targets a step
constexpr uint32_t BP_CHUNK = BP_THREADS * BP_OWN;             // strides a workgroup
constexpr uint32_t BP_CHUNKS = (BYTE_S_MAX - BYTE_S_MIN + BP_CHUNK) / BP_CHUNK;       // 16
constexpr uint32_t BP_HIST = BP_CHUNK + GRID_TILE - 1;         // history bytes a workgroup reaches
constexpr uint32_t BP_HIST_WORDS = BP_HIST + BP_HIST / BP_OWN + 1;
constexpr uint32_t BP_WINDOW = 2 * BP_OWN - 1;
constexpr uint32_t BP_ARGMIN_THREADS = 1024;
// the planes: byte_delta.hip's images
constexpr uint32_t BP_IMG_FRONT = 4;                           // words in front of an image (a read starts up to 16 bytes early)
constexpr uint32_t BP_IMG_WORDS = BP_IMG_FRONT + 4 * SH_NGI;
constexpr uint32_t BP_COPIES = 2, BP_PITCH = 257;
constexpr uint32_t BP_PLANE_BLOCKS = 1024;                     // workgroups a segment's tiles are dealt to
static_assert(BP_TILE % BYTE_RUN == 0 && BYTE_RUN == LG_RUN && BP_TILE == SH_TILE, "a tile holds whole runs");
static_assert(GRID_TILE % BP_OWN == 0 && BP_CHUNKS * BP_CHUNK >= BYTE_S_MAX - BYTE_S_MIN + 1, "the chunks cover every stride");
static_assert(BYTE_LAGS * 1 <= 4 * BP_FRONT, "the window reaches the longest lag");

__device__ __forceinline__ uint32_t bp_len(const unsigned long long *len, uint32_t i, uint32_t max_len)
{
    const unsigned long long l = len[i];
    return (l > max_len ? max_len : (uint32_t)l) & ~7u;
}

// a - b on four packed bytes (byte_delta.hip's bd_sub4)
__device__ __forceinline__ uint32_t bp_sub4(uint32_t a, uint32_t b) { return ((a | BP_H) - (b & ~BP_H)) ^ ((a ^ ~b) & BP_H); }

// ---------------------------------------------------------------------------
// the lag sums
// ---------------------------------------------------------------------------
// eight bytes at p as two dwords
__device__ __forceinline__ uint2 bp_load8(const uint8_t *p, bool aligned)
{
    if (aligned) return *reinterpret_cast<const uint2 *>(p);
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint2(w[0], w[1]);
}

// bytes [t, t + n) of the segment at `in` (n a multiple of 8, at most a tile) to the image behind the front words of raw
__device__ __forceinline__ void bp_stage(const uint8_t *in, bool al, uint32_t t, uint32_t n, uint32_t *raw)
{
    for (uint32_t o = 16 * threadIdx.x; o < n; o += 16 * BP_THREADS) {
        uint32_t *dst = raw + BP_FRONT + o / 4;
        if (al && n - o >= 16) {
            *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(in + t + o);
        } else {
            const uint2 q = bp_load8(in + t + o, al);
            dst[0] = q.x; dst[1] = q.y;
            if (n - o >= 16) { const uint2 r = bp_load8(in + t + o + 8, al); dst[2] = r.x; dst[3] = r.y; }
        }
    }
}

// what the granule in w[4 ..] (HALF: its first eight bytes) adds to the 16 sums; w[0 .. 3] the 16 bytes in front of it
template <bool HALF>
__device__ __forceinline__ void bp_granule(const uint32_t (&w)[2 * BP_FRONT], uint32_t (&acc)[BYTE_LAGS])
{
    constexpr uint32_t ND = HALF ? 2 : 4;                      // the granule's dwords that count
#pragma unroll
    for (uint32_t l = 1; l <= BYTE_LAGS; l++) {
#pragma unroll
        for (uint32_t m = 0; m < ND; m++) {
            const uint32_t b = 4 * BP_FRONT + 4 * m - l;       // the window byte the predecessors start at: 0 .. 27
            const uint32_t p = (b & 3) ? __builtin_amdgcn_alignbyte(w[b / 4 + 1], w[b / 4], b & 3) : w[b / 4];
            const uint32_t d = bp_sub4(w[BP_FRONT + m], p);
            const uint32_t s = d & BP_H;                       // a byte of 128 and more becomes 255 - d = ~d
            acc[l - 1] = __builtin_amdgcn_sad_u8(d ^ (s | (s - (s >> 7))), 0u, acc[l - 1]);
        }
    }
}

__global__ __launch_bounds__(BP_THREADS) void k_bp_lags(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                        const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                        uint32_t span, unsigned long long *__restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) uint32_t raw[BP_RAW_WORDS];
    __shared__ uint32_t s_red[BP_THREADS / 64][BYTE_LAGS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t P = bp_len(data_len, b, max_len);
    const unsigned long long s0 = (unsigned long long)blockIdx.y * span;
    if (s0 >= P) return;
    const uint32_t t0 = (uint32_t)s0, t1 = P - t0 > span ? t0 + span : P;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    if (tid < BP_FRONT) raw[tid] = 0;                          // (every tile starts a run: never a predecessor)
    uint32_t acc[BYTE_LAGS];
#pragma unroll
    for (uint32_t i = 0; i < BYTE_LAGS; i++) acc[i] = 0;
    for (uint32_t t = t0; t < t1; t += BP_TILE) {
        const uint32_t n = min(BP_TILE, t1 - t);               // a multiple of 8
        __syncthreads();                                       // (the tile before has been read)
        bp_stage(in, al, t, n, raw);
        __syncthreads();
        for (uint32_t o = 16 * tid; o < n; o += 16 * BP_THREADS) {
            uint32_t w[2 * BP_FRONT];
            const uint4 *src = reinterpret_cast<const uint4 *>(raw + o / 4);      // 16 bytes in front of the granule
            const uint4 f = src[0], g = src[1];
            const bool head = (o & (BYTE_RUN - 1)) == 0;       // what lies in front of a run head counts as zero
            w[0] = head ? 0u : f.x; w[1] = head ? 0u : f.y; w[2] = head ? 0u : f.z; w[3] = head ? 0u : f.w;
            w[4] = g.x; w[5] = g.y; w[6] = g.z; w[7] = g.w;
            if (n - o >= 16) bp_granule<false>(w, acc);
            else bp_granule<true>(w, acc);
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < BYTE_LAGS; i++) {
        const uint32_t v = wave_sum(acc[i]);
        if (lane == 0) s_red[wave][i] = v;
    }
    __syncthreads();
    if (tid < BYTE_LAGS) {
        unsigned long long v = 0;
#pragma unroll
        for (uint32_t k = 0; k < BP_THREADS / 64; k++) v += s_red[k][tid];
        if (v) atomicAdd(&sums[(size_t)b * BYTE_LAGS + tid], v);
    }
}

// ---------------------------------------------------------------------------
// the stride sums
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BP_THREADS) void k_bp_init(const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                        uint32_t *__restrict__ sums)
{
    const uint32_t b = blockIdx.x;
    const uint32_t N = bp_len(data_len, b, max_len);
    const uint32_t wmax = N < BYTE_MIN_LEN ? 0u : grid_wmax(N);
    uint32_t *row = sums + (size_t)b * BYTE_SUM_ROW;
    for (uint32_t w = threadIdx.x; w < BYTE_SUM_ROW; w += BP_THREADS) row[w] = w >= BYTE_S_MIN && w <= wmax ? 0u : GRID_NO_SUM;
}

// the leading zeros of the folded difference of two bytes, counted in 32 bits: 32 less bitlen(fold((x - p) mod 256))
__device__ __forceinline__ uint32_t bp_pair_clz(uint32_t x, uint32_t p)
{
    const int d = (int)((x - p) << 24) >> 24;                  // (the difference modulo 2^8, its sign spread)
    const uint32_t f = ((uint32_t)d << 1) ^ (uint32_t)(d >> 31);
    return (uint32_t)__clz((int)f);
}

// grid: (segments, 32 tiles x 16 chunks)
__global__ __launch_bounds__(BP_THREADS) void k_bp_strides(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                           const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                           uint32_t *__restrict__ sums)
{
    __shared__ uint32_t hist[BP_HIST_WORDS];
    __shared__ uint32_t tgt[GRID_TILE];
    const uint32_t b = blockIdx.x, y = blockIdx.y, tid = threadIdx.x;
    const uint32_t t = y / BP_CHUNKS, c = y % BP_CHUNKS;
    const uint32_t N = bp_len(data_len, b, max_len);
    if (N < BYTE_MIN_LEN) return;
    const uint32_t wmax = grid_wmax(N), wlo = BYTE_S_MIN + c * BP_CHUNK;
    if (wlo > wmax) return;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const unsigned long long bt = grid_tile_start(N, wmax, t);  // bt + 256 <= N
    uint32_t *row = sums + (size_t)b * BYTE_SUM_ROW;
    // history position p is byte hb + p; the pair (target j, stride W) meets position j + BP_CHUNK - 1 - (W - wlo).  Positions in
    // front of the segment belong to strides above wmax alone, which are not written; the last position is byte bt + 254 - wlo
    const long long hb = (long long)bt - (long long)wlo - (long long)(BP_CHUNK - 1);
    for (uint32_t p = tid; p < BP_HIST; p += BP_THREADS) {
        const long long i = hb + (long long)p;
        hist[p + p / BP_OWN] = i >= 0 ? (uint32_t)in[i] : 0u;
    }
    tgt[tid] = in[bt + tid];
    __syncthreads();
    // this lane's strides: wlo + BP_OWN tid + r; target jb + s meets window element s - r + BP_OWN - 1 of the window at position q0 + jb
    const uint32_t q0 = BP_CHUNK - BP_OWN * (tid + 1);
    uint32_t acc[BP_OWN], win[BP_WINDOW];
#pragma unroll
    for (uint32_t r = 0; r < BP_OWN; r++) acc[r] = 0;
    const uint32_t *h = hist + q0 + q0 / BP_OWN;
#pragma unroll
    for (uint32_t i = 0; i < BP_OWN - 1; i++) win[i] = h[i];
#pragma unroll 1
    for (uint32_t jb = 0; jb < GRID_TILE; jb += BP_OWN) {
        uint32_t x[BP_OWN];
#pragma unroll
        for (uint32_t s = 0; s < BP_OWN; s++) x[s] = tgt[jb + s];
#pragma unroll
        for (uint32_t i = BP_OWN - 1; i < BP_WINDOW; i++) win[i] = h[i + i / BP_OWN];
#pragma unroll
        for (uint32_t s = 0; s < BP_OWN; s++) {
#pragma unroll
            for (uint32_t r = 0; r < BP_OWN; r++) acc[r] += bp_pair_clz(x[s], win[s - r + BP_OWN - 1]);
        }
#pragma unroll
        for (uint32_t i = 0; i < BP_OWN - 1; i++) win[i] = win[i + BP_OWN];
        h += BP_OWN + 1;
    }
#pragma unroll
    for (uint32_t r = 0; r < BP_OWN; r++) {
        const uint32_t W = wlo + BP_OWN * tid + r;
        if (W <= wmax) atomicAdd(&row[W], 32u * GRID_TILE - acc[r]);
    }
}

// grid: (segments); winners: {lag, stride} a segment
__global__ __launch_bounds__(BP_ARGMIN_THREADS) void k_bp_argmin(const unsigned long long *__restrict__ lag_sums, const uint32_t *__restrict__ sums,
                                                                 const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                                 uint32_t *__restrict__ winners)
{
    __shared__ unsigned long long s_key[BP_ARGMIN_THREADS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t N = bp_len(data_len, b, max_len);
    if (tid == 0) winners[(size_t)b * 2] = byte_lag_argmin(lag_sums + (size_t)b * BYTE_LAGS);
    if (N < BYTE_MIN_LEN) {
        if (tid == 0) winners[(size_t)b * 2 + 1] = 0;
        return;
    }
    const uint32_t wmax = grid_wmax(N);
    const uint32_t *row = sums + (size_t)b * BYTE_SUM_ROW;
    unsigned long long key = ~0ull;                            // (sum, stride): the smallest key is the winner
#pragma unroll 8
    for (uint32_t w = BYTE_S_MIN + tid; w <= wmax; w += BP_ARGMIN_THREADS) {
        const unsigned long long v = (unsigned long long)row[w] << 32 | w;
        key = v < key ? v : key;
    }
    s_key[tid] = key;
    __syncthreads();
    for (uint32_t m = BP_ARGMIN_THREADS / 2; m >= 1; m >>= 1) {
        if (tid < m) s_key[tid] = s_key[tid + m] < s_key[tid] ? s_key[tid + m] : s_key[tid];
        __syncthreads();
    }
    if (tid == 0) winners[(size_t)b * 2 + 1] = (uint32_t)s_key[0];
}

// ---------------------------------------------------------------------------
// the planes: byte_delta.hip's forward tile, counted instead of stored
// ---------------------------------------------------------------------------
// the byte mask of a granule whose byte k has the index (r + k) mod M: 0xFF where that index is at least T (r < M, 16 <= M)
__device__ __forceinline__ void bp_keep(uint32_t r, uint32_t M, uint32_t T, uint32_t (&m)[4])
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

// grid: (segments, up to BP_PLANE_BLOCKS); words: {lag, stride} a segment
__global__ __launch_bounds__(SH_THREADS) void k_bp_planes(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                          const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                          const uint32_t *__restrict__ words, uint32_t *__restrict__ planes)
{
    __shared__ __attribute__((aligned(16))) uint32_t raw[BP_IMG_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t above[BP_IMG_WORDS];
    __shared__ uint32_t s_h[BP_COPIES * BYTE_ROWS * BP_PITCH];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t len = bp_len(data_len, b, max_len);
    const uint32_t nt = (len + SH_TILE - 1) / SH_TILE;
    if (len < BYTE_MIN_LEN || blockIdx.y >= nt) return;
    const uint32_t lag = lag_clamp(words[(size_t)b * 2]), stride = byte_stride_word(words[(size_t)b * 2 + 1]);
    const uint32_t P = stride ? ct_grid_period(stride) : LG_RUN;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    for (uint32_t i = tid; i < BP_COPIES * BYTE_ROWS * BP_PITCH; i += SH_THREADS) s_h[i] = 0;
    uint32_t *H = s_h + (tid & (BP_COPIES - 1)) * BYTE_ROWS * BP_PITCH;
    for (uint32_t t = blockIdx.y; t < nt; t += gridDim.y) {
        const uint32_t a = t * SH_TILE, cnt = min(SH_TILE, len - a);               // cnt: a multiple of 8
        __syncthreads();                                       // (the tile before has been read; the counters are zero)
        // the tile's bytes and, with a stride, the bytes `stride` in front of them as aligned 16-byte granules, each image at its
        // own alignment; no granule wholly in front of the segment is read (its bytes have an index below the stride)
        const long long ab = (long long)a - (long long)stride;
        const uint32_t s = (uint32_t)(((unsigned long long)(uintptr_t)in + a) & 15);
        const uint32_t sb = (uint32_t)(((unsigned long long)(uintptr_t)in + (unsigned long long)ab) & 15);
        const uint32_t ng = (s + cnt + 15) / 16, ngb = (sb + cnt + 15) / 16;       // <= SH_NGI
        for (uint32_t g = tid; g < ng; g += SH_THREADS)
            reinterpret_cast<uint4 *>(raw + BP_IMG_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + ((long long)a - (long long)s) + 16ll * g);
        if (stride) {
            for (uint32_t g = tid; g < ngb; g += SH_THREADS) {
                const long long off = ab - (long long)sb + 16ll * g;               // the aligned granule's first byte in the segment
                if (off > -16) reinterpret_cast<uint4 *>(above + BP_IMG_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + off);
            }
        }
        __syncthreads();
        const uint32_t nge = (cnt + 15) / 16, rt = a % P;
        for (uint32_t g0 = wave * 64; g0 < nge; g0 += SH_THREADS) {
            const uint32_t g = g0 + lane, o = 16 * g;
            const uint32_t n = g < nge ? min(16u, cnt - o) : 0u;                   // 0, 8 or 16
            const bool whole = cnt - 16 * g0 >= 1024;          // wave-uniform
            uint32_t d0[4] = {0, 0, 0, 0}, d1[4] = {0, 0, 0, 0};
            if (n) {
                // c: the granule, p: the 16 bytes `lag` back; ca, pa: the same of the row above
                uint32_t c[4], p[4], mr[4], m[4];
                lg_read16(raw + BP_IMG_FRONT, (int)(s + o), c);
                lg_read16(raw + BP_IMG_FRONT, (int)(s + o) - (int)lag, p);
                bp_keep(o & (LG_RUN - 1), LG_RUN, lag, mr);
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) d0[k] = bp_sub4(c[k], p[k] & mr[k]);
                if (stride) {
                    uint32_t ca[4], pa[4];
                    const uint32_t r = (rt + o) % P;
                    lg_read16(above + BP_IMG_FRONT, (int)(sb + o), ca);
                    lg_read16(above + BP_IMG_FRONT, (int)(sb + o) - (int)lag, pa);
                    bp_keep(r, P, stride, m);
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) c[k] = bp_sub4(c[k], ca[k] & m[k]);
                    bp_keep(r, P, stride + lag, m);            // (byte i - lag has a row above; where it is in another run it is not used)
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) p[k] = bp_sub4(p[k], pa[k] & m[k]);
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++) d1[k] = bp_sub4(c[k], p[k] & mr[k]);
                }
            }
            ph_group<BP_PITCH>(H, d0, n, whole, 0, 1, lane);
            if (stride) ph_group<BP_PITCH>(H, d1, n, whole, 1, 1, lane);
        }
    }
    __syncthreads();
    uint32_t *out = planes + (size_t)b * BYTE_ROWS * 256;
    for (uint32_t i = tid; i < BYTE_ROWS * 256; i += SH_THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < BP_COPIES; k++) c += s_h[k * BYTE_ROWS * BP_PITCH + (i >> 8) * BP_PITCH + (i & 255u)];
        if (c) atomicAdd(&out[i], c);
    }
}

__device__ __forceinline__ unsigned long long bp_wave_sum64(unsigned long long x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += (unsigned long long)__shfl_xor((long long)x, m, 64);
    return x;
}

// grid: (segments); one wave per row
__global__ __launch_bounds__(BYTE_ROWS * 64) void k_bp_cost(const uint32_t *__restrict__ planes, const unsigned long long *__restrict__ data_len,
                                                            uint32_t max_len, const uint32_t *__restrict__ words,
                                                            unsigned long long *__restrict__ costs)
{
    const uint32_t b = blockIdx.x, row = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint4 q = *reinterpret_cast<const uint4 *>(planes + ((size_t)b * BYTE_ROWS + row) * 256 + 4 * lane);
    const uint32_t h[4] = {q.x, q.y, q.z, q.w};
    const unsigned long long N = bp_wave_sum64((unsigned long long)h[0] + h[1] + h[2] + h[3]);
    unsigned long long c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) c += filter_symbol_cost(h[k], N);
    c = bp_wave_sum64(c);
    if (lane == 0) {
        const bool cand = bp_len(data_len, b, max_len) >= BYTE_MIN_LEN && (row == 0 || byte_stride_word(words[(size_t)b * 2 + 1]));
        costs[(size_t)b * BYTE_ROWS + row] = cand ? c : GRID_NO_COST;
    }
}

// spans: multiples of 16 KiB, at least BP_MIN_SPAN, at most BP_MAX_SPANS of them a segment
static dim3 bp_grid(uint32_t count, uint32_t max_len, uint32_t *span)
{
    const unsigned long long tiles = ((unsigned long long)max_len + BP_TILE - 1) / BP_TILE;
    unsigned long long per = (tiles + BP_MAX_SPANS - 1) / BP_MAX_SPANS;
    if (per < BP_MIN_SPAN / BP_TILE) per = BP_MIN_SPAN / BP_TILE;
    *span = (uint32_t)(per * BP_TILE);
    return dim3(count, (uint32_t)((tiles + per - 1) / per));
}

hipError_t byte_probe_sums(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                           uint32_t count, uint32_t max_len, unsigned long long *lag_sums, uint32_t *stride_sums, uint32_t *winners)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(lag_sums, 0, (size_t)count * BYTE_LAGS * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bp_init, dim3(count), dim3(BP_THREADS), 0, st, data_len, max_len, stride_sums);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (max_len >= 8) {
        uint32_t span;
        const dim3 grid = bp_grid(count, max_len, &span);
        hipLaunchKernelGGL(k_bp_lags, grid, dim3(BP_THREADS), 0, st, data, data_off, data_len, max_len, span, lag_sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (max_len >= BYTE_MIN_LEN) {
        hipLaunchKernelGGL(k_bp_strides, dim3(count, GRID_TILES * BP_CHUNKS), dim3(BP_THREADS), 0, st, data, data_off, data_len, max_len,
                           stride_sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bp_argmin, dim3(count), dim3(BP_ARGMIN_THREADS), 0, st, lag_sums, stride_sums, data_len, max_len, winners);
    return hipGetLastError();
}

// grid: (ceil(segments / 256)); words: {the winner of the segment's lag sums, stride 0}
__global__ __launch_bounds__(BP_THREADS) void k_bp_lag_words(const unsigned long long *__restrict__ lag_sums, uint32_t count, uint32_t *__restrict__ words)
{
    const uint32_t b = blockIdx.x * BP_THREADS + threadIdx.x;
    if (b >= count) return;
    words[(size_t)b * 2] = byte_lag_argmin(lag_sums + (size_t)b * BYTE_LAGS);
    words[(size_t)b * 2 + 1] = 0;
}

hipError_t byte_probe_lags(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                           uint32_t count, uint32_t max_len, unsigned long long *lag_sums, uint32_t *words)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(lag_sums, 0, (size_t)count * BYTE_LAGS * 8, st);
    if (e != hipSuccess) return e;
    if (max_len >= 8) {
        uint32_t span;
        const dim3 grid = bp_grid(count, max_len, &span);
        hipLaunchKernelGGL(k_bp_lags, grid, dim3(BP_THREADS), 0, st, data, data_off, data_len, max_len, span, lag_sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bp_lag_words, dim3((count + BP_THREADS - 1) / BP_THREADS), dim3(BP_THREADS), 0, st, lag_sums, count, words);
    return hipGetLastError();
}

hipError_t byte_probe_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                             uint32_t count, uint32_t max_len, const uint32_t *words, uint32_t *planes, unsigned long long *costs)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(planes, 0, (size_t)count * BYTE_ROWS * 1024, st);
    if (e != hipSuccess) return e;
    if (max_len >= BYTE_MIN_LEN) {
        const uint32_t nt = (uint32_t)(((unsigned long long)max_len + SH_TILE - 1) / SH_TILE);
        hipLaunchKernelGGL(k_bp_planes, dim3(count, std::min(nt, BP_PLANE_BLOCKS)), dim3(SH_THREADS), 0, st, data, data_off, data_len, max_len,
                           words, planes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bp_cost, dim3(count), dim3(BYTE_ROWS * 64), 0, st, planes, data_len, max_len, words, costs);
    return hipGetLastError();
}

} // namespace glc
