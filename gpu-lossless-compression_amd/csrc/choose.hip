// choose.hip -- the bigram probe of the container's CHOOSE codec (INTEGRATION.md 4b "choose", choose_rule.h).  gfx950 / wave64.
//   k_ch_probe    one workgroup of 1024 lanes per segment.  For 2 <= p < L the key of position p is the hashed two-byte context
//                 ctx = (31 x[p-2] + x[p-1]) & 255 and the symbol x[p]; the kernel counts every key exactly and gives the
//                 segment's {S2, SR, SC, M} (choose_rule.h).  The table of 256 x 256 counts is kept in LDS as 32-bit counters,
//                 one half of the contexts at a time: 128 rows of 256 counters = 128 KiB of the CU's 160 KiB, two passes over
//                 the segment (the second reads what the first left in the caches), every count exact up to the 2^20 - 2 one
//                 cell can hold.  A wave takes 1 KiB a step, a lane 16 bytes of it and the two bytes in front (the lane before
//                 it has them; lane 0 reads them).  A lane whose 18 bytes are one value has 16 equal keys and adds 16 with ONE
//                 atomic, and a wave of such lanes of one value adds 1024 with one (a block of zeros would otherwise serialise
//                 every atomic on one address); the other lanes count their 16 positions one by one, without any validity
//                 test where the wave's whole step lies inside the segment.  Within a row the cells are rotated by the
//                 context, so that a frequent symbol's counters spread over the LDS banks.  Behind a pass the row sums (a wave
//                 per row), the sum of N (N - 1) and the column sums (into a 256-entry side table that both passes add to)
//                 come from reads of the table, no second set of atomics.
//   k_ch_probe16  the same four words in ONE pass for segments of up to 65 536 bytes: no cell passes 65 534 there, so the table is
//                 kept as 16-bit counters, two to a dword, all 256 rows in the same 128 KiB.  bigram_probe_segments takes it when
//                 max_len <= 65536.
// Any segment length up to 2^20, any byte alignment (16-byte loads where the segment's address allows).
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t CH_THREADS = 1024, CH_WAVES = CH_THREADS / 64, CH_STEP = 1024, CH_ROWS = 128;

// sum over the wave of values below 2^52 (two 32-bit sums of 26-bit halves)
__device__ __forceinline__ unsigned long long ch_wave_sum(unsigned long long x)
{
    const uint32_t lo = wave_sum((uint32_t)x & 0x3FFFFFFu), hi = wave_sum((uint32_t)(x >> 26));
    return ((unsigned long long)hi << 26) + lo;
}

// a lane's 16 positions of one pass: the key of position k is (ctx, sym) with ctx from the two bytes in front; those of this
// pass's half of the contexts are counted.  Row ctx & 127 keeps symbol b in cell (b + ctx) & 255: the LDS bank of a counter is
// its cell's low five bits, and frequent symbols would otherwise pile the lanes of a wave onto a few banks whatever their rows.
// CHECKED: bit k of vm says whether position k exists (the block's first two bytes have no context, the last step may be short)
template <bool CHECKED>
__device__ __forceinline__ void ch_steps(uint32_t *s_t, const uint32_t (&w)[4], uint32_t front, uint32_t half, uint32_t vm)
{
    uint32_t x2 = front & 255u, x1 = front >> 8;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t sym = (w[k >> 2] >> (8 * (k & 3))) & 255u, ctx = 31u * x2 + x1;       // (ctx: its low 8 bits)
        bool mine = ((ctx >> 7) & 1u) == half;
        if (CHECKED) mine = mine && ((vm >> k) & 1u) != 0;
        if (mine) atomicAdd(&s_t[(ctx & 127u) << 8 | ((sym + ctx) & 255u)], 1u);
        x2 = x1; x1 = sym;
    }
}

__global__ __launch_bounds__(CH_THREADS) void k_ch_probe(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                         const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                         unsigned long long *__restrict__ stats)
{
    __shared__ uint4 s_t4[CH_ROWS * 256 / 4];
    __shared__ uint32_t s_c[256];
    __shared__ unsigned long long s_sum[3];
    uint32_t *s_t = reinterpret_cast<uint32_t *>(s_t4);
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long l64 = data_len[b];
    const uint32_t L = l64 > max_len ? max_len : (uint32_t)l64;
    unsigned long long *out = stats + (size_t)CHOOSE_STATS * b;
    if (L < 3) {                                               // no position, or one: nothing can collide
        if (tid < CHOOSE_STATS) out[tid] = tid == 3 && L == 3 ? 1ull : 0ull;
        return;
    }
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    if (tid < 256) s_c[tid] = 0;
    if (tid < 3) s_sum[tid] = 0;
    unsigned long long s2 = 0, sr = 0;
    for (uint32_t half = 0; half < 2; half++) {
        for (uint32_t i = tid; i < CH_ROWS * 256 / 4; i += CH_THREADS) s_t4[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        for (uint32_t o0 = wave * CH_STEP; o0 < L; o0 += CH_WAVES * CH_STEP) {     // (wave-uniform)
            const uint32_t o = o0 + 16 * lane, n = o < L ? min(16u, L - o) : 0u;
            uint32_t w[4] = {0, 0, 0, 0};
            if (al && n == 16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(in + o);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 16; k++) if (k < n) w[k >> 2] |= (uint32_t)in[o + k] << (8 * (k & 3));
            }
            // the two bytes in front of the lane's 16: the last two of the lane before it; lane 0 reads them (none at p = 0)
            uint32_t front = wave_prev(w[3]) >> 16;
            if (lane == 0) front = o0 ? (uint32_t)in[o0 - 2] | (uint32_t)in[o0 - 1] << 8 : 0u;
            // a lane whose 18 bytes are one value has 16 equal keys: one atomic; a wave of such lanes of one value: one for all
            const uint32_t b0 = w[0] & 255u, rep = b0 * 0x01010101u;
            const bool uni = n == 16 && o0 != 0 && w[0] == rep && w[1] == rep && w[2] == rep && w[3] == rep && front == (rep & 0xFFFFu);
            const uint32_t uctx = (32u * b0) & 255u, ucell = (uctx & 127u) << 8 | ((b0 + uctx) & 255u);
            const bool umine = (uctx >> 7) == half;
            if (__ballot(!uni) == 0 && __ballot(b0 != (uint32_t)__builtin_amdgcn_readfirstlane((int)b0)) == 0) {
                if (lane == 0 && umine) atomicAdd(&s_t[ucell], CH_STEP);
                continue;
            }
            if (uni) {
                if (umine) atomicAdd(&s_t[ucell], 16u);
            } else if (o0 != 0 && o0 + CH_STEP <= L) {               // (wave-uniform: every lane has 16 bytes behind two more)
                ch_steps<false>(s_t, w, front, half, 0u);
            } else if (n) {
                const uint32_t lo = o >= 2 ? 0u : 2u - o;
                ch_steps<true>(s_t, w, front, half, ((1u << n) - 1u) & ~((1u << lo) - 1u));
            }
        }
        __syncthreads();
        // behind the pass: every row's sum and its cells' N (N - 1), a wave per row; the column sums, a lane per column
        for (uint32_t r = wave; r < CH_ROWS; r += CH_WAVES) {
            uint32_t rs = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t v = s_t[r * 256 + 64 * k + lane];
                rs += v;
                s2 += (unsigned long long)v * (v - 1u);        // (v = 0: 0 times anything)
            }
            rs = wave_sum(rs);
            if (lane == 0) sr += (unsigned long long)rs * (rs - 1u);
        }
        if (tid < 256) {
            uint32_t c = 0;
            for (uint32_t r = 0; r < CH_ROWS; r++) c += s_t[r * 256 + ((tid + r + 128u * half) & 255u)];
            s_c[tid] += c;
        }
        __syncthreads();
    }
    unsigned long long sc = 0;
    if (tid < 256) { const uint32_t c = s_c[tid]; sc = (unsigned long long)c * (c - 1u); }
    // (a lane's partial sums stay below the segment's M (M - 1) < 2^40)
    s2 = ch_wave_sum(s2); sr = ch_wave_sum(sr); sc = ch_wave_sum(sc);
    if (lane == 0) { atomicAdd(&s_sum[0], s2); atomicAdd(&s_sum[1], sr); atomicAdd(&s_sum[2], sc); }
    __syncthreads();
    if (tid < CHOOSE_STATS) out[tid] = tid < 3 ? s_sum[tid] : (unsigned long long)(L - 2);
}

// ---------------------------------------------------------------------------
// the one-pass form for segments of up to 65 536 bytes: every cell is at most M = L - 2 <= 65 534, so the whole table fits the same
// 128 KiB as 16-bit counters, two to a dword.  Row ctx keeps symbol b at r = (b + ctx) & 255: dword r & 127 of the row, its upper
// half where r >= 128.  A 32-bit atomic add of 1 or 1 << 16 cannot carry from the lower half (no cell passes 65 534), so it is
// exact.  A row is 128 dwords, a multiple of the bank count, so the bank of a counter is the low bits of b + ctx whatever its row.
// ---------------------------------------------------------------------------
constexpr uint32_t CH16_MAX_LEN = 65536, CH16_ROW = 128;
__device__ __forceinline__ uint32_t ch16_cell(uint32_t ctx, uint32_t sym) { return (ctx & 255u) * CH16_ROW + ((sym + ctx) & 127u); }
__device__ __forceinline__ uint32_t ch16_one(uint32_t ctx, uint32_t sym) { return 1u << (((sym + ctx) >> 3) & 16u); }     // (bit 7 of r picks the half)

template <bool CHECKED>
__device__ __forceinline__ void ch16_steps(uint32_t *s_t, const uint32_t (&w)[4], uint32_t front, uint32_t vm)
{
    uint32_t x2 = front & 255u, x1 = front >> 8;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t sym = (w[k >> 2] >> (8 * (k & 3))) & 255u, ctx = 31u * x2 + x1;       // (ctx: its low 8 bits)
        if (!CHECKED || ((vm >> k) & 1u) != 0) atomicAdd(&s_t[ch16_cell(ctx, sym)], ch16_one(ctx, sym));
        x2 = x1; x1 = sym;
    }
}

__global__ __launch_bounds__(CH_THREADS) void k_ch_probe16(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                           const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                           unsigned long long *__restrict__ stats)
{
    __shared__ uint4 s_t4[256 * CH16_ROW / 4];
    __shared__ uint32_t s_c[256];
    __shared__ unsigned long long s_sum[3];
    uint32_t *s_t = reinterpret_cast<uint32_t *>(s_t4);
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long l64 = data_len[b];
    uint32_t L = l64 > max_len ? max_len : (uint32_t)l64;
    L = L > CH16_MAX_LEN ? CH16_MAX_LEN : L;                   // (the launcher keeps max_len within it: a cell must fit its half)
    unsigned long long *out = stats + (size_t)CHOOSE_STATS * b;
    if (L < 3) {                                               // no position: nothing can collide
        if (tid < CHOOSE_STATS) out[tid] = 0ull;
        return;
    }
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    if (tid < 256) s_c[tid] = 0;
    if (tid < 3) s_sum[tid] = 0;
    for (uint32_t i = tid; i < 256 * CH16_ROW / 4; i += CH_THREADS) s_t4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for (uint32_t o0 = wave * CH_STEP; o0 < L; o0 += CH_WAVES * CH_STEP) {         // (wave-uniform)
        const uint32_t o = o0 + 16 * lane, n = o < L ? min(16u, L - o) : 0u;
        uint32_t w[4] = {0, 0, 0, 0};
        if (al && n == 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(in + o);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) if (k < n) w[k >> 2] |= (uint32_t)in[o + k] << (8 * (k & 3));
        }
        uint32_t front = wave_prev(w[3]) >> 16;
        if (lane == 0) front = o0 ? (uint32_t)in[o0 - 2] | (uint32_t)in[o0 - 1] << 8 : 0u;
        // the shortcuts of k_ch_probe: a lane of one value adds 16 with one atomic, a wave of such lanes of one value 1024
        const uint32_t b0 = w[0] & 255u, rep = b0 * 0x01010101u;
        const bool uni = n == 16 && o0 != 0 && w[0] == rep && w[1] == rep && w[2] == rep && w[3] == rep && front == (rep & 0xFFFFu);
        const uint32_t uctx = (32u * b0) & 255u, ucell = ch16_cell(uctx, b0), uone = ch16_one(uctx, b0);
        if (__ballot(!uni) == 0 && __ballot(b0 != (uint32_t)__builtin_amdgcn_readfirstlane((int)b0)) == 0) {
            if (lane == 0) atomicAdd(&s_t[ucell], CH_STEP * uone);
            continue;
        }
        if (uni) {
            atomicAdd(&s_t[ucell], 16u * uone);
        } else if (o0 != 0 && o0 + CH_STEP <= L) {                   // (wave-uniform: every lane has 16 bytes behind two more)
            ch16_steps<false>(s_t, w, front, 0u);
        } else if (n) {
            const uint32_t lo = o >= 2 ? 0u : 2u - o;
            ch16_steps<true>(s_t, w, front, ((1u << n) - 1u) & ~((1u << lo) - 1u));
        }
    }
    __syncthreads();
    // every row's sum and its cells' N (N - 1), a wave per row; the column sums, four lanes per column over 64 rows each
    unsigned long long s2 = 0, sr = 0;
    for (uint32_t r = wave; r < 256; r += CH_WAVES) {
        uint32_t rs = 0;
#pragma unroll
        for (uint32_t k = 0; k < CH16_ROW / 64; k++) {
            const uint32_t v = s_t[r * CH16_ROW + 64 * k + lane], v0 = v & 0xFFFFu, v1 = v >> 16;
            rs += v0 + v1;
            s2 += (unsigned long long)(v0 * (v0 - 1u)) + (unsigned long long)(v1 * (v1 - 1u));    // (below 2^32 each; v = 0: 0 times anything)
        }
        rs = wave_sum(rs);
        if (lane == 0) sr += (unsigned long long)rs * (rs - 1u);
    }
    {
        const uint32_t col = tid & 255u, r0 = (tid >> 8) * 64u;
        uint32_t c = 0;
        for (uint32_t r = r0; r < r0 + 64u; r++) {
            const uint32_t p = (col + r) & 255u, v = s_t[r * CH16_ROW + (p & 127u)];
            c += p & 128u ? v >> 16 : v & 0xFFFFu;
        }
        atomicAdd(&s_c[col], c);
    }
    __syncthreads();
    unsigned long long sc = 0;
    if (tid < 256) { const uint32_t c = s_c[tid]; sc = (unsigned long long)c * (c - 1u); }
    s2 = ch_wave_sum(s2); sr = ch_wave_sum(sr); sc = ch_wave_sum(sc);
    if (lane == 0) { atomicAdd(&s_sum[0], s2); atomicAdd(&s_sum[1], sr); atomicAdd(&s_sum[2], sc); }
    __syncthreads();
    if (tid < CHOOSE_STATS) out[tid] = tid < 3 ? s_sum[tid] : (unsigned long long)(L - 2);
}

hipError_t bigram_probe_segments(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                                 uint32_t count, uint32_t max_len, unsigned long long *stats)
{
    if (count == 0) return hipSuccess;
    if (max_len <= CH16_MAX_LEN) hipLaunchKernelGGL(k_ch_probe16, dim3(count), dim3(CH_THREADS), 0, st, data, data_off, data_len, max_len, stats);
    else hipLaunchKernelGGL(k_ch_probe, dim3(count), dim3(CH_THREADS), 0, st, data, data_off, data_len, max_len, stats);
    return hipGetLastError();
}

} // namespace glc
