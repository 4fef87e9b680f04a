// filter_probe.hip -- the filter probe (INTEGRATION.md 4b "filter: auto"; the rows and the costs are defined in filter_rule.h):
// which byte-plane filter a segment wants, from one read of it.  gfx950 / wave64.
//   k_fp_probe   the 22 histograms of a segment.  A workgroup of 256 lanes owns a span of the segment, a multiple of 16 KiB, so
//                that every delta restart of every element size (2048 elements: 4, 8 and 16 KiB) that falls into the span is
//                found from the offset alone and nothing before the span is needed.  A wave takes 1 KiB a pass and a lane 16
//                bytes of it, 8 bytes at a time: eight counts for the A rows, and four 16-bit, two 32-bit and one 64-bit delta
//                with eight counts each.  The element before a lane's first comes with an overlapping 8-byte load (a hit in
//                the line the neighbouring lane reads); at a restart there is none.  16-byte loads where the segment's address
//                allows, a byte path where it does not.
//                Counts go to LDS counters: 22 rows of 257 words, FP_COPIES copies picked by the lane's low bits.  Two copies
//                are 45,232 bytes: three workgroups, twelve waves, a CU (160 KiB).  Zeros, a constant or a regular-step series
//                would put all 64 lanes on one counter sixteen times a group, so each of the four groups (A, D_2, D_4, D_8)
//                first asks with one ballot whether every lane holds the first lane's sixteen bytes; if so sixteen lanes add
//                64 each, one per byte.  Typed data does the same to some of the sixteen byte positions -- the high bytes of an
//                element or of its delta -- so otherwise the OR over the wave of (bytes ^ first lane's) says which positions
//                hold one value, and those cost one add of 64 as well.  A span's counters are added to the segment's rows with
//                global atomics, zeros skipped.
//   k_fp_cost    the seven costs of a segment from its rows: one wave per plane (29 planes, eight waves a workgroup), a lane
//                four symbols, AUTO_COST from constant memory; lane s of the first wave then sums candidate s.
// Any segment length up to 2^31, any byte alignment; only the first L - L % 8 bytes are counted.
#include "container_internal.h"
#include "filter_rule.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t FP_THREADS = 256, FP_PASS = 1024, FP_TILE = 16384;
constexpr uint32_t FP_COPIES = 2, FP_PITCH = 257, FP_COPY_WORDS = FILTER_ROWS * FP_PITCH;
constexpr uint32_t FP_MIN_SPAN = 4 * FP_TILE, FP_MAX_SPANS = 1024;     // a span amortises its 5632 global adds over >= 64 KiB

__device__ __forceinline__ uint32_t fp_len(const unsigned long long *len, uint32_t i, uint32_t max_len)
{
    const unsigned long long l = len[i];
    return (l > max_len ? max_len : (uint32_t)l) & ~7u;
}

// eight bytes at p as two dwords
__device__ __forceinline__ uint2 fp_load8(const uint8_t *p, bool aligned)
{
    if (aligned) return *reinterpret_cast<const uint2 *>(p);
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint2(w[0], w[1]);
}

// the 16-bit deltas of the two halves of w; prev = the dword before it (its high half is the element before)
__device__ __forceinline__ uint32_t fp_delta16(uint32_t w, uint32_t prev)
{
    const uint32_t lo = (w & 0xFFFFu) - (prev >> 16), hi = (w >> 16) - (w & 0xFFFFu);
    return (lo & 0xFFFFu) | (hi << 16);
}

// the OR of x over the wave, in every lane's scalar: wave_incl_add's DPP steps with | for +
__device__ __forceinline__ uint32_t fp_wave_or(uint32_t x)
{
    x |= GLC_DPP(x, 0x111, 0xf);
    x |= GLC_DPP(x, 0x112, 0xf);
    x |= GLC_DPP(x, 0x114, 0xf);
    x |= GLC_DPP(x, 0x118, 0xf);
    x |= GLC_DPP(x, 0x142, 0xa);
    x |= GLC_DPP(x, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

__global__ __launch_bounds__(FP_THREADS) void k_fp_probe(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                         const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                         uint32_t span, uint32_t *__restrict__ planes)
{
    __shared__ uint32_t s_h[FP_COPIES * FP_COPY_WORDS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t P = fp_len(data_len, b, max_len);
    const unsigned long long s0 = (unsigned long long)blockIdx.y * span;
    if (s0 >= P) return;
    const uint32_t t0 = (uint32_t)s0, t1 = P - t0 > span ? t0 + span : P;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    for (uint32_t i = tid; i < FP_COPIES * FP_COPY_WORDS; i += FP_THREADS) s_h[i] = 0;
    __syncthreads();
    uint32_t *H = s_h + (tid & (FP_COPIES - 1)) * FP_COPY_WORDS;
    // one group of a pass: this lane's n (0, 8 or 16) bytes d of histograms row0 .. row0 + e - 1, byte k to row row0 + k % e
    auto group = [&](const uint32_t d[4], uint32_t n, bool whole, uint32_t row0, uint32_t e) {
        if (whole) {                                           // every lane holds 16 bytes: are they the first lane's?
            uint32_t f[4];
            bool same = true;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                f[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)d[k]);
                same = same && d[k] == f[k];
            }
            if (__ballot(!same) == 0) {
                if (lane < 16) {
                    const uint32_t w = lane < 4 ? f[0] : lane < 8 ? f[1] : lane < 12 ? f[2] : f[3];
                    atomicAdd(&H[(row0 + (lane & (e - 1))) * FP_PITCH + ((w >> (8 * (lane & 3))) & 0xFFu)], 64u);
                }
                return;
            }
            // typed data: the high bytes of an element, or of its delta, are one value in every lane while the low ones vary.
            // The OR over the wave of d ^ first says which of the sixteen byte positions do; those cost one add of 64.
            // A deliberate trade: the 24 DPP steps a group cost the inputs that never take the shortcut a tenth to a fifth
            // (float32 587 -> 510 GB/s, noise 663 -> 518) and take int64 timestamps from 231 to 506 (profiles/filter_auto.md)
            uint32_t var[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) var[k] = fp_wave_or(d[k] ^ f[k]);
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                uint32_t *row = H + (row0 + (k & (e - 1))) * FP_PITCH;
                if ((var[k >> 2] >> (8 * (k & 3))) & 0xFFu) atomicAdd(&row[(d[k >> 2] >> (8 * (k & 3))) & 0xFFu], 1u);
                else if (lane == 0) atomicAdd(&row[(f[k >> 2] >> (8 * (k & 3))) & 0xFFu], 64u);
            }
            return;
        }
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (k < n) atomicAdd(&H[(row0 + (k & (e - 1))) * FP_PITCH + ((d[k >> 2] >> (8 * (k & 3))) & 0xFFu)], 1u);
    };
    for (uint32_t o0 = t0 + wave * FP_PASS; o0 < t1; o0 += 4 * FP_PASS) {
        const uint32_t o = o0 + 16 * lane;
        const uint32_t n = o < t1 ? min(16u, t1 - o) : 0u;     // 0, 8 or 16: t1 and o are multiples of 8
        const bool whole = t1 - o0 >= FP_PASS;                 // wave-uniform
        uint32_t v[4] = {0, 0, 0, 0}, p[2] = {0, 0};
        if (n == 16 && al) {
            const uint4 q = *reinterpret_cast<const uint4 *>(in + o);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else if (n) {
            const uint2 q = fp_load8(in + o, al);
            v[0] = q.x; v[1] = q.y;
            if (n == 16) { const uint2 r = fp_load8(in + o + 8, al); v[2] = r.x; v[3] = r.y; }
        }
        if (n && (o & (FP_TILE - 1))) {                        // (at a multiple of 16 KiB every element size restarts)
            const uint2 q = fp_load8(in + o - 8, al);
            p[0] = q.x; p[1] = q.y;
        }
        // the element before the lane's first, 0 where the first is a restart: then its delta is the element itself
        const uint32_t p2 = (o & (2 * FILTER_RUN - 1)) ? p[1] : 0u, p4 = (o & (4 * FILTER_RUN - 1)) ? p[1] : 0u;
        const bool r8 = (o & (8 * FILTER_RUN - 1)) == 0;
        const unsigned long long p8 = r8 ? 0ull : ((unsigned long long)p[1] << 32) | p[0];
        const unsigned long long x0 = ((unsigned long long)v[1] << 32) | v[0], x1 = ((unsigned long long)v[3] << 32) | v[2];
        const unsigned long long e0 = x0 - p8, e1 = x1 - x0;
        const uint32_t d2[4] = {fp_delta16(v[0], p2), fp_delta16(v[1], v[0]), fp_delta16(v[2], v[1]), fp_delta16(v[3], v[2])};
        const uint32_t d4[4] = {v[0] - p4, v[1] - v[0], v[2] - v[1], v[3] - v[2]};
        const uint32_t d8[4] = {(uint32_t)e0, (uint32_t)(e0 >> 32), (uint32_t)e1, (uint32_t)(e1 >> 32)};
        group(v, n, whole, 0, 8);
        group(d2, n, whole, filter_delta_row(2), 2);
        group(d4, n, whole, filter_delta_row(4), 4);
        group(d8, n, whole, filter_delta_row(8), 8);
    }
    __syncthreads();
    uint32_t *out = planes + (size_t)b * FILTER_ROWS * 256;
    for (uint32_t i = tid; i < FILTER_ROWS * 256; i += FP_THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t k = 0; k < FP_COPIES; k++) c += s_h[k * FP_COPY_WORDS + (i >> 8) * FP_PITCH + (i & 255u)];
        if (c) atomicAdd(&out[i], c);
    }
}

__device__ __forceinline__ unsigned long long fp_wave_sum64(unsigned long long x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += (unsigned long long)__shfl_xor((long long)x, m, 64);
    return x;
}

constexpr uint32_t FP_COST_WAVES = 8;

__global__ __launch_bounds__(FP_COST_WAVES * 64) void k_fp_cost(const uint32_t *__restrict__ planes, uint32_t count,
                                                                unsigned long long *__restrict__ costs)
{
    __shared__ unsigned long long s_plane[FILTER_PLANES];
    const uint32_t b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (b >= count) return;
    const uint32_t *rows = planes + (size_t)b * FILTER_ROWS * 256;
    for (uint32_t pl = wave; pl < FILTER_PLANES; pl += FP_COST_WAVES) {
        const FilterPlane f = filter_plane(pl);
        uint32_t h[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < f.count; k++) {
            const uint4 q = *reinterpret_cast<const uint4 *>(rows + (size_t)(f.first + k * f.step) * 256 + 4 * lane);
            h[0] += q.x; h[1] += q.y; h[2] += q.z; h[3] += q.w;
        }
        const unsigned long long N = fp_wave_sum64((unsigned long long)h[0] + h[1] + h[2] + h[3]);
        unsigned long long c = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) c += filter_symbol_cost(h[k], N);
        c = fp_wave_sum64(c);
        if (lane == 0) s_plane[pl] = c;
    }
    __syncthreads();
    if (threadIdx.x < FILTER_CANDS) {
        unsigned long long c = 0;
        for (uint32_t pl = filter_first_plane(threadIdx.x); pl < filter_first_plane(threadIdx.x + 1); pl++) c += s_plane[pl];
        costs[(size_t)b * FILTER_CANDS + threadIdx.x] = c;
    }
}

hipError_t filter_probe_segments(hipStream_t st, const uint8_t *data, const unsigned long long *data_off,
                                 const unsigned long long *data_len, uint32_t count, uint32_t max_len, uint32_t *planes,
                                 unsigned long long *costs)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(planes, 0, (size_t)count * FILTER_ROWS * 1024, st);
    if (e != hipSuccess) return e;
    if (max_len >= 8) {
        // spans: multiples of 16 KiB, at least FP_MIN_SPAN, at most FP_MAX_SPANS of them a segment
        const unsigned long long tiles = ((unsigned long long)max_len + FP_TILE - 1) / FP_TILE;
        unsigned long long per = (tiles + FP_MAX_SPANS - 1) / FP_MAX_SPANS;
        if (per < FP_MIN_SPAN / FP_TILE) per = FP_MIN_SPAN / FP_TILE;
        const uint32_t span = (uint32_t)(per * FP_TILE), spans = (uint32_t)((tiles + per - 1) / per);
        hipLaunchKernelGGL(k_fp_probe, dim3(count, spans), dim3(FP_THREADS), 0, st, data, data_off, data_len, max_len, span, planes);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_fp_cost, dim3(count), dim3(FP_COST_WAVES * 64), 0, st, planes, count, costs);
    return hipGetLastError();
}

} // namespace glc
