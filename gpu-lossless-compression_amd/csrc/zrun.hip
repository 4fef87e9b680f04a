// zrun.hip -- the zero-run mode of the container's BWT codec (record kind 4, format version 6): the two
// bandwidth-bound passes between the MTF and the batched order-0 kernels of hd_batch.hip.  gfx950 / wave64.
// A segment x[0, n) (the MTF bytes of a block) is cut into tiles of 256 bytes.  Position i is a RUN START when x[i] = 0 and
// (i % 256 = 0 or x[i - 1] != 0); A is x at the positions that are non-zero or run starts, B has one byte per run start: the
// zeros from there to the next non-zero byte, tile edge or n, minus one.  No run crosses a tile, so a tile needs nothing of
// another but the number of bytes the tiles in front of it put into A and B.
//   k_zr_split  one workgroup of 16 waves per segment, 16 KiB a pass: a wave takes four tiles, a lane the bytes 64 j + lane of
//               each (j = 0 .. 3), so a tile's zero mask is four ballots, in position order.  Starts and kept positions are
//               mask arithmetic on wave-uniform words, a start's length a count of trailing ones from its bit, ranks inside
//               the tile popcounts below the bit.  The waves' counts meet in LDS (one barrier a pass, two buffers), the
//               segment's running totals are carried in registers: no waiting between workgroups, no atomics, and the
//               outputs do not depend on scheduling
//   k_zr_join   one workgroup per segment: the output is zeroed, then A is walked 4 KiB a pass, four bytes a lane -- a scan
//               of the zeros gives every zero its entry of B, a scan of (A[k] ? 1 : B[z] + 1) every byte its output position,
//               both carried from pass to pass -- and only the non-zero bytes are scattered.  Tolerant: a zero beyond B's end
//               is a run of one, a position at or beyond n is not written, nothing is read outside A and B
// Byte-granular loads and stores throughout (a wave's are 64 consecutive bytes): any length up to 2^20, any alignment.
// The container's own steps (segments, nz and record sizes, nz and pairs into the records, B's counts out of a record) are the
// small kernels at the end.
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t ZR_THREADS = 1024, ZR_WAVES = ZR_THREADS / WAVE, ZR_TPW = 4;
constexpr uint32_t ZR_PASS = ZR_WAVES * ZR_TPW * ZR_TILE;          // bytes of x a workgroup takes per pass of the split
constexpr uint32_t ZJ_PER = 4, ZJ_PASS = ZR_THREADS * ZJ_PER;      // bytes of A a lane / a workgroup takes per pass of the join

__device__ __forceinline__ uint32_t zr_clamp(unsigned long long l, uint32_t max_len) { return l > max_len ? max_len : (uint32_t)l; }
__device__ __forceinline__ uint8_t *zr_ptr(const uint8_t *base, unsigned long long off)
{
    return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(base) + off);
}

// starts and kept positions of word j of a tile from its zero masks z[0 .. 3] and the word's valid mask
__device__ __forceinline__ unsigned long long zr_starts(const unsigned long long z[4], uint32_t j)
{
    return z[j] & ~((z[j] << 1) | (j ? z[j - 1] >> 63 : 0ull));
}

__global__ __launch_bounds__(ZR_THREADS) void k_zr_split(ZrSegs g)
{
    __shared__ uint32_t s_cnt[2][ZR_WAVES];                        // a wave's bytes of A (low half) and of B (high half) in this pass
    const uint32_t i = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g.skip && g.skip[i]) return;
    const uint32_t L = zr_clamp(g.x_len[i], g.max_len);
    const uint8_t *x = zr_ptr(g.x, g.x_off[i]);
    uint8_t *A = zr_ptr(g.a, g.a_off[i]), *B = zr_ptr(g.b, g.b_off[i]);
    uint32_t doneA = 0, doneB = 0;
    for (uint32_t p0 = 0, par = 0; p0 < L; p0 += ZR_PASS, par ^= 1u) {
        const uint32_t w0 = p0 + wave * ZR_TPW * ZR_TILE;          // (L <= 2^20: no wrap)
        uint8_t v[ZR_TPW][4];
        unsigned long long Z[ZR_TPW][4];
        uint32_t ca = 0, cb = 0;
#pragma unroll
        for (uint32_t t = 0; t < ZR_TPW; t++) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t pos = w0 + t * ZR_TILE + 64 * j + lane;
                v[t][j] = pos < L ? x[pos] : (uint8_t)1;
                Z[t][j] = __ballot((int)(v[t][j] == 0));
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t first = w0 + t * ZR_TILE + 64 * j;
                const unsigned long long valid = first >= L ? 0ull : L - first >= 64 ? ~0ull : (1ull << (L - first)) - 1ull;
                const unsigned long long S = zr_starts(Z[t], j);
                ca += __popcll(valid & (~Z[t][j] | S));
                cb += __popcll(S);
            }
        }
        if (lane == 0) s_cnt[par][wave] = ca | (cb << 16);         // (at most 1024 each; 16384 over the workgroup)
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < ZR_WAVES; w++) { const uint32_t c = s_cnt[par][w]; before += w < wave ? c : 0u; all += c; }
        uint32_t ra = doneA + (before & 0xFFFFu), rb = doneB + (before >> 16);
        doneA += all & 0xFFFFu; doneB += all >> 16;
#pragma unroll
        for (uint32_t t = 0; t < ZR_TPW; t++) {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const uint32_t first = w0 + t * ZR_TILE + 64 * j;
                const unsigned long long valid = first >= L ? 0ull : L - first >= 64 ? ~0ull : (1ull << (L - first)) - 1ull;
                const unsigned long long S = zr_starts(Z[t], j), K = valid & (~Z[t][j] | S);
                if ((K >> lane) & 1ull) A[ra + mbcnt(K)] = v[t][j];
                if ((S >> lane) & 1ull) {
                    // the ones from this bit on, through the following words of the tile while a word ends in ones
                    uint32_t r = 0;
                    bool open = true;
#pragma unroll
                    for (uint32_t jj = j; jj < 4; jj++) {
                        const unsigned long long nz = ~(jj == j ? Z[t][jj] >> lane : Z[t][jj]);   // (the shift brings zeros in: a one above)
                        const uint32_t width = jj == j ? 64u - lane : 64u;
                        const uint32_t c = nz ? (uint32_t)__builtin_ctzll(nz) : 64u;
                        r += open ? c : 0u;
                        open = open && c == width;
                    }
                    B[rb + mbcnt(S)] = (uint8_t)(r - 1u);
                }
                ra += __popcll(K); rb += __popcll(S);
            }
        }
    }
    if (threadIdx.x == 0) { g.a_len[i] = doneA; g.b_len[i] = doneB; }
}

// exclusive prefix of x over the workgroup and the workgroup's sum; s_w (ZR_WAVES words) is free on entry and on return
// is read by nobody after the caller's next barrier
__device__ __forceinline__ uint32_t zr_scan(uint32_t x, uint32_t *s_w, uint32_t *all)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t inc = wave_incl_add(x);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < ZR_WAVES; w++) { const uint32_t c = s_w[w]; before += w < wave ? c : 0u; tot += c; }
    *all = tot;
    return before + inc - x;
}

__global__ __launch_bounds__(ZR_THREADS) void k_zr_join(ZrSegs g)
{
    __shared__ uint32_t s_z[ZR_WAVES], s_o[ZR_WAVES];
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    if (g.skip && g.skip[i]) return;
    const uint32_t n = zr_clamp(g.x_len[i], g.max_len), nA = zr_clamp(g.a_len[i], g.max_len), nB = zr_clamp(g.b_len[i], g.max_len);
    uint8_t *out = zr_ptr(g.x, g.x_off[i]);
    const uint8_t *A = zr_ptr(g.a, g.a_off[i]), *B = zr_ptr(g.b, g.b_off[i]);
    {   // zeros everywhere: bytes up to the first 16-byte boundary, granules, the bytes behind the last one
        const uint32_t head = min(n, (uint32_t)((16u - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u)), gran = (n - head) / 16;
        if (tid < head) out[tid] = 0;
        uint4 *q = reinterpret_cast<uint4 *>(out + head);
        for (uint32_t k = tid; k < gran; k += ZR_THREADS) q[k] = make_uint4(0, 0, 0, 0);
        const uint32_t tail0 = head + 16 * gran;
        if (tid < n - tail0) out[tail0 + tid] = 0;
    }
    __syncthreads();                                               // (the scatter below overwrites what other lanes zeroed)
    uint32_t doneZ = 0, doneO = 0;                                 // zeros of A and output bytes in front of this pass
    for (uint32_t k0 = 0; k0 < nA; k0 += ZJ_PASS) {
        const uint32_t k = k0 + ZJ_PER * tid;
        uint8_t a[ZJ_PER];
        uint32_t zc = 0;
#pragma unroll
        for (uint32_t q = 0; q < ZJ_PER; q++) {
            a[q] = k + q < nA ? A[k + q] : (uint8_t)1;
            zc += a[q] == 0 ? 1u : 0u;
        }
        uint32_t allz, allo;
        uint32_t z = doneZ + zr_scan(zc, s_z, &allz);
        uint32_t len[ZJ_PER], tot = 0;
#pragma unroll
        for (uint32_t q = 0; q < ZJ_PER; q++) {
            len[q] = k + q < nA ? 1u : 0u;
            if (a[q] == 0) { len[q] = z < nB ? (uint32_t)B[z] + 1u : 1u; z++; }
            tot += len[q];
        }
        uint32_t pos = doneO + zr_scan(tot, s_o, &allo);           // (at most 2^20 * 256: no wrap)
#pragma unroll
        for (uint32_t q = 0; q < ZJ_PER; q++) {
            if (a[q] != 0 && k + q < nA && pos < n) out[pos] = a[q];
            pos += len[q];
        }
        doneZ += allz; doneO += allo;
    }
}

hipError_t zrun_split(hipStream_t st, const ZrSegs &g)
{
    if (g.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_zr_split, dim3(g.count), dim3(ZR_THREADS), 0, st, g);
    return hipGetLastError();
}

hipError_t zrun_join(hipStream_t st, const ZrSegs &g)
{
    if (g.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_zr_join, dim3(g.count), dim3(ZR_THREADS), 0, st, g);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the container encoder's steps around them (container_api.cpp, Encoder::frame_runs)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_zr_segs(CtEncRuns r, const uint8_t *mtf, unsigned long long mtf_stride, uint32_t nb, uint32_t blk_len)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    r.x_off[b] = (unsigned long long)(uintptr_t)mtf + b * mtf_stride;
    r.x_len[b] = blk_len;
    r.seg_off[b] = (unsigned long long)(uintptr_t)r.a + (unsigned long long)b * r.stride;
    r.seg_off[nb + b] = (unsigned long long)(uintptr_t)r.b + (unsigned long long)b * r.stride;
}

__global__ __launch_bounds__(256) void k_zr_empty(CtEncRuns r, uint32_t nb)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) r.skip_b[b] = r.seg_len[nb + b] == 0 ? 1u : 0u;
}

// ct_enc_kind with the runs mode on (one workgroup per block): nz from B's counts; the record is nz, the pairs, the stream of
// A and, when B is not empty, the stream of B; raw under the record rule, and no other kind
__global__ __launch_bounds__(256) void k_zr_kind(CtEncFrame f, CtEncRuns r, uint32_t nb, uint32_t blk_len, unsigned long long table_bytes,
                                                 const CtEncState *state)
{
    __shared__ uint32_t s_tmp[256 / WAVE + 1];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned long long nB = r.seg_len[nb + b];
    const uint32_t c = nB ? r.hist_b[(size_t)b * 256 + tid] : 0u;
    uint32_t nz = 0;
    (void)block_excl_add<256>(c ? 1u : 0u, s_tmp, &nz);
    if (tid) return;
    const unsigned long long words = 1ull + nz + r.nun[b] + (nB ? r.nun[nb + b] : 0ull);
    const bool raw = ct_put_record(f, b, CT_KIND_RUNS, words, blk_len, table_bytes, state);
    f.only[b] = raw ? 1u : 0u;
    r.nz[b] = nz;
    r.skip_enc[b] = raw ? 1u : 0u;
    r.skip_enc[nb + b] = raw || nB == 0 ? 1u : 0u;
}

// behind the payload offsets: nz and the pairs (v << 24) | count, v ascending, into the kind-4 records that end inside the
// capacity, and where the two streams of every block start
__global__ __launch_bounds__(256) void k_zr_place(CtEncFrame f, CtEncRuns r, uint32_t nb, uint32_t *out, unsigned long long cap_words)
{
    __shared__ uint32_t s_tmp[256 / WAVE + 1];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t nz = r.nz[b];
    const uint32_t c = r.seg_len[nb + b] ? r.hist_b[(size_t)b * 256 + tid] : 0u;
    const uint32_t rank = block_excl_add<256>(c ? 1u : 0u, s_tmp);
    const unsigned long long o = f.boff[b];
    if (tid == 0) { r.unit_off[b] = o + 1 + nz; r.unit_off[nb + b] = o + 1 + nz + r.nun[b]; }
    if (f.kind[b] != CT_KIND_RUNS || f.boff[b + 1] > cap_words) return;
    if (tid == 0) out[o] = nz;
    if (c) out[o + 1 + rank] = (tid << 24) | c;                    // (c <= 2^20)
}

hipError_t ct_enc_runs_segs(hipStream_t st, const CtEncRuns &r, const uint8_t *mtf, size_t mtf_stride, uint32_t nb, uint32_t blk_len)
{
    hipLaunchKernelGGL(k_zr_segs, dim3((nb + 255) / 256), dim3(256), 0, st, r, mtf, (unsigned long long)mtf_stride, nb, blk_len);
    return hipGetLastError();
}

hipError_t ct_enc_runs_empty(hipStream_t st, const CtEncRuns &r, uint32_t nb)
{
    hipLaunchKernelGGL(k_zr_empty, dim3((nb + 255) / 256), dim3(256), 0, st, r, nb);
    return hipGetLastError();
}

hipError_t ct_enc_runs_kind(hipStream_t st, const CtEncFrame &f, const CtEncRuns &r, uint32_t nb, uint32_t blk_len, const CtEncState *state)
{
    const CtTables T = ct_tables(nb, blk_len);
    hipLaunchKernelGGL(k_zr_kind, dim3(nb), dim3(256), 0, st, f, r, nb, blk_len, 4 * T.words, state);
    return hipGetLastError();
}

hipError_t ct_enc_runs_place(hipStream_t st, const CtEncFrame &f, const CtEncRuns &r, uint32_t nb, uint32_t *out, unsigned long long cap_words)
{
    hipLaunchKernelGGL(k_zr_place, dim3(nb), dim3(256), 0, st, f, r, nb, out, cap_words);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the decoder's step in front of the verdict: B's counts out of the unverified record of every kind-4 block (one workgroup
// each).  Every read is clamped to the record, which is clamped to the payload; counts a valid record cannot hold (0, or more
// than blk_len) and pairs out of order leave all zeros and no table, and the verdict refuses the block
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_zr_dec_hist(const uint8_t *frame, uint32_t nb, uint32_t blk_len, unsigned long long P, CtDecHuff0 h0)
{
    __shared__ uint32_t s_bad;
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *W = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR);
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(W + T.pay_off);
    const uint32_t *pay = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words);
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned long long lo = po[b], hi = po[b + 1];
    bool ok = W[T.kind + b] == CT_KIND_RUNS && lo <= hi && hi <= P && hi - lo >= 1;
    const uint32_t nz = ok ? pay[lo] : 0u;
    ok = ok && nz <= 256 && hi - lo >= 1ull + nz;
    if (tid == 0) s_bad = 0;
    h0.hist_b[(size_t)b * 256 + tid] = 0;
    __syncthreads();
    uint32_t v = 0, c = 0;
    if (ok && tid < nz) {
        const uint32_t w = pay[lo + 1 + tid];
        v = w >> 24; c = w & 0xFFFFFFu;
        if (c == 0 || c > blk_len || (tid > 0 && (pay[lo + tid] >> 24) >= v)) s_bad = 1;
    }
    __syncthreads();
    ok = ok && s_bad == 0;
    if (ok && tid < nz) h0.hist_b[(size_t)b * 256 + v] = c;        // (ascending: every v once)
    if (tid == 0) h0.skip_tb[b] = ok && nz ? 0u : 1u;
}

hipError_t ct_dec_runs_hist(hipStream_t st, const uint8_t *frame, uint32_t nb, uint32_t blk_len, unsigned long long payload_words,
                            const CtDecHuff0 &h0)
{
    hipLaunchKernelGGL(k_zr_dec_hist, dim3(nb), dim3(256), 0, st, frame, nb, blk_len, payload_words, h0);
    return hipGetLastError();
}

} // namespace glc
