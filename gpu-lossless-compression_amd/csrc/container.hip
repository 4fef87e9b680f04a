// container.hip -- kernels of the BWT container: CRC-32 of ragged device segments, and the encode /
// decode side of a frame (record kinds, raw records, tables, checks), all on the device; the host side is container_api.cpp.
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

__device__ const CrcTables g_crc = crc_make_tables();
__device__ const CrcX2n g_x2n = crc_make_x2n();

__device__ __forceinline__ uint32_t shift_bytes(uint32_t r, unsigned long long n) { return crc_multmodp(crc_x8n(n, g_x2n), r); }

// ---------------------------------------------------------------------------
// CRC-32 of segments.  A segment [p, p + L) splits into a HEAD of whole 16-byte granules ending at E16 = (p + L) & ~15 and a
// tail of < 16 bytes.  The head is read as rows of 64 granules (1 KiB, one 16-byte load per lane) laid out from a virtual
// start E16 - rows * 1024: the bytes before p in that range count as zeros, which a raw CRC ignores, so every row is whole
// and every shift is by a fixed amount.  Lane l folds its column of granules (acc = acc * x^8192 ^ crc16(granule): 4 + 16
// table reads from LDS); a wave's 64 columns combine in a 6-level tree (x^(128 * 2^k)); a wave's share of a segment adds its
// raw CRC, shifted by the bytes that follow it, into the segment's word with atomicXor -- XOR is the addition of GF(2)
// polynomials, so the order the waves finish in does not matter.  Rows are dealt out as tiles of 16 rows, contiguous
// ranges of the tile list (all segments together) per wave.
// ---------------------------------------------------------------------------
struct SegGeom { unsigned long long p, end, e16; uint32_t nrows; };
__device__ __forceinline__ SegGeom seg_geom(const uint8_t *base, const unsigned long long *off, const unsigned long long *len, uint32_t s)
{
    SegGeom g;
    g.p = (unsigned long long)(uintptr_t)base + off[s];
    g.end = g.p + len[s];
    g.e16 = g.end & ~15ull;
    const unsigned long long g0 = g.p & ~15ull;
    g.nrows = g.e16 > g.p ? (uint32_t)(((g.e16 - g0) / 16 + 63) / 64) : 0u;
    return g;
}

__global__ __launch_bounds__(1024) void k_crc_scan(const uint8_t *base, const unsigned long long *__restrict__ off,
                                                   const unsigned long long *__restrict__ len, uint32_t count,
                                                   uint32_t *__restrict__ tile_start, uint32_t *__restrict__ crc)
{
    __shared__ uint32_t s_tmp[20];
    __shared__ uint32_t s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (uint32_t c = 0; c < count; c += 1024) {
        const uint32_t i = c + threadIdx.x;
        uint32_t nt = 0;
        if (i < count) {
            nt = (seg_geom(base, off, len, i).nrows + CRC_TILE_ROWS - 1) / CRC_TILE_ROWS;
            crc[i] = 0;
        }
        uint32_t tot = 0;
        const uint32_t ex = block_excl_add<1024>(nt, s_tmp, &tot);
        const uint32_t run = s_run;
        if (i < count) tile_start[i] = run + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_run = run + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_start[count] = s_run;
}

constexpr uint32_t CRC_GRID = 1024;                            // persistent: 4 waves per workgroup, 4096 wave workers

__global__ __launch_bounds__(256) void k_crc_rows(const uint8_t *base, const unsigned long long *__restrict__ off,
                                                  const unsigned long long *__restrict__ len, uint32_t count,
                                                  const uint32_t *__restrict__ tile_start, uint32_t *__restrict__ crc)
{
    // slice tables in LDS: a lookup is a random ds_read_b32, 32 lanes per LDS cycle over 32 banks (a few-way conflict on
    // random bytes); 20 KiB leaves room for 8 workgroups per CU
    __shared__ uint32_t sT[16][256];
    __shared__ uint32_t sR[4][256];
    for (uint32_t i = threadIdx.x; i < 16 * 256; i += 256) sT[i >> 8][i & 255] = g_crc.t[i >> 8][i & 255];
    for (uint32_t i = threadIdx.x; i < 4 * 256; i += 256) sR[i >> 8][i & 255] = g_crc.row[i >> 8][i & 255];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long total = tile_start[count], W = (unsigned long long)gridDim.x * 4;
    const unsigned long long w = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned long long t0 = w * total / W, t1 = (w + 1) * total / W;
    if (t0 >= t1) return;
    uint32_t lo = 0, hi = count - 1;                           // last segment whose tiles start at or before t0
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (tile_start[mid] <= t0) lo = mid; else hi = mid - 1;
    }
    unsigned long long t = t0;
    for (uint32_t s = lo; t < t1 && s < count; s++) {
        const unsigned long long ts = tile_start[s], te = tile_start[s + 1];
        if (te <= t) continue;                                  // (no head)
        const unsigned long long tend = te < t1 ? te : t1;
        const SegGeom g = seg_geom(base, off, len, s);
        const unsigned long long a0 = g.e16 - (unsigned long long)g.nrows * CRC_ROW;
        const uint32_t r0 = (uint32_t)(t - ts) * CRC_TILE_ROWS;
        const uint32_t r1 = (uint32_t)min((unsigned long long)g.nrows, (tend - ts) * CRC_TILE_ROWS);
        uint32_t acc = 0;
        for (uint32_t r = r0; r < r1; r += CRC_TILE_ROWS) {
            uint4 q[CRC_TILE_ROWS];
#pragma unroll
            for (uint32_t j = 0; j < CRC_TILE_ROWS; j++) {
                const unsigned long long a = a0 + (unsigned long long)(r + j) * CRC_ROW + lane * 16;
                q[j] = make_uint4(0, 0, 0, 0);
                if (r + j < r1 && a + 16 > g.p) q[j] = *reinterpret_cast<const uint4 *>((uintptr_t)a);
                if (a < g.p && a + 16 > g.p) {                   // the granule p starts in: bytes before p are zeros
                    const uint32_t k = (uint32_t)(g.p - a);      // 1 .. 15
                    uint32_t *qq = reinterpret_cast<uint32_t *>(&q[j]);
#pragma unroll
                    for (uint32_t d = 0; d < 4; d++) {
                        const uint32_t b0 = 4 * d;
                        const uint32_t m = k <= b0 ? 0xFFFFFFFFu : (k >= b0 + 4 ? 0u : (0xFFFFFFFFu << (8 * (k - b0))));
                        qq[d] &= m;
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < CRC_TILE_ROWS; j++) {
                if (r + j >= r1) continue;
                const uint32_t x = q[j].x, y = q[j].y, z = q[j].z, u = q[j].w;
                const uint32_t sh = sR[0][acc & 255] ^ sR[1][(acc >> 8) & 255] ^ sR[2][(acc >> 16) & 255] ^ sR[3][acc >> 24];
                acc = sh ^ sT[15][x & 255] ^ sT[14][(x >> 8) & 255] ^ sT[13][(x >> 16) & 255] ^ sT[12][x >> 24]
                         ^ sT[11][y & 255] ^ sT[10][(y >> 8) & 255] ^ sT[9][(y >> 16) & 255] ^ sT[8][y >> 24]
                         ^ sT[7][z & 255] ^ sT[6][(z >> 8) & 255] ^ sT[5][(z >> 16) & 255] ^ sT[4][z >> 24]
                         ^ sT[3][u & 255] ^ sT[2][(u >> 8) & 255] ^ sT[1][(u >> 16) & 255] ^ sT[0][u >> 24];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 6; k++) {                      // lane l's column is followed by 16 (63 - l) bytes of its row
            const uint32_t o = (uint32_t)__shfl_down((int)acc, 1 << k, 64);
            acc = crc_multmodp(g_x2n.v[7 + k], acc) ^ o;        // x^(8 * 16 * 2^k)
        }
        if (lane == 0) atomicXor(&crc[s], shift_bytes(acc, (unsigned long long)(g.nrows - r1) * CRC_ROW));
        t = tend;
    }
}

__global__ __launch_bounds__(256) void k_crc_finish(const uint8_t *base, const unsigned long long *__restrict__ off,
                                                    const unsigned long long *__restrict__ len, uint32_t count,
                                                    uint32_t *__restrict__ crc)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= count) return;
    const SegGeom g = seg_geom(base, off, len, s);
    uint32_t r = crc[s];
    for (unsigned long long a = g.e16 > g.p ? g.e16 : g.p; a < g.end; a++)
        r = g_crc.t[0][(r ^ *reinterpret_cast<const uint8_t *>((uintptr_t)a)) & 255] ^ (r >> 8);
    crc[s] = r ^ shift_bytes(0xFFFFFFFFu, len[s]) ^ 0xFFFFFFFFu;
}

hipError_t crc32_segments(hipStream_t st, const uint8_t *base, const unsigned long long *d_off,
                          const unsigned long long *d_len, uint32_t count, uint32_t *d_crc)
{
    if (count == 0) return hipSuccess;
    uint32_t *ts = nullptr;
    hipError_t e = glc_dev_alloc_async((void **)&ts, ((size_t)count + 1) * 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_crc_scan, dim3(1), dim3(1024), 0, st, base, d_off, d_len, count, ts, d_crc);
    hipLaunchKernelGGL(k_crc_rows, dim3(CRC_GRID), dim3(256), 0, st, base, d_off, d_len, count, (const uint32_t *)ts, d_crc);
    hipLaunchKernelGGL(k_crc_finish, dim3((count + 255) / 256), dim3(256), 0, st, base, d_off, d_len, count, d_crc);
    e = hipGetLastError();
    const hipError_t e2 = hipFreeAsync(ts, st);
    return e != hipSuccess ? e : e2;
}

// The CRC of nb consecutive blocks of blk_len bytes from theirs: crc = XOR over b of shift(crc_b, (nb - 1 - b) blk_len) (the
// combine rule unrolled from the CRC of nothing, 0), one term per thread, summed into *acc with atomicXor
__global__ __launch_bounds__(256) void k_fold_terms(const uint32_t *__restrict__ crcs, uint32_t nb, uint32_t blk_len, uint32_t *acc)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) atomicXor(acc, shift_bytes(crcs[b], (unsigned long long)(nb - 1 - b) * blk_len));
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
struct CtHdrWords { uint32_t w[8]; };

__global__ void k_ct_header(uint8_t *out, unsigned long long cap, CtHdrWords h, CtEncState *state)
{
    if (threadIdx.x < 8 && cap >= CT_HDR) reinterpret_cast<uint32_t *>(out)[threadIdx.x] = h.w[threadIdx.x];
    if (threadIdx.x == 0) { state->cursor = CT_HDR; state->crc_all = 0; state->frames = 0; state->frame_acc = 0; }
}

// per block (one wave each): raw when a sub-block needs more than HUFF_MAX_WORDS words or under the record rule; the record's
// words go to f.size (what the payload offsets are scanned from) and the packer's mask to f.only
__global__ __launch_bounds__(256) void k_ct_kind(CtEncFrame f, uint32_t nb, uint32_t blk_len, unsigned long long table_bytes,
                                                 const CtEncState *state)
{
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nb) return;
    const uint32_t nsub = (blk_len + HUFF_BLOCK - 1) / HUFF_BLOCK;
    const uint32_t size = f.size[b];
    const uint32_t *eo = f.enc_off + (size_t)b * nsub;
    bool over = false;
    for (uint32_t s = lane; s < nsub; s += 64) {
        const uint32_t nx = s + 1 < nsub ? eo[s + 1] : size;
        over |= nx - eo[s] - 1 > HUFF_MAX_WORDS;
    }
    const bool any_over = __any((int)over);
    if (lane) return;
    const bool raw = ct_put_record(f, b, CT_KIND_HUFF, size, blk_len, table_bytes, state, any_over);
    f.only[b] = raw ? 0u : 1u;
}

// the order-0 codec's kinds in each of its modes (one thread per block; the rule is at ct_enc_kind0's declaration).  MODE says
// which scratch exists: nothing of a mode that is off is read.
template <uint32_t MODE>                                       // a CtMode
__global__ __launch_bounds__(256) void k_ct_kind0(CtEncFrame f, CtEncHuff0 h, CtEncSparse sp, CtEncAns an, CtEncAuto au, uint32_t nb,
                                                  uint32_t blk_len, unsigned long long table_bytes, const CtEncState *state)
{
    constexpr bool SPARSE = MODE == CT_MODE_SPARSE || MODE == CT_MODE_AUTO, ANS = MODE == CT_MODE_ANS || MODE == CT_MODE_AUTO;
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const bool pick5 = MODE == CT_MODE_ANS || (MODE == CT_MODE_AUTO && au.pick5[b] != 0), is3 = SPARSE && !pick5 && sp.is3[b] != 0;
    const unsigned long long klen = is3 ? sp.klen[b] : 0ull;
    const unsigned long long words = pick5 ? ans_words_of(an.sc.counts + (size_t)b * an.sc.nch_max, ans_chunks(blk_len))
                                   : is3 ? sp_mask_words(blk_len) + (klen ? h.nun[b] : 0ull) : h.nun[b];
    const bool raw = ct_put_record(f, b, pick5 ? CT_KIND_ANS : is3 ? CT_KIND_SPARSE : CT_KIND_HUFF0, words, blk_len, table_bytes, state);
    f.only[b] = raw || pick5 || (is3 && klen == 0) ? 1u : 0u;
    f.bwt[b] = !raw && is3 ? (int)(sp.fill[b] & 255u) : 0;
    if (ANS) an.skip_ans[b] = pick5 && !raw ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_ct_block_offsets(unsigned long long *off, unsigned long long *len, uint32_t nb, uint32_t blk_len)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb) { off[b] = (unsigned long long)b * blk_len; len[b] = blk_len; }
}

// a raw block's record: its bytes, zero-padded to a whole word (skipped when it would pass the capacity)
__global__ __launch_bounds__(256) void k_ct_raw_records(const uint8_t *__restrict__ in, uint32_t blk_len, const uint32_t *__restrict__ kind,
                                                        const unsigned long long *__restrict__ boff, uint8_t *out,
                                                        unsigned long long cap_words)
{
    const uint32_t b = blockIdx.y;
    if (kind[b] != CT_KIND_RAW) return;
    const uint32_t rw = ct_raw_words(blk_len);
    const unsigned long long o = boff[b];
    if (o + rw > cap_words) return;
    const uint8_t *src = in + (size_t)b * blk_len;
    uint32_t *dst = reinterpret_cast<uint32_t *>(out) + o;
    const bool al = (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < rw; i += gridDim.x * 256) {
        uint32_t v;
        if (al && 4 * i + 4 <= blk_len) v = reinterpret_cast<const uint32_t *>(src)[i];
        else {
            v = 0;
            for (uint32_t k = 0; k < 4; k++) if (4 * i + k < blk_len) v |= (uint32_t)src[4 * i + k] << (8 * k);
        }
        dst[i] = v;
    }
}

__global__ __launch_bounds__(256) void k_ct_segs(CtEncFrame f, const uint8_t *in, uint32_t nb, uint32_t blk_len, const uint8_t *out,
                                                 unsigned long long cap_words)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    f.seg_off[b] = (unsigned long long)(uintptr_t)(in + (size_t)b * blk_len);
    f.seg_len[b] = blk_len;
    const unsigned long long o = f.boff[b], e = f.boff[b + 1];
    f.seg_off[nb + b] = (unsigned long long)(uintptr_t)out + 4 * o;
    f.seg_len[nb + b] = e <= cap_words ? 4 * (e - o) : 0;
}

// header (table_crc still 0) and tables at the cursor; block b of the grid writes block b's rows
__global__ __launch_bounds__(256) void k_ct_tables(CtEncFrame f, uint32_t nb, uint32_t blk_len, uint8_t *out, unsigned long long cap,
                                                   const CtEncState *state)
{
    const CtTables T = ct_tables(nb, blk_len);
    const unsigned long long F = state->cursor;
    const bool fits = F + CT_FRAME_HDR + 4 * T.words <= cap;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const unsigned long long P = f.boff[nb] - f.boff[0];
    if (b == 0 && tid == 0) {
        f.seg_off[2 * nb] = (unsigned long long)(uintptr_t)out + F;
        f.seg_len[2 * nb] = fits ? 24 : 0;
        f.seg_off[2 * nb + 1] = (unsigned long long)(uintptr_t)out + F + CT_FRAME_HDR;
        f.seg_len[2 * nb + 1] = fits ? 4 * T.words : 0;
        // the payload's pad word (whole frames are 8-byte multiples)
        if ((P & 1) && f.boff[nb] + 1 <= cap / 4) reinterpret_cast<uint32_t *>(out)[f.boff[nb]] = 0;
    }
    if (!fits) return;
    uint32_t *H = reinterpret_cast<uint32_t *>(out + F);
    uint32_t *W = H + CT_FRAME_HDR / 4;
    const bool raw = f.kind[b] == CT_KIND_RAW;
    if (tid == 0) {
        W[T.kind + b] = f.kind[b];
        W[T.bwt + b] = raw ? 0u : (uint32_t)f.bwt[b];
        W[T.crc_raw + b] = f.crc[b];
        W[T.crc_rec + b] = f.crc[nb + b];
        reinterpret_cast<unsigned long long *>(W + T.pay_off)[b] = f.boff[b] - f.boff[0];
    }
    for (uint32_t i = tid; i < 256; i += 256) W[T.hist + (size_t)b * 256 + i] = raw ? 0u : f.hist[(size_t)b * 256 + i];
    const bool bwt = f.kind[b] == CT_KIND_HUFF;                // (an order-0 record has no sub-block offsets)
    for (uint32_t i = tid; i < T.nsub; i += 256) W[T.enc_off + (size_t)b * T.nsub + i] = bwt ? f.enc_off[(size_t)b * T.nsub + i] : 0u;
    if (b == 0 && tid == 0) {
        H[0] = CT_MAGIC_FRAME; H[1] = nb; H[2] = blk_len; H[3] = 0;
        H[4] = (uint32_t)P; H[5] = (uint32_t)(P >> 32); H[6] = 0; H[7] = 0;
        reinterpret_cast<unsigned long long *>(W + T.pay_off)[nb] = P;
        if (nb & 1) { W[T.kind + nb] = 0; W[T.bwt + nb] = 0; W[T.crc_raw + nb] = 0; W[T.crc_rec + nb] = 0; }
        if (((unsigned long long)nb * T.nsub) & 1) W[T.enc_off + (unsigned long long)nb * T.nsub] = 0;
    }
}

__global__ void k_ct_end(CtEncFrame f, uint32_t nb, uint32_t blk_len, uint8_t *out, unsigned long long cap, CtEncState *state)
{
    const CtTables T = ct_tables(nb, blk_len);
    const unsigned long long F = state->cursor;
    if (F + CT_FRAME_HDR + 4 * T.words <= cap)
        reinterpret_cast<uint32_t *>(out + F)[6] = shift_bytes(f.tcrc[0], 4 * T.words) ^ f.tcrc[1];
    const unsigned long long P = f.boff[nb] - f.boff[0];
    state->crc_all = shift_bytes(state->crc_all, (unsigned long long)nb * blk_len) ^ state->frame_acc;
    state->frame_acc = 0;
    state->frames += 1;
    state->cursor = F + CT_FRAME_HDR + 4 * T.words + 4 * (P + (P & 1));
}

__global__ void k_ct_trailer(uint8_t *out, unsigned long long cap, CtEncState *state, unsigned long long *d_len)
{
    const unsigned long long F = state->cursor, total = F + CT_TRAILER;
    if (total <= cap) {
        uint32_t w[4] = {CT_MAGIC_END, state->frames, state->crc_all, 0};
        uint32_t r = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < 12; i++) r = g_crc.t[0][(r ^ (w[i / 4] >> (8 * (i & 3)))) & 255] ^ (r >> 8);
        w[3] = ~r;
        for (int i = 0; i < 4; i++) reinterpret_cast<uint32_t *>(out + F)[i] = w[i];
    }
    *d_len = total;
}

hipError_t ct_enc_header(hipStream_t st, uint8_t *out, unsigned long long cap, const uint32_t hdr[8], CtEncState *state)
{
    CtHdrWords h;
    for (int i = 0; i < 8; i++) h.w[i] = hdr[i];
    hipLaunchKernelGGL(k_ct_header, dim3(1), dim3(64), 0, st, out, cap, h, state);
    return hipGetLastError();
}

hipError_t ct_enc_kind(hipStream_t st, const CtEncFrame &f, uint32_t nb, uint32_t blk_len, const CtEncState *state)
{
    const CtTables T = ct_tables(nb, blk_len);
    hipLaunchKernelGGL(k_ct_kind, dim3((nb + 3) / 4), dim3(256), 0, st, f, nb, blk_len, 4 * T.words, state);
    return hipGetLastError();
}

hipError_t ct_enc_kind0(hipStream_t st, CtMode mode, const CtEncFrame &f, const CtEncHuff0 &h, const CtEncSparse &sp, const CtEncAns &an,
                        const CtEncAuto &au, uint32_t nb, uint32_t blk_len, const CtEncState *state)
{
    const CtTables T = ct_tables(nb, blk_len);
    const auto k = mode == CT_MODE_SPARSE ? k_ct_kind0<CT_MODE_SPARSE> : mode == CT_MODE_ANS ? k_ct_kind0<CT_MODE_ANS> :
                   mode == CT_MODE_AUTO ? k_ct_kind0<CT_MODE_AUTO> : k_ct_kind0<CT_MODE_PLAIN>;
    hipLaunchKernelGGL(k, dim3((nb + 255) / 256), dim3(256), 0, st, f, h, sp, an, au, nb, blk_len, 4 * T.words, state);
    return hipGetLastError();
}

hipError_t ct_block_offsets(hipStream_t st, unsigned long long *off, unsigned long long *len, uint32_t nb, uint32_t blk_len)
{
    hipLaunchKernelGGL(k_ct_block_offsets, dim3((nb + 255) / 256), dim3(256), 0, st, off, len, nb, blk_len);
    return hipGetLastError();
}

// blocks of blk_len bytes from `bytes` on as CRC segments [0, nb)
__global__ __launch_bounds__(256) void k_ct_block_segs(unsigned long long *seg_off, unsigned long long *seg_len, const uint8_t *bytes,
                                                       uint32_t nb, uint32_t blk_len)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    seg_off[b] = (unsigned long long)(uintptr_t)(bytes + (size_t)b * blk_len);
    seg_len[b] = blk_len;
}

// format version 10: the frame's filter into word 3 of the header k_ct_tables has just written, in front of the header's CRC
__global__ void k_ct_frame_word(uint32_t nb, uint32_t blk_len, uint8_t *out, unsigned long long cap, const CtEncState *state, uint32_t word)
{
    const unsigned long long F = state->cursor;
    if (F + CT_FRAME_HDR + 4 * ct_tables(nb, blk_len).words <= cap) reinterpret_cast<uint32_t *>(out + F)[3] = word;
}

hipError_t ct_enc_after_pack(hipStream_t st, const CtEncFrame &f, const uint8_t *in, const uint8_t *orig, uint32_t nb,
                             uint32_t blk_len, uint8_t *out, unsigned long long cap, CtEncState *state, uint32_t frame_word)
{
    const uint32_t rw = ct_raw_words(blk_len);
    hipLaunchKernelGGL(k_ct_raw_records, dim3(min(8u, (rw + 255) / 256), nb), dim3(256), 0, st, in, blk_len, f.kind,
                       f.boff, out, cap / 4);
    hipLaunchKernelGGL(k_ct_segs, dim3((nb + 255) / 256), dim3(256), 0, st, f, in, nb, blk_len, (const uint8_t *)out, cap / 4);
    hipError_t e = crc32_segments(st, nullptr, f.seg_off, f.seg_len, 2 * nb, f.crc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ct_tables, dim3(nb), dim3(256), 0, st, f, nb, blk_len, out, cap, (const CtEncState *)state);
    if (frame_word) hipLaunchKernelGGL(k_ct_frame_word, dim3(1), dim3(1), 0, st, nb, blk_len, out, cap, (const CtEncState *)state, frame_word);
    e = crc32_segments(st, nullptr, f.seg_off + 2 * nb, f.seg_len + 2 * nb, 2, f.tcrc);
    if (e != hipSuccess) return e;
    if (orig) {                                                // the tables have the shuffled blocks' CRCs: their slots are free again
        hipLaunchKernelGGL(k_ct_block_segs, dim3((nb + 255) / 256), dim3(256), 0, st, f.seg_off, f.seg_len, orig, nb, blk_len);
        e = crc32_segments(st, nullptr, f.seg_off, f.seg_len, nb, f.crc);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_fold_terms, dim3((nb + 255) / 256), dim3(256), 0, st, (const uint32_t *)f.crc, nb, blk_len, &state->frame_acc);
    hipLaunchKernelGGL(k_ct_end, dim3(1), dim3(1), 0, st, f, nb, blk_len, out, cap, state);
    return hipGetLastError();
}

hipError_t ct_enc_trailer(hipStream_t st, uint8_t *out, unsigned long long cap, CtEncState *state, unsigned long long *d_len)
{
    hipLaunchKernelGGL(k_ct_trailer, dim3(1), dim3(1), 0, st, out, cap, state, d_len);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// decode: the host has checked that the frame (header, tables, payload_words of payload) lies inside the container; the
// tables themselves are unverified until k_cd_verdict, so everything read from them is clamped first
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cd_segs(CtDecFrame f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                                                 unsigned long long P, uint32_t *skip0, uint32_t kinds)
{
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *W = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR);
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(W + T.pay_off);
    const uint8_t *pay = frame + CT_FRAME_HDR + 4 * T.words;
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b == 0) { f.verdict[0] = 0; f.verdict[1] = ~0ull; }
    if (b < nb) {
        if (skip0) {                                           // (version 3 and later: whose tables are built next)
            const uint32_t kind = W[T.kind + b];
            skip0[b] = (kind == CT_KIND_HUFF0 || kind == CT_KIND_SPARSE || kind == CT_KIND_RUNS) && (kinds >> kind & 1u) ? 0u : 1u;   // (a kind-5 block has no Huffman table)
        }
        const unsigned long long lo = po[b], hi = po[b + 1];
        const bool ok = lo <= hi && hi <= P;
        f.seg_off[b] = (unsigned long long)(uintptr_t)pay + (ok ? 4 * lo : 0);
        f.seg_len[b] = ok ? 4 * (hi - lo) : 0;
    } else if (b == nb) {
        f.seg_off[b] = (unsigned long long)(uintptr_t)frame; f.seg_len[b] = 24;
    } else if (b == nb + 1) {
        f.seg_off[b] = (unsigned long long)(uintptr_t)(frame + CT_FRAME_HDR); f.seg_len[b] = 4 * T.words;
    }
}

// nun0 (version 3 and later, else null): the units the histogram of each kind-2 or kind-3 block asks for; h0: where the
// verdict leaves what the decoder of the kind-3 blocks needs
__global__ __launch_bounds__(256) void k_cd_verdict(CtDecFrame f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                                                    unsigned long long P, const unsigned long long *nun0, CtDecHuff0 h0)
{
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *H = reinterpret_cast<const uint32_t *>(frame);
    const uint32_t *W = H + CT_FRAME_HDR / 4;
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(W + T.pay_off);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b == 0 && (shift_bytes(f.crc[nb], 4 * T.words) ^ f.crc[nb + 1]) != H[6]) f.verdict[0] = 1;
    if (b >= nb) return;
    const uint32_t kind = W[T.kind + b];
    reinterpret_cast<uint32_t *>(f.verdict + 2)[b] = kind;
    const unsigned long long lo = po[b], hi = po[b + 1];
    const uint32_t legal = nun0 ? h0.kinds : ct_kinds(CT_VERSION);   // (version 6: not kind 3; 7: neither 3 nor 4; 8: not 4)
    bool bad = kind > 31u || !(legal >> kind & 1u) || lo > hi || hi > P || (b == 0 && lo != 0) || (b + 1 == nb && hi != P);
    const bool runs = nun0 && (legal >> CT_KIND_RUNS & 1u);
    unsigned long long klen = 0, nB = 0, nzw = 0;
    if (!bad) {
        const unsigned long long w = hi - lo;
        if (kind == CT_KIND_RAW) bad = w != ct_raw_words(blk_len);
        else if (kind == CT_KIND_ANS) {
            // an rANS record, the checks in the order of INTEGRATION.md 4b: the counts are the block's, nothing else is set, the
            // record holds its chunk counts (read only once it is known to), no chunk has more units than symbols, and the
            // record is exactly the counts, every chunk's 64 states and its units -- so the decoder's offsets stay inside it
            const uint32_t *h = W + T.hist + 256ull * b;
            const uint32_t nch = ans_chunks(blk_len);
            unsigned long long sum = 0, need = nch;
            for (uint32_t s = 0; s < 256; s++) sum += h[s];
            bad = sum != blk_len || W[T.bwt + b] != 0;
            const uint32_t *eo = W + T.enc_off + (size_t)b * T.nsub;
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] != 0;
            bad = bad || w < nch;
            const uint32_t *rec = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words) + lo;
            for (uint32_t c = 0; c < nch && !bad; c++) {
                const uint32_t u = rec[c];
                bad = u > min(ANS_CHUNK, blk_len - c * ANS_CHUNK);
                need += ANS_LANES + (u + 1ull) / 2;
            }
            bad = bad || need != w;
        } else if (kind == CT_KIND_RUNS) {
            // a zero-run record, the checks in the order of INTEGRATION.md 4b: the BWT index inside the block, nothing else set,
            // counts of a non-empty A; nz and the pairs read only once the record is known to hold them; the pairs ascending
            // with counts of their own that sum to A's zeros and, with A's other bytes, expand to exactly blk_len; and behind
            // the pairs exactly the units the two tables ask for -- so decoding nA and nB symbols consumes the record exactly
            // and the join of what they decode to fills the block exactly
            const uint32_t *h = W + T.hist + 256ull * b;
            const uint32_t *rec = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words) + lo;
            bad = W[T.bwt + b] >= blk_len;
            const uint32_t *eo = W + T.enc_off + (size_t)b * T.nsub;
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] != 0;
            unsigned long long sum = 0, cnt = 0, expand = 0;
            for (uint32_t s = 0; s < 256; s++) sum += h[s];
            bad = bad || sum < 1 || w < 1;
            nzw = bad ? 0 : rec[0];
            bad = bad || nzw > 256 || w < 1 + nzw;
            for (uint32_t s = 0; s < nzw && !bad; s++) {
                const unsigned long long v = rec[1 + s] >> 24, c = rec[1 + s] & 0xFFFFFFu;
                bad = c < 1 || (s > 0 && (rec[s] >> 24) >= v);
                cnt += c; expand += c * (v + 1);
            }
            bad = bad || cnt != h[0] || (sum - h[0]) + expand != blk_len;
            klen = sum; nB = cnt;
            bad = bad || w != 1 + nzw + nun0[b] + (nB ? h0.nun_b[b] : 0ull);
        } else if (kind == CT_KIND_SPARSE) {
            // a sparse record: a fill byte, nothing else set, a whole mask with its unused bits zero (read only once the record
            // is known to hold it), the counts those of the kept bytes, and behind the mask exactly the units their table asks
            // for -- so decoding klen symbols consumes the record exactly and the expansion reads exactly klen bytes
            const uint32_t nch = (blk_len + SP_CHUNK - 1) / SP_CHUNK, mw = sp_mask_words(blk_len);
            bad = W[T.bwt + b] > 255u;
            const uint32_t *eo = W + T.enc_off + (size_t)b * T.nsub;
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] != 0;
            bad = bad || w < mw;
            if (!bad) {
                const uint32_t *mask = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words) + lo;
                unsigned long long kept = 0, sum = 0;
                for (uint32_t i = 0; i < mw; i++) kept += __popc(mask[i]);
                bad = (nch & 31u) && (mask[mw - 1] >> (nch & 31u)) != 0;
                const uint32_t last = (mask[(nch - 1) >> 5] >> ((nch - 1) & 31u)) & 1u;
                klen = bad ? 0 : SP_CHUNK * kept - (last ? SP_CHUNK * nch - blk_len : 0u);
                const uint32_t *h = W + T.hist + 256ull * b;
                for (uint32_t s = 0; s < 256; s++) sum += h[s];
                bad = bad || sum != klen || w != mw + (klen ? nun0[b] : 0ull);
            }
        } else if (kind == CT_KIND_HUFF0) {
            // an order-0 record: the counts are the block's, nothing else is set, and the record has exactly the units the
            // table of those counts asks for -- so decoding blk_len symbols consumes it exactly
            unsigned long long sum = 0;
            const uint32_t *h = W + T.hist + 256ull * b;
            for (uint32_t s = 0; s < 256; s++) sum += h[s];
            bad = W[T.bwt + b] != 0 || sum != blk_len || w != nun0[b];
            const uint32_t *eo = W + T.enc_off + (size_t)b * T.nsub;
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] != 0;
        } else {
            bad = W[T.bwt + b] >= blk_len || w > (unsigned long long)T.nsub * (HUFF_MAX_WORDS + 1);
            const uint32_t *eo = W + T.enc_off + (size_t)b * T.nsub;
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] >= w || (s > 0 && eo[s] <= eo[s - 1]);
        }
    }
    if (runs) {                                                  // A into the kept space, B beside it, the join into the MTF rows
        const bool k4 = !bad && kind == CT_KIND_RUNS;
        const size_t slot = b % h0.chunk;
        h0.k_off[b] = (unsigned long long)(uintptr_t)(h0.kept + slot * h0.kept_stride);
        h0.k_len[b] = k4 ? klen : 0;
        h0.u_off[b] = k4 ? lo + 1 + nzw : 0;
        h0.skip3[b] = k4 ? 0u : 1u;
        h0.b_off[b] = (unsigned long long)(uintptr_t)(h0.kept_b + slot * h0.kept_stride);
        h0.b_len[b] = k4 ? nB : 0;
        h0.ub_off[b] = k4 ? lo + 1 + nzw + nun0[b] : 0;
        h0.skip_b[b] = k4 && nB ? 0u : 1u;
        h0.m_off[b] = (unsigned long long)(uintptr_t)(h0.mtf + slot * h0.mtf_stride);
        h0.m_len[b] = blk_len;
    } else if (nun0 && (legal >> CT_KIND_SPARSE & 1u)) {
        const bool k3 = !bad && kind == CT_KIND_SPARSE;
        h0.k_off[b] = (unsigned long long)(uintptr_t)(h0.kept + (size_t)(b % h0.chunk) * h0.kept_stride);
        h0.k_len[b] = k3 ? klen : 0;
        h0.u_off[b] = k3 ? lo + sp_mask_words(blk_len) : 0;
        h0.skip3[b] = k3 && klen ? 0u : 1u;
    }
    if (bad) atomicMin(&f.verdict[1], ((unsigned long long)CT_FRAME_TABLE << 32) | b);
    else if (f.crc[b] != W[T.crc_rec + b]) atomicMin(&f.verdict[1], ((unsigned long long)CT_RECORD_CRC << 32) | b);
}

// raw records out (verified); every block's output range becomes a segment for the decoded-bytes check
__global__ __launch_bounds__(256) void k_cd_raw(CtDecFrame f, const uint8_t *frame, uint32_t nb, uint32_t blk_len, uint8_t *out,
                                                uint32_t first)
{
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *W = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR);
    const uint32_t b = first + blockIdx.y;
    uint8_t *dst = out + (size_t)b * blk_len;
    if (blockIdx.x == 0 && threadIdx.x == 0) { f.seg_off[b] = (unsigned long long)(uintptr_t)dst; f.seg_len[b] = blk_len; }
    if (W[T.kind + b] != CT_KIND_RAW) return;
    const unsigned long long lo = reinterpret_cast<const unsigned long long *>(W + T.pay_off)[b];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words) + lo;
    const bool al = (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < ct_raw_words(blk_len); i += gridDim.x * 256) {
        const uint32_t v = src[i];
        if (al && 4 * i + 4 <= blk_len) reinterpret_cast<uint32_t *>(dst)[i] = v;
        else for (uint32_t k = 0; k < 4; k++) if (4 * i + k < blk_len) dst[4 * i + k] = (uint8_t)(v >> (8 * k));
    }
}

__global__ __launch_bounds__(256) void k_cd_check(CtDecFrame f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                                                  uint32_t frame_index, CtDecState *state, uint32_t first, uint32_t end)
{
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *W = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR);
    const uint32_t b = first + blockIdx.x * 256 + threadIdx.x;
    if (b < end && f.crc[b] != W[T.crc_raw + b]) atomicMin(&state->err, (((unsigned long long)frame_index << 32) | b) + 1);
}

__global__ void k_cd_end(uint32_t nb, uint32_t blk_len, CtDecState *state)
{
    state->crc_all = shift_bytes(state->crc_all, (unsigned long long)nb * blk_len) ^ state->frame_acc;
    state->frame_acc = 0;
}

hipError_t ct_dec_verify(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                         unsigned long long payload_words, const CtDecHuff0 *h0, KernelProf *prof)
{
    hipLaunchKernelGGL(k_cd_segs, dim3((nb + 2 + 255) / 256), dim3(256), 0, st, f, frame, nb, blk_len, payload_words,
                       h0 ? h0->skip : nullptr, h0 ? h0->kinds : ct_kinds(CT_VERSION));
    hipError_t e = hipSuccess;
    if (h0) {
        const CtTables T = ct_tables(nb, blk_len);
        uint32_t *hist = const_cast<uint32_t *>(reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR) + T.hist);   // (read only)
        if (h0->kinds >> CT_KIND_DEDUP & 1u) {                 // (version 9: a kind-6 block has a table like a kind-2 block's)
            e = ct_dec_dedup_skip(st, frame, nb, h0->skip);
            if (e != hipSuccess) return e;
        }
        const HdbSegs g{nullptr, nullptr, nullptr, nb, blk_len};
        e = hdb_tables(st, g, false, hist, nullptr, nullptr, h0->lut, h0->nun, h0->skip, prof);
        if (e != hipSuccess) return e;
        if (h0->kinds >> CT_KIND_RUNS & 1u) {                  // (version 6: the tables of B, from the counts in the records)
            e = ct_dec_runs_hist(st, frame, nb, blk_len, payload_words, *h0);
            if (e != hipSuccess) return e;
            e = hdb_tables(st, g, false, h0->hist_b, nullptr, nullptr, h0->lut_b, h0->nun_b, h0->skip_tb, prof);
            if (e != hipSuccess) return e;
        }
    }
    e = crc32_segments(st, nullptr, f.seg_off, f.seg_len, nb + 2, f.crc);
    if (e != hipSuccess) return e;
    if (h0 && (h0->kinds >> CT_KIND_DEDUP & 1u)) return ct_dec_dedup_verdict(st, f, frame, nb, blk_len, payload_words, *h0);
    hipLaunchKernelGGL(k_cd_verdict, dim3((nb + 255) / 256), dim3(256), 0, st, f, frame, nb, blk_len, payload_words,
                       h0 ? (const unsigned long long *)h0->nun : nullptr, h0 ? *h0 : CtDecHuff0{});
    return hipGetLastError();
}

hipError_t ct_dec_raw(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len, uint8_t *out,
                      uint32_t first, uint32_t count)
{
    if (first >= nb) return hipSuccess;
    if (count == 0 || count > nb - first) count = nb - first;
    hipLaunchKernelGGL(k_cd_raw, dim3(min(8u, (ct_raw_words(blk_len) + 255) / 256), count), dim3(256), 0, st, f, frame, nb, blk_len, out,
                       first);
    return hipGetLastError();
}

hipError_t ct_dec_check(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                        const uint8_t *out, uint32_t frame_index, CtDecState *state, bool fold, uint32_t first, uint32_t count)
{
    (void)out;                                                 // (k_cd_raw put the output ranges in f.seg_*)
    if (first >= nb) return hipSuccess;
    if (count == 0 || count > nb - first) count = nb - first;
    hipError_t e = crc32_segments(st, nullptr, f.seg_off + first, f.seg_len + first, count, f.crc + first);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cd_check, dim3((count + 255) / 256), dim3(256), 0, st, f, frame, nb, blk_len, frame_index, state, first,
                       first + count);
    if (!fold || count != nb) return hipGetLastError();
    hipLaunchKernelGGL(k_fold_terms, dim3((nb + 255) / 256), dim3(256), 0, st, (const uint32_t *)f.crc, nb, blk_len, &state->frame_acc);
    hipLaunchKernelGGL(k_cd_end, dim3(1), dim3(1), 0, st, nb, blk_len, state);
    return hipGetLastError();
}

hipError_t ct_dec_fold(hipStream_t st, const CtDecFrame &f, const uint8_t *bytes, uint32_t nb, uint32_t blk_len, CtDecState *state)
{
    hipLaunchKernelGGL(k_ct_block_segs, dim3((nb + 255) / 256), dim3(256), 0, st, f.seg_off, f.seg_len, bytes, nb, blk_len);
    hipError_t e = crc32_segments(st, nullptr, f.seg_off, f.seg_len, nb, f.crc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fold_terms, dim3((nb + 255) / 256), dim3(256), 0, st, (const uint32_t *)f.crc, nb, blk_len, &state->frame_acc);
    hipLaunchKernelGGL(k_cd_end, dim3(1), dim3(1), 0, st, nb, blk_len, state);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// the frame index of a container in device memory: ct_walk, the walk every reader makes, run by one thread.  The chain is
// serial by nature -- a frame's size is in its header and the next header lies behind it -- so there is nothing for a second
// lane to do: one dependent 32-byte read per frame.  Every read lies inside [in, in + len): the walk tests the position of a
// header against len before it fetches it.  Entry fi is written only while fi < cap.
// ---------------------------------------------------------------------------
__global__ void k_ct_index(const uint8_t *in, unsigned long long len, uint32_t plan_n, uint32_t reader, CtIndexHead *head,
                           CtFrameRef *entries, unsigned long long cap)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    CtIndexHead h = {};
    const CtWalkEnd end = ct_walk(
        g_crc, len, plan_n, reader,
        [&](uint32_t *dst, unsigned long long pos, uint32_t bytes, unsigned long long) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(in + pos);       // (pos is a multiple of 8, as is `in`)
            for (uint32_t i = 0; i < bytes / 4; i++) dst[i] = src[i];
            return true;
        },
        [&](const uint32_t *hdr, const CtFormat &, uint32_t, unsigned long long) {
            for (int i = 0; i < 8; i++) h.hdr[i] = hdr[i];
            return true;
        },
        [&](uint32_t fi, const uint32_t *, const CtFrameRef &ref) {
            if (fi >= cap) return false;
            entries[fi] = ref;
            h.frames = fi + 1;
            return true;
        },
        [&](const uint32_t *tr, uint32_t) {
            for (int i = 0; i < 4; i++) h.trailer[i] = tr[i];
            return true;
        });
    h.what = end.what;
    h.frame = end.frame;
    *head = h;
}

hipError_t ct_index_device(hipStream_t st, const uint8_t *in, unsigned long long len, uint32_t plan_n, uint32_t reader,
                           CtIndexHead *head, CtFrameRef *entries, unsigned long long cap)
{
    hipLaunchKernelGGL(k_ct_index, dim3(1), dim3(64), 0, st, in, len, plan_n, reader, head, entries, cap);
    return hipGetLastError();
}

__global__ void k_ct_put(unsigned long long *p, unsigned long long v) { *p = v; }
hipError_t ct_put_u64(hipStream_t st, unsigned long long *p, unsigned long long v)
{
    hipLaunchKernelGGL(k_ct_put, dim3(1), dim3(1), 0, st, p, v);
    return hipGetLastError();
}

} // namespace glc
