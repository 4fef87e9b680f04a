// sparse.hip -- the sparse mode of the container's order-0 codec (record kind 3, format version 5): the
// bandwidth-bound passes in front of and behind the batched Huffman kernels of hd_batch.hip.  gfx950 / wave64.
// A segment (a block of a frame) is cut into chunks of 64 bytes; a chunk whose bytes all equal the segment's fill byte is
// ELIDED, the others are KEPT: bit c % 32 of mask word c / 32 is 1 for a kept chunk.  A workgroup of 256 lanes owns a tile
// of 16 KiB = 256 chunks = 8 mask words of one segment; a lane moves 16 bytes, four lanes a chunk.
//   k_sp_mask     one read of the segment: every lane compares its 16 bytes with the broadcast fill, the wave's ballot is
//                 the verdict of 16 chunks per KiB (a chunk is elided when its four lanes all agree), a wave writes two words
//   k_sp_count    one workgroup per segment: kept chunks = popcount of its mask words; the bytes of K
//   k_sp_compact  the kept chunks, in order, to the segment's scratch.  A tile finds its output offset itself: 64 * popcount
//                 of the segment's mask words in front of it (at most 512 words for 1 MiB, summed by the workgroup), so no
//                 workgroup waits for another and there is no scan across workgroups
//   k_sp_join     the inverse: every chunk is 64 bytes of fill or the chunk at 64 * (its rank among the kept ones) of K
// 16-byte loads and stores where the segment's address allows, a byte-granular path where it does not; any length, any
// byte alignment, out of place.  The container's own steps (fill byte, kind 3 or 2 with the histogram correction, record
// sizes, masks into the records) are the small kernels at the end.
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t SP_THREADS = 256, SP_TILE_WORDS = 8;

__device__ __forceinline__ uint32_t sp_len(const SpSegs &g, uint32_t i)
{
    const unsigned long long l = g.data_len[i];
    return l > g.max_len ? g.max_len : (uint32_t)l;
}
__device__ __forceinline__ uint8_t *sp_data(const SpSegs &g, uint32_t i) { return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.data) + g.data_off[i]); }
__device__ __forceinline__ uint8_t *sp_kept(const SpSegs &g, uint32_t i) { return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.kept) + g.kept_off[i]); }
__device__ __forceinline__ uint32_t *sp_mask(const SpSegs &g, uint32_t i)
{
    return g.mask + (g.mask_off ? g.mask_off[i] : (unsigned long long)i * g.mask_stride);
}

// n <= 16 bytes at p as four dwords; bytes from n on read as `pad`
__device__ __forceinline__ uint4 sp_load16(const uint8_t *p, uint32_t n, bool aligned, uint32_t pad)
{
    if (aligned && n == 16) return *reinterpret_cast<const uint4 *>(p);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) w[k >> 2] |= (uint32_t)(k < n ? p[k] : (uint8_t)pad) << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void sp_store16(uint8_t *p, uint32_t n, bool aligned, uint4 v)
{
    if (aligned && n == 16) { *reinterpret_cast<uint4 *>(p) = v; return; }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) if (k < n) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_mask(SpSegs g)
{
    const uint32_t b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g.skip && g.skip[b]) return;
    const uint32_t L = sp_len(g, b), nch = (L + SP_CHUNK - 1) / SP_CHUNK, mw = (nch + 31) / 32;
    const uint32_t w0 = blockIdx.y * SP_TILE_WORDS + 2 * wave;     // this wave's two words: 4 KiB, four passes of 1 KiB
    if (w0 >= mw) return;
    const uint8_t *in = sp_data(g, b);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const uint32_t f4 = (g.fill[b] & 255u) * 0x01010101u;
    uint4 q[4];
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) {
        const unsigned long long o = ((unsigned long long)w0 * 32 + 16 * p) * SP_CHUNK + 16 * lane;
        q[p] = make_uint4(f4, f4, f4, f4);                         // (past the end: never a reason to keep a chunk)
        if (o < L) q[p] = sp_load16(in + o, (uint32_t)min(16ull, L - o), al, f4);
    }
    uint32_t words[2] = {0, 0};
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) {
        const bool ne = ((q[p].x ^ f4) | (q[p].y ^ f4) | (q[p].z ^ f4) | (q[p].w ^ f4)) != 0;
        unsigned long long v = __ballot((int)ne);
        v |= v >> 1; v |= v >> 2;                                  // bit 4 j: any of chunk j's four lanes differs
        uint32_t m = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) m |= (uint32_t)((v >> (4 * j)) & 1ull) << j;
        words[p >> 1] |= m << (16 * (p & 1));
    }
    if (lane == 0) {
        uint32_t *mask = sp_mask(g, b);
        mask[w0] = words[0];
        if (w0 + 1 < mw) mask[w0 + 1] = words[1];
    }
}

// kept chunks of a segment from its mask words, on every lane of the workgroup
__device__ __forceinline__ uint32_t sp_kept_chunks(const uint32_t *mask, uint32_t nwords, uint32_t *s_tmp)
{
    uint32_t c = 0, total = 0;
    for (uint32_t i = threadIdx.x; i < nwords; i += SP_THREADS) c += __popc(mask[i]);
    (void)block_excl_add<SP_THREADS>(c, s_tmp, &total);
    return total;
}

// the bytes of K: whole chunks but for a kept short last one
__device__ __forceinline__ uint32_t sp_klen(const uint32_t *mask, uint32_t kept, uint32_t L, uint32_t nch)
{
    if (nch == 0) return 0;
    const uint32_t last = (mask[(nch - 1) >> 5] >> ((nch - 1) & 31)) & 1u;
    return SP_CHUNK * kept - (last ? SP_CHUNK * nch - L : 0u);
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_count(SpSegs g, unsigned long long *klen)
{
    __shared__ uint32_t s_tmp[SP_THREADS / WAVE + 1];
    const uint32_t b = blockIdx.x;
    if (g.skip && g.skip[b]) return;
    const uint32_t L = sp_len(g, b), nch = (L + SP_CHUNK - 1) / SP_CHUNK, mw = (nch + 31) / 32;
    const uint32_t *mask = sp_mask(g, b);
    const uint32_t kept = sp_kept_chunks(mask, mw, s_tmp);
    if (threadIdx.x == 0) klen[b] = sp_klen(mask, kept, L, nch);
}

// JOIN = false: kept chunks of the tile from the segment to K; true: every chunk of the tile from K or from the fill
template <bool JOIN>
__global__ __launch_bounds__(SP_THREADS) void k_sp_move(SpSegs g)
{
    __shared__ uint32_t s_tmp[SP_THREADS / WAVE + 1];
    __shared__ uint32_t s_m[SP_TILE_WORDS];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (g.skip && g.skip[b]) return;
    const uint32_t L = sp_len(g, b), nch = (L + SP_CHUNK - 1) / SP_CHUNK, mw = (nch + 31) / 32;
    const uint32_t w0 = blockIdx.y * SP_TILE_WORDS;
    if (w0 >= mw) return;
    const uint32_t *mask = sp_mask(g, b);
    if (tid < SP_TILE_WORDS) s_m[tid] = w0 + tid < mw ? mask[w0 + tid] : 0u;
    const uint32_t before = sp_kept_chunks(mask, w0, s_tmp);       // (its barriers also publish s_m)
    uint32_t rank0[SP_TILE_WORDS];                                 // kept chunks in front of each word of the tile
    uint32_t run = before;
#pragma unroll
    for (uint32_t j = 0; j < SP_TILE_WORDS; j++) { rank0[j] = run; run += __popc(s_m[j]); }
    uint8_t *data = sp_data(g, b), *K = sp_kept(g, b);
    const bool al_d = (reinterpret_cast<uintptr_t>(data) & 15) == 0, al_k = (reinterpret_cast<uintptr_t>(K) & 15) == 0;
    const uint32_t f4 = (g.fill[b] & 255u) * 0x01010101u;
#pragma unroll
    for (uint32_t p = 0; p < SP_TILE_WORDS / 2; p++) {             // 64 chunks a pass
        const uint32_t cl = 64 * p + (tid >> 2), word = cl >> 5, bit = cl & 31;
        const uint32_t c = w0 * 32 + cl;
        const unsigned long long o = (unsigned long long)c * SP_CHUNK + 16 * (tid & 3);
        if (c >= nch || o >= L) continue;
        const uint32_t n = (uint32_t)min(16ull, L - o);
        const uint32_t m = s_m[word];
        const bool kept = (m >> bit) & 1u;
        uint32_t r = 0;
#pragma unroll
        for (uint32_t j = 0; j < SP_TILE_WORDS; j++) if (j == word) r = rank0[j];
        const unsigned long long ko = (unsigned long long)(r + __popc(m & ((1u << bit) - 1u))) * SP_CHUNK + 16 * (tid & 3);
        if (JOIN) sp_store16(data + o, n, al_d, kept ? sp_load16(K + ko, n, al_k, 0) : make_uint4(f4, f4, f4, f4));
        else if (kept) sp_store16(K + ko, n, al_k, sp_load16(data + o, n, al_d, 0));
    }
}

static uint32_t sp_tiles(uint32_t max_len)
{
    const uint32_t mw = ((max_len + SP_CHUNK - 1) / SP_CHUNK + 31) / 32;
    return (mw + SP_TILE_WORDS - 1) / SP_TILE_WORDS;
}

hipError_t sparse_mask(hipStream_t st, const SpSegs &g)
{
    if (g.count == 0 || g.max_len == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sp_mask, dim3(g.count, sp_tiles(g.max_len)), dim3(SP_THREADS), 0, st, g);
    return hipGetLastError();
}

hipError_t sparse_count(hipStream_t st, const SpSegs &g, unsigned long long *d_klen)
{
    if (g.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sp_count, dim3(g.count), dim3(SP_THREADS), 0, st, g, d_klen);
    return hipGetLastError();
}

hipError_t sparse_compact(hipStream_t st, const SpSegs &g)
{
    if (g.count == 0 || g.max_len == 0) return hipSuccess;
    hipLaunchKernelGGL((k_sp_move<false>), dim3(g.count, sp_tiles(g.max_len)), dim3(SP_THREADS), 0, st, g);
    return hipGetLastError();
}

hipError_t sparse_join(hipStream_t st, const SpSegs &g)
{
    if (g.count == 0 || g.max_len == 0) return hipSuccess;
    hipLaunchKernelGGL((k_sp_move<true>), dim3(g.count, sp_tiles(g.max_len)), dim3(SP_THREADS), 0, st, g);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the container encoder's steps around them (container_api.cpp, Encoder::frame_sparse)
// ---------------------------------------------------------------------------------------------------------------------
// fill = the block's most frequent byte, the lowest value on a tie: one wave per block, four symbols a lane
__global__ __launch_bounds__(256) void k_sp_fill(const uint32_t *__restrict__ hist, uint32_t nb, uint32_t *__restrict__ fill)
{
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nb) return;
    uint32_t best = 0;                                             // (count << 8) | (255 - symbol); counts are at most 2^20
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t s = 4 * lane + k, key = (hist[(size_t)b * 256 + s] << 8) | (255u - s);
        best = key > best ? key : best;
    }
    best = wave_max(best);
    if (lane == 0) fill[b] = 255u - (best & 255u);
}

// kind 3 or 2 per block (one workgroup each): E elided chunks, kind 3 when 32 E >= nch.  A kind-3 block's histogram becomes
// that of K without a pass over the data -- only the fill's count changes, by the elided bytes -- and the block becomes the
// segment (kept scratch, klen) the tables and the encoder then work on; the others stay (frame block, blk_len).
__global__ __launch_bounds__(SP_THREADS) void k_sp_decide(SpSegs g, CtEncSparse sp, uint32_t *hist, unsigned long long *in_off,
                                                         unsigned long long *in_len)
{
    __shared__ uint32_t s_tmp[SP_THREADS / WAVE + 1];
    const uint32_t b = blockIdx.x;
    const uint32_t L = sp_len(g, b), nch = (L + SP_CHUNK - 1) / SP_CHUNK, mw = (nch + 31) / 32;
    const uint32_t *mask = sp_mask(g, b);
    const uint32_t kept = sp_kept_chunks(mask, mw, s_tmp);
    if (threadIdx.x) return;
    const uint32_t klen = sp_klen(mask, kept, L, nch);
    const bool is3 = 32ull * (nch - kept) >= nch;
    sp.klen[b] = klen;
    sp.is3[b] = is3 ? 1u : 0u;
    sp.skip_move[b] = is3 ? 0u : 1u;
    sp.skip_table[b] = is3 && klen ? 0u : 1u;
    if (is3) hist[(size_t)b * 256 + (g.fill[b] & 255u)] -= L - klen;
    in_off[b] = (unsigned long long)(uintptr_t)(is3 ? sp_kept(g, b) : sp_data(g, b));
    in_len[b] = is3 ? klen : L;
}

// behind the payload offsets: the masks into the kind-3 records (those that end inside the capacity), and where every
// block's stream starts
__global__ __launch_bounds__(256) void k_sp_place(CtEncFrame f, CtEncSparse sp, uint32_t blk_len, uint32_t *out, unsigned long long cap_words)
{
    const uint32_t b = blockIdx.x, mw = sp_mask_words(blk_len);
    const bool is3 = f.kind[b] == CT_KIND_SPARSE;
    const unsigned long long o = f.boff[b];
    if (threadIdx.x == 0) sp.unit_off[b] = o + (is3 ? mw : 0u);
    if (!is3 || f.boff[b + 1] > cap_words) return;
    const uint32_t *mask = sp.mask + (size_t)b * sp.mask_stride;
    for (uint32_t i = threadIdx.x; i < mw; i += 256) out[o + i] = mask[i];
}

hipError_t ct_enc_sparse_decide(hipStream_t st, const SpSegs &g, const CtEncSparse &sp, uint32_t *hist, unsigned long long *in_off,
                                unsigned long long *in_len)
{
    hipLaunchKernelGGL(k_sp_decide, dim3(g.count), dim3(SP_THREADS), 0, st, g, sp, hist, in_off, in_len);
    return hipGetLastError();
}

hipError_t ct_enc_sparse_fill(hipStream_t st, const uint32_t *hist, uint32_t nb, uint32_t *fill)
{
    hipLaunchKernelGGL(k_sp_fill, dim3((nb + 3) / 4), dim3(256), 0, st, hist, nb, fill);
    return hipGetLastError();
}

hipError_t ct_enc_sparse_place(hipStream_t st, const CtEncFrame &f, const CtEncSparse &sp, uint32_t nb, uint32_t blk_len, uint32_t *out,
                               unsigned long long cap_words)
{
    hipLaunchKernelGGL(k_sp_place, dim3(nb), dim3(256), 0, st, f, sp, blk_len, out, cap_words);
    return hipGetLastError();
}

} // namespace glc
