// dedup.hip -- the passes of the container's dedup mode ("dedup"): which 512-byte chunks of a frame repeat an
// earlier chunk of the same frame, and the copy that puts them back.  gfx950 / wave64.
// The segments of a call are the blocks of one frame, in order; segment i is cut into chunks of 512 bytes from its start (the
// last may be short) and chunk c of segment i has the frame-wide id g = i * nch + c, nch = ceil(max_len / 512).  Eight lanes own
// a chunk, 64 bytes a lane; a workgroup of 256 lanes takes 32 chunks a pass.
//   k_dd_hash    one read of the frame: a lane sums its eight products (w + k)(w' + k'), the eight partial sums are folded
//                across the DPP row (two quad permutes and the half mirror), the chunk's length is added and fmix64 finishes the
//                hash.  The hash goes to hash[g] and, in the same kernel, into the table: a slot is claimed by a compare-and-swap
//                on its 64-bit key, the smallest id that came for a key is kept with atomicMin, probing is linear.  A chunk
//                whose hash equals that of the chunk in front of it in the same workgroup (DD_PASSES * 32 consecutive ids of one
//                segment) leaves the table alone: the id in front is smaller, the minimum does not change, and a frame of
//                equal chunks sends one atomic per workgroup to the slot instead of one per chunk.
//   k_dd_verify  cand(g) = the id stored with hash[g]; where it is smaller than g, the eight lanes compare their 64 bytes with
//                the candidate's, one ballot per wave decides eight chunks; src[g] = cand(g) when bytes and lengths agree, else g
//   k_dd_fill    the inverse: every chunk whose entry is not its own id is copied from the chunk the entry names
// Loads are the address-aligned 16-byte granules that cover a lane's 64 bytes (five when the address is not 16-byte aligned,
// funnelled in registers; a granule that holds a byte of a buffer lies in that byte's page, as in shuffle.hip), so any byte
// alignment runs the same code.  No kernel needs more LDS than the 33 hashes of a pass.
// Behind them the container's own steps: per block the mask, the refs, the lowest source block and kind 6 or 2 (k_dd_decide), the
// record sizes (k_dd_kind), mask and refs into the records (k_dd_place); and for the decoder the verdict of a version-9 frame
// (k_dd_verdict), the frame's map and the masks widened to 64-byte chunks (k_dd_dec_expand), with which sparse.hip's mover does
// the compaction and the join.
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t DD_THREADS = 256, DD_PASS_CHUNKS = DD_THREADS / 8, DD_PASSES = 4;
constexpr uint64_t DD_EMPTY = ~0ull, DD_GOLD = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint32_t dd_len(const DdSegs &g, uint32_t i)
{
    const unsigned long long l = g.data_len[i];
    return l > g.max_len ? g.max_len : (uint32_t)l;
}
__device__ __forceinline__ uint8_t *dd_data(const DdSegs &g, uint32_t i) { return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.data) + g.data_off[i]); }

// the n <= 64 bytes at p (n > 0, any alignment) as sixteen little-endian words, bytes from n on zero.  Only aligned 16-byte
// granules that hold one of the n bytes are read.
__device__ __forceinline__ void dd_load64(const uint8_t *p, uint32_t n, uint32_t (&w)[16])
{
    const uintptr_t A = reinterpret_cast<uintptr_t>(p), A0 = A & ~(uintptr_t)15;
    const uint32_t s = (uint32_t)(A - A0);
    uint32_t d[21];
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (16 * k < s + n) v = *reinterpret_cast<const uint4 *>(A0 + 16 * k);
        d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
    d[20] = 0;
    // s = 4 * dw + sb: whole dwords by two select stages (no run-time register index), the bytes by a funnel shift
    if (s & 4) {
#pragma unroll
        for (uint32_t j = 0; j < 20; j++) d[j] = d[j + 1];
    }
    if (s & 8) {
#pragma unroll
        for (uint32_t j = 0; j < 19; j++) d[j] = d[j + 2];
    }
    const uint32_t sh = 8 * (s & 3);
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) w[j] = __funnelshift_r(d[j], d[j + 1], sh);
    if (n < 64) {
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t have = n > 4 * j ? n - 4 * j : 0u;          // bytes of word j inside the chunk
            w[j] = have >= 4 ? w[j] : have == 0 ? 0u : w[j] & ((1u << (8 * have)) - 1u);
        }
    }
}

// sum over the eight lanes of a chunk, on every one of them: lanes 8 q .. 8 q + 7 of a DPP row
__device__ __forceinline__ uint64_t dd_fold8(uint64_t x)
{
#pragma unroll
    for (uint32_t step = 0; step < 3; step++) {
        const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
        uint32_t ylo, yhi;
        if (step == 0) { ylo = GLC_DPP(lo, 0xB1, 0xf); yhi = GLC_DPP(hi, 0xB1, 0xf); }         // quad_perm [1,0,3,2]
        else if (step == 1) { ylo = GLC_DPP(lo, 0x4E, 0xf); yhi = GLC_DPP(hi, 0x4E, 0xf); }    // quad_perm [2,3,0,1]
        else { ylo = GLC_DPP(lo, 0x141, 0xf); yhi = GLC_DPP(hi, 0x141, 0xf); }                 // row_half_mirror: the other quad
        x += ((uint64_t)yhi << 32) | ylo;
    }
    return x;
}

__device__ __forceinline__ uint64_t dd_fmix64(uint64_t h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

// this lane's share of the sum: words 16 sub .. 16 sub + 15 of the chunk
__device__ __forceinline__ uint64_t dd_partial(const uint32_t (&w)[16], uint32_t sub)
{
    uint64_t kk = DD_GOLD * (16 * sub + 1), acc = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        const uint32_t k0 = (uint32_t)(kk >> 32), k1 = (uint32_t)((kk + DD_GOLD) >> 32);
        kk += 2 * DD_GOLD;
        acc += (uint64_t)(w[2 * i] + k0) * (uint64_t)(w[2 * i + 1] + k1);
    }
    return acc;
}

// key -> slot walk.  INSERT: claim or find the key's slot and keep the smallest id; else: the id stored with the key (or `g`)
template <bool INSERT>
__device__ __forceinline__ uint32_t dd_table(const DdSegs &g, uint64_t h, uint32_t id)
{
    if (h == DD_EMPTY) {                                               // the one key the empty mark hides: a slot of its own
        uint32_t *own = &g.table[g.slots].id;
        if (INSERT) { atomicMin(own, id); return id; }
        return *own;
    }
    const uint32_t mask = g.slots - 1;
    uint32_t s = (uint32_t)(h >> 20) & mask;
    for (uint32_t tries = 0; tries < g.slots; tries++, s = (s + 1) & mask) {
        if (INSERT) {
            const unsigned long long k = atomicCAS(reinterpret_cast<unsigned long long *>(&g.table[s].key), (unsigned long long)DD_EMPTY,
                                                   (unsigned long long)h);
            if (k == DD_EMPTY || k == h) { atomicMin(&g.table[s].id, id); return id; }
        } else {
            const uint64_t k = g.table[s].key;
            if (k == h) return g.table[s].id;
            if (k == DD_EMPTY) return id;
        }
    }
    return id;
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_hash(DdSegs g)
{
    __shared__ uint64_t s_h[DD_PASS_CHUNKS + 1];                       // [0]: the chunk in front of the pass, [1 + q]: chunk q of it
    const uint32_t b = blockIdx.x, tid = threadIdx.x, q = tid >> 3, sub = tid & 7;
    const uint32_t L = dd_len(g, b), nch = g.nch;
    const uint32_t c_first = blockIdx.y * (DD_PASSES * DD_PASS_CHUNKS);
    if ((unsigned long long)c_first * DD_CHUNK >= L) return;           // (workgroup-uniform)
    const uint8_t *in = dd_data(g, b);
    for (uint32_t p = 0; p < DD_PASSES; p++) {
        const uint32_t c = c_first + p * DD_PASS_CHUNKS + q;
        const uint32_t o = c * DD_CHUNK;                               // (c <= 2048 + 127: no overflow)
        const bool live = c < nch && o < L;
        const uint32_t clen = live ? min(DD_CHUNK, L - o) : 0u;
        uint32_t w[16];
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) w[j] = 0;
        if (64 * sub < clen) dd_load64(in + o + 64 * sub, min(64u, clen - 64 * sub), w);
        const uint64_t h = dd_fmix64(dd_fold8(dd_partial(w, sub)) + clen);
        if (sub == 0) s_h[1 + q] = h;
        __syncthreads();
        if (sub == 0 && live) {
            const uint32_t id = b * nch + c;
            g.hash[id] = h;
            const bool twin_in_front = (p | q) != 0 && s_h[q] == h;   // the chunk in front is live whenever this one is
            if (!twin_in_front) (void)dd_table<true>(g, h, id);
        }
        __syncthreads();
        if (tid == DD_THREADS - 8) s_h[0] = h;
    }
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_verify(DdSegs g)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x, q = tid >> 3, sub = tid & 7, lane = tid & 63;
    const uint32_t L = dd_len(g, b), nch = g.nch;
    const uint32_t c = blockIdx.y * DD_PASS_CHUNKS + q;
    if (blockIdx.y * DD_PASS_CHUNKS >= nch) return;
    const uint32_t o = c * DD_CHUNK, id = b * nch + c;
    const bool live = c < nch && o < L;
    const uint32_t clen = live ? min(DD_CHUNK, L - o) : 0u;
    uint32_t cand = id;
    if (live) cand = dd_table<false>(g, g.hash[id], id);
    bool differ = false;
    if (cand < id) {
        const uint32_t sb = cand / nch, sc = cand - sb * nch;
        const uint32_t SL = dd_len(g, sb), so = sc * DD_CHUNK;
        const uint32_t slen = so < SL ? min(DD_CHUNK, SL - so) : 0u;
        if (slen != clen) differ = true;
        else if (64 * sub < clen) {
            const uint32_t n = min(64u, clen - 64 * sub);
            uint32_t x[16], y[16];
            dd_load64(dd_data(g, b) + o + 64 * sub, n, x);
            dd_load64(dd_data(g, sb) + so + 64 * sub, n, y);
            uint32_t acc = 0;
#pragma unroll
            for (uint32_t j = 0; j < 16; j++) acc |= x[j] ^ y[j];
            differ = acc != 0;
        }
    }
    const unsigned long long v = __ballot((int)differ);
    const bool same = ((v >> (lane & ~7u)) & 0xFFull) == 0;
    if (sub == 0 && c < nch) g.src[id] = same ? cand : id;
}

// sixteen words to the n <= 64 bytes at p
__device__ __forceinline__ void dd_store64(uint8_t *p, uint32_t n, const uint32_t (&w)[16])
{
    if (n == 64 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) reinterpret_cast<uint4 *>(p)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 64; j++) if (j < n) p[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}

__global__ __launch_bounds__(DD_THREADS) void k_dd_fill(DdSegs g, uint32_t first)
{
    const uint32_t b = first + blockIdx.x, tid = threadIdx.x, q = tid >> 3, sub = tid & 7;
    const uint32_t L = dd_len(g, b), nch = g.nch;
    const uint32_t c = blockIdx.y * DD_PASS_CHUNKS + q;
    const uint32_t o = c * DD_CHUNK, id = b * nch + c;
    if (c >= nch || o >= L) return;
    const uint32_t clen = min(DD_CHUNK, L - o);
    const uint32_t from = g.src[id];
    if (from >= id) return;                                            // kept, or an entry the format does not allow
    const uint32_t sb = from / nch, sc = from - sb * nch;
    const uint32_t SL = dd_len(g, sb), so = sc * DD_CHUNK;
    if (so >= SL || min(DD_CHUNK, SL - so) != clen || 64 * sub >= clen) return;
    const uint32_t n = min(64u, clen - 64 * sub);
    uint32_t w[16];
    dd_load64(dd_data(g, sb) + so + 64 * sub, n, w);
    dd_store64(dd_data(g, b) + o + 64 * sub, n, w);
}

size_t dedup_slots(size_t chunks)
{
    size_t s = 64;
    while (s < 2 * chunks) s <<= 1;
    return s;
}

hipError_t dedup_map(hipStream_t st, const DdSegs &g)
{
    if (g.count == 0 || g.nch == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(g.table, 0xFF, ((size_t)g.slots + 1) * sizeof(DdSlot), st);
    if (e != hipSuccess) return e;
    const uint32_t per = DD_PASSES * DD_PASS_CHUNKS;
    hipLaunchKernelGGL(k_dd_hash, dim3(g.count, (g.nch + per - 1) / per), dim3(DD_THREADS), 0, st, g);
    hipLaunchKernelGGL(k_dd_verify, dim3(g.count, (g.nch + DD_PASS_CHUNKS - 1) / DD_PASS_CHUNKS), dim3(DD_THREADS), 0, st, g);
    return hipGetLastError();
}

hipError_t dedup_fill(hipStream_t st, const DdSegs &g, uint32_t first, uint32_t count)
{
    if (g.count == 0 || g.nch == 0 || first >= g.count) return hipSuccess;
    if (count == 0 || count > g.count - first) count = g.count - first;
    hipLaunchKernelGGL(k_dd_fill, dim3(count, (g.nch + DD_PASS_CHUNKS - 1) / DD_PASS_CHUNKS), dim3(DD_THREADS), 0, st, g, first);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the container encoder's steps around the map (container_api.cpp, Encoder::frame_dedup)
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t dd_chunks(uint32_t len) { return (len + DD_CHUNK - 1) / DD_CHUNK; }
__host__ __device__ inline uint32_t dd_mask_words(uint32_t len) { return (dd_chunks(len) + 31) / 32; }

// the byte of a 64-byte-chunk mask (sparse.hip's) that stands for 512-byte chunk c of a block of L bytes when it is kept
__device__ __forceinline__ uint32_t dd_byte64(uint32_t L, uint32_t c)
{
    const uint32_t clen = min(DD_CHUNK, L - c * DD_CHUNK);
    return (1u << ((clen + SP_CHUNK - 1) / SP_CHUNK)) - 1u;
}

// per block (one workgroup each), from its row of the map: the mask, E, the refs in chunk order (a prefix count over the mask
// words), the lowest block a source lies in, kind 6 or 2 by the rule 15 E >= mask words, and for a kind-6 block what the
// compaction (sparse.hip's mover, driven by the mask widened to 64-byte chunks), the tables and the encoder then work on
__global__ __launch_bounds__(256) void k_dd_decide(CtEncDedup dd, CtEncSparse sp, const unsigned long long *blk_off, const uint8_t *d_in,
                                                   uint32_t blk_len, uint32_t *hist, unsigned long long *in_off, unsigned long long *in_len)
{
    __shared__ uint32_t s_tmp[256 / WAVE + 1];
    __shared__ uint32_t s_lo;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t nch = dd_chunks(blk_len), mw = dd_mask_words(blk_len), mw64 = sp_mask_words(blk_len);
    const uint32_t *row = dd.src + (size_t)b * dd.nch;
    if (tid == 0) s_lo = b;
    uint32_t word = 0, elided = 0;
    if (tid < mw) {
        for (uint32_t k = 0; k < 32; k++) {
            const uint32_t c = 32 * tid + k;
            if (c < nch && row[c] == b * dd.nch + c) word |= 1u << k;
        }
        elided = min(32u, nch - 32 * tid) - __popc(word);
        dd.mask[(size_t)b * dd.mask_stride + tid] = word;
        uint32_t *m64 = sp.mask + (size_t)b * sp.mask_stride;
        for (uint32_t j = 0; j < 8; j++) {
            uint32_t w = 0;
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t c = 32 * tid + 4 * j + k;
                if (c < nch && (word >> (4 * j + k) & 1u)) w |= dd_byte64(blk_len, c) << (8 * k);
            }
            if (8 * tid + j < mw64) m64[8 * tid + j] = w;
        }
    }
    uint32_t E = 0;
    uint32_t at = block_excl_add<256>(elided, s_tmp, &E);          // (its barriers also publish s_lo)
    if (tid < mw) {
        for (uint32_t k = 0; k < 32; k++) {
            const uint32_t c = 32 * tid + k;
            if (c >= nch || (word >> k & 1u)) continue;
            const uint32_t r = row[c];
            dd.refs[(size_t)b * dd.nch + at++] = r;
            atomicMin(&s_lo, r / dd.nch);
        }
    }
    __syncthreads();
    const bool is6 = 15ull * E >= mw;                              // (E = 0 never is: mw >= 1)
    const bool last_elided = !(row[nch - 1] == b * dd.nch + nch - 1);
    const uint32_t klen = blk_len - (DD_CHUNK * E - (last_elided ? DD_CHUNK * nch - blk_len : 0u));
    if (is6 && klen == 0) hist[(size_t)b * 256 + tid] = 0;         // (no table of nothing: the counts of K are zeros)
    if (tid) return;
    dd.E[b] = E;
    dd.lo[b] = s_lo;
    sp.fill[b] = 0;                                                // (sparse.hip's mover reads a fill byte; the compaction does not use it)
    sp.klen[b] = klen;
    sp.is3[b] = is6 ? 1u : 0u;
    sp.skip_move[b] = is6 ? 0u : 1u;
    sp.skip_table[b] = is6 && klen == 0 ? 1u : 0u;
    in_off[b] = (unsigned long long)(uintptr_t)(is6 ? sp.kept + sp.kept_off[b] : d_in + blk_off[b]);
    in_len[b] = is6 ? klen : blk_len;
}

// the dedup mode's ct_enc_kind (one thread per block): kind 6 where the rule chose it -- mask, refs and, when anything is kept, the
// stream h.nun counts -- else kind 2, and raw under the record rule whichever it was; the lowest source block into f.bwt
__global__ __launch_bounds__(256) void k_dd_kind(CtEncFrame f, CtEncHuff0 h, CtEncSparse sp, CtEncDedup dd, uint32_t nb, uint32_t blk_len,
                                                 unsigned long long table_bytes, const CtEncState *state)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const bool is6 = sp.is3[b] != 0;
    const unsigned long long klen = is6 ? sp.klen[b] : 0ull;
    const unsigned long long words = is6 ? dd_mask_words(blk_len) + dd.E[b] + (klen ? h.nun[b] : 0ull) : h.nun[b];
    const bool raw = ct_put_record(f, b, is6 ? CT_KIND_DEDUP : CT_KIND_HUFF0, words, blk_len, table_bytes, state);
    f.only[b] = raw || (is6 && klen == 0) ? 1u : 0u;
    f.bwt[b] = !raw && is6 ? (int)dd.lo[b] : 0;
}

// behind the payload offsets: mask and refs into the kind-6 records (those that end inside the capacity), and where every
// block's stream starts
__global__ __launch_bounds__(256) void k_dd_place(CtEncFrame f, CtEncSparse sp, CtEncDedup dd, uint32_t blk_len, uint32_t *out,
                                                  unsigned long long cap_words)
{
    const uint32_t b = blockIdx.x, mw = dd_mask_words(blk_len);
    const bool is6 = f.kind[b] == CT_KIND_DEDUP;
    const unsigned long long o = f.boff[b];
    const uint32_t E = is6 ? dd.E[b] : 0u;
    if (threadIdx.x == 0) sp.unit_off[b] = o + (is6 ? mw + E : 0u);
    if (!is6 || f.boff[b + 1] > cap_words) return;
    for (uint32_t i = threadIdx.x; i < mw; i += 256) out[o + i] = dd.mask[(size_t)b * dd.mask_stride + i];
    for (uint32_t i = threadIdx.x; i < E; i += 256) out[o + mw + i] = dd.refs[(size_t)b * dd.nch + i];
}

hipError_t ct_enc_dedup_decide(hipStream_t st, const CtEncDedup &dd, const CtEncSparse &sp, const unsigned long long *blk_off, const uint8_t *d_in,
                               uint32_t nb, uint32_t blk_len, uint32_t *hist, unsigned long long *in_off, unsigned long long *in_len)
{
    hipLaunchKernelGGL(k_dd_decide, dim3(nb), dim3(256), 0, st, dd, sp, blk_off, d_in, blk_len, hist, in_off, in_len);
    return hipGetLastError();
}

hipError_t ct_enc_dedup_kind(hipStream_t st, const CtEncFrame &f, const CtEncHuff0 &h, const CtEncSparse &sp, const CtEncDedup &dd, uint32_t nb,
                             uint32_t blk_len, const CtEncState *state)
{
    const CtTables T = ct_tables(nb, blk_len);
    hipLaunchKernelGGL(k_dd_kind, dim3((nb + 255) / 256), dim3(256), 0, st, f, h, sp, dd, nb, blk_len, 4 * T.words, state);
    return hipGetLastError();
}

hipError_t ct_enc_dedup_place(hipStream_t st, const CtEncFrame &f, const CtEncSparse &sp, const CtEncDedup &dd, uint32_t nb, uint32_t blk_len,
                              uint32_t *out, unsigned long long cap_words)
{
    hipLaunchKernelGGL(k_dd_place, dim3(nb), dim3(256), 0, st, f, sp, dd, blk_len, out, cap_words);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the container decoder's steps (container_api.cpp, Decoder::frame; container.hip, ct_dec_verify)
// ---------------------------------------------------------------------------------------------------------------------
__device__ const CrcX2n g_dd_x2n = crc_make_x2n();
__device__ __forceinline__ uint32_t dd_shift_bytes(uint32_t r, unsigned long long n) { return crc_multmodp(crc_x8n(n, g_dd_x2n), r); }

// a kind-6 block's table is built from its histogram like a kind-2 block's (k_cd_segs leaves it out)
__global__ __launch_bounds__(256) void k_dd_dec_skip(const uint8_t *frame, uint32_t nb, uint32_t *skip0)
{
    const uint32_t *W = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b < nb && W[b] == CT_KIND_DEDUP) skip0[b] = 0;             // (T.kind = 0)
}

// the verdict of a version-9 frame (kinds 0, 1, 2 and 6): k_cd_verdict's checks of kinds 0, 1 and 2 word for word, and for kind 6
// the field checks of INTEGRATION.md 4b in their order, one workgroup per block.  The mask and the refs are read only once the
// record is known to hold them; a source in another kind-6 block is looked up in that block's mask only when that block's own
// record holds it.  With the checks passed the decoder reads nothing outside the record and the fill writes nothing outside
// the block.
__global__ __launch_bounds__(256) void k_dd_verdict(CtDecFrame f, const uint8_t *frame, uint32_t nb, uint32_t blk_len, unsigned long long P,
                                                    const unsigned long long *nun0, CtDecHuff0 h0)
{
    __shared__ uint32_t s_tmp[256 / WAVE + 1];
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *H = reinterpret_cast<const uint32_t *>(frame);
    const uint32_t *W = H + CT_FRAME_HDR / 4;
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(W + T.pay_off);
    const uint32_t *pay = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words);
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b == 0 && tid == 0 && (dd_shift_bytes(f.crc[nb], 4 * T.words) ^ f.crc[nb + 1]) != H[6]) f.verdict[0] = 1;
    const uint32_t kind = W[T.kind + b];
    if (tid == 0) reinterpret_cast<uint32_t *>(f.verdict + 2)[b] = kind;
    const unsigned long long lo = po[b], hi = po[b + 1];
    const uint32_t legal = h0.kinds;
    bool bad = kind > 31u || !(legal >> kind & 1u) || lo > hi || hi > P || (b == 0 && lo != 0) || (b + 1 == nb && hi != P);
    const unsigned long long w = bad ? 0 : hi - lo;
    const uint32_t *eo = W + T.enc_off + (size_t)b * T.nsub;
    const uint32_t *h = W + T.hist + 256ull * b;
    const uint32_t nch = dd_chunks(blk_len), mw = dd_mask_words(blk_len);
    unsigned long long klen = 0, E = 0;
    if (!bad && kind == CT_KIND_DEDUP) {                           // (workgroup-uniform: every lane sees the same fields)
        bool eo_set = false;
        for (uint32_t s = tid; s < T.nsub; s += 256) eo_set |= eo[s] != 0;
        bad = __syncthreads_or((int)eo_set) != 0 || w < mw;
        if (!bad) {
            const uint32_t *mask = pay + lo;
            uint32_t kept = 0;
            for (uint32_t i = 0; i < mw; i++) kept += __popc(mask[i]);
            const bool unused = (nch & 31u) && (mask[mw - 1] >> (nch & 31u)) != 0;
            E = unused ? 0 : nch - kept;
            bad = unused || w < mw + E;
            if (!bad) {
                const uint32_t *refs = mask + mw;
                const uint32_t lob = W[T.bwt + b];
                bool wrong = false;
                for (uint32_t c = tid; c < nch; c += 256) {
                    if (mask[c >> 5] >> (c & 31u) & 1u) continue;
                    uint32_t rank = c - __popc(mask[c >> 5] & ((1u << (c & 31u)) - 1u));
                    for (uint32_t i = 0; i < (c >> 5); i++) rank -= __popc(mask[i]);
                    const uint32_t r = refs[rank], sb = r / nch, sc = r - sb * nch;
                    bool ok = r < b * nch + c && sb >= lob && sb <= b &&
                              min(DD_CHUNK, blk_len - sc * DD_CHUNK) == min(DD_CHUNK, blk_len - c * DD_CHUNK);
                    if (ok && sb == b) ok = (mask[sc >> 5] >> (sc & 31u) & 1u) != 0;
                    else if (ok && W[T.kind + sb] == CT_KIND_DEDUP) {  // (another kind: all its chunks are kept)
                        const unsigned long long slo = po[sb], shi = po[sb + 1];
                        ok = slo <= shi && shi <= P && shi - slo >= mw && (pay[slo + (sc >> 5)] >> (sc & 31u) & 1u) != 0;
                    }
                    wrong |= !ok;
                }
                bad = __syncthreads_or((int)wrong) != 0 || lob > b;
                const uint32_t last = (mask[(nch - 1) >> 5] >> ((nch - 1) & 31u)) & 1u;
                klen = DD_CHUNK * (unsigned long long)kept - (last ? DD_CHUNK * nch - blk_len : 0u);
                uint32_t sum_lo = 0, sum_hi = 0;               // (two 16-bit halves: 256 counts of any value sum without a wrap)
                (void)block_excl_add<256>(h[tid] & 0xFFFFu, s_tmp, &sum_lo);
                (void)block_excl_add<256>(h[tid] >> 16, s_tmp, &sum_hi);
                bad = bad || (((unsigned long long)sum_hi << 16) + sum_lo) != klen || w != mw + E + (klen ? nun0[b] : 0ull);
            }
        }
    } else if (!bad && tid == 0) {
        if (kind == CT_KIND_RAW) bad = w != ct_raw_words(blk_len);
        else if (kind == CT_KIND_HUFF0) {
            unsigned long long sum = 0;
            for (uint32_t s = 0; s < 256; s++) sum += h[s];
            bad = W[T.bwt + b] != 0 || sum != blk_len || w != nun0[b];
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] != 0;
        } else {
            bad = W[T.bwt + b] >= blk_len || w > (unsigned long long)T.nsub * (HUFF_MAX_WORDS + 1);
            for (uint32_t s = 0; s < T.nsub && !bad; s++) bad = eo[s] >= w || (s > 0 && eo[s] <= eo[s - 1]);
        }
    }
    if (tid) return;
    const bool k6 = !bad && kind == CT_KIND_DEDUP;
    h0.k_off[b] = (unsigned long long)(uintptr_t)(h0.kept + (size_t)(b % h0.chunk) * h0.kept_stride);
    h0.k_len[b] = k6 ? klen : 0;
    h0.u_off[b] = k6 ? lo + mw + E : 0;
    h0.skip3[b] = k6 && klen ? 0u : 1u;
    if (bad) atomicMin(&f.verdict[1], ((unsigned long long)CT_FRAME_TABLE << 32) | b);
    else if (f.crc[b] != W[T.crc_rec + b]) atomicMin(&f.verdict[1], ((unsigned long long)CT_RECORD_CRC << 32) | b);
}

// blocks [first, first + count) of a verified frame.  MASKS = false: their src rows (own ids; for a kind-6 block the refs at its
// elided chunks).  MASKS = true: for the kind-6 blocks, the mask widened to 64-byte chunks in row b % chunk of mask64, what
// sparse.hip's join reads (rows are reused from one decoder chunk to the next, so this runs with each chunk's join)
template <bool MASKS>
__global__ __launch_bounds__(256) void k_dd_dec_expand(const uint8_t *frame, uint32_t nb, uint32_t blk_len, uint32_t first, CtDecDedup dd)
{
    const CtTables T = ct_tables(nb, blk_len);
    const uint32_t *W = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR);
    const unsigned long long *po = reinterpret_cast<const unsigned long long *>(W + T.pay_off);
    const uint32_t *pay = reinterpret_cast<const uint32_t *>(frame + CT_FRAME_HDR + 4 * T.words);
    const uint32_t b = first + blockIdx.x, tid = threadIdx.x;
    const uint32_t nch = dd_chunks(blk_len), mw = dd_mask_words(blk_len), mw64 = sp_mask_words(blk_len);
    uint32_t *row = dd.src + (size_t)b * nch;
    if (W[T.kind + b] != CT_KIND_DEDUP) {
        if (!MASKS) for (uint32_t c = tid; c < nch; c += 256) row[c] = b * nch + c;
        return;
    }
    const uint32_t *mask = pay + po[b], *refs = mask + mw;
    uint32_t *m64 = dd.mask64 + (size_t)(b % dd.chunk) * dd.stride64;
    for (uint32_t c = tid; c < nch && !MASKS; c += 256) {
        const bool kept = (mask[c >> 5] >> (c & 31u) & 1u) != 0;
        uint32_t rank = c - __popc(mask[c >> 5] & ((1u << (c & 31u)) - 1u));
        for (uint32_t i = 0; i < (c >> 5); i++) rank -= __popc(mask[i]);
        row[c] = kept ? b * nch + c : refs[rank];
    }
    for (uint32_t i = tid; i < mw64 && MASKS; i += 256) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t c = 4 * i + k;
            if (c < nch && (mask[c >> 5] >> (c & 31u) & 1u)) w |= dd_byte64(blk_len, c) << (8 * k);
        }
        m64[i] = w;
    }
}

hipError_t ct_dec_dedup_skip(hipStream_t st, const uint8_t *frame, uint32_t nb, uint32_t *skip0)
{
    hipLaunchKernelGGL(k_dd_dec_skip, dim3((nb + 255) / 256), dim3(256), 0, st, frame, nb, skip0);
    return hipGetLastError();
}

hipError_t ct_dec_dedup_verdict(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                                unsigned long long payload_words, const CtDecHuff0 &h0)
{
    hipLaunchKernelGGL(k_dd_verdict, dim3(nb), dim3(256), 0, st, f, frame, nb, blk_len, payload_words, (const unsigned long long *)h0.nun, h0);
    return hipGetLastError();
}

hipError_t ct_dec_dedup_expand(hipStream_t st, const uint8_t *frame, uint32_t nb, uint32_t blk_len, uint32_t first, uint32_t count,
                               const CtDecDedup &dd, bool masks)
{
    hipLaunchKernelGGL(masks ? k_dd_dec_expand<true> : k_dd_dec_expand<false>, dim3(count), dim3(256), 0, st, frame, nb, blk_len, first, dd);
    return hipGetLastError();
}

} // namespace glc
