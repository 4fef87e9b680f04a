// hd_device.h -- device code the single-stream kernels (hd_encode.hip, hd_decode.hip) and the batched ones (hd_batch.hip)
// of the CUHD-shaped Huffman-only stream share: the table builder's body, the encoder's per-tile loads and merge, the
// decoder's per-span walks.  gfx950 / wave64.
#pragma once
#include "glc_device.h"
#include "../../include/glc_hd.h"

namespace glc {

// ---------------------------------------------------------------------------------------------------------------------
// table: glcHdBuildTable (hd_decode.hip) restated for one workgroup of 512 lanes
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HT_NT = 512;
constexpr int HT_MAXI = 512;                            // items of a level: at most 2m - 1 = 511
constexpr int HT_LEVELS = GLC_HD_MAX_LEN;               // L0 .. L10
constexpr uint16_t HT_PKG = 0x8000;                     // item reference: package j = HT_PKG | j, else leaf index

// LUT16 = false: table2048 is the reference's {num_bits, symbol}[2048] (entries no codeword reaches {0, 0}); true: the u16
// form the decode kernels read, (bits << 8) | symbol, with 1 bit for the entries no codeword reaches.  lens, codes and
// table2048 may each be null.  Returns the bits a stream of the histogram's symbols takes, the sum of hist[s] * lens[s]
// (in every lane).
template <class HistT, bool LUT16>
__device__ __forceinline__ unsigned long long hd_table_body(const HistT *__restrict__ hist, uint8_t *__restrict__ lens,
                                                            uint16_t *__restrict__ codes, uint32_t *__restrict__ table2048)
{
    __shared__ unsigned long long s_hist[256];
    __shared__ unsigned long long s_leaf[256];          // A: leaf weights, ascending (the stable sort)
    __shared__ unsigned long long s_w[2][HT_MAXI];      // weights of level k-1 / k by position
    __shared__ unsigned long long s_pk[HT_MAXI / 2];    // packages of level k-1
    __shared__ uint16_t s_ref[HT_LEVELS][HT_MAXI];      // what item p of level k is
    __shared__ uint32_t s_mult[2][HT_MAXI];
    __shared__ uint8_t s_sym[256];                      // leaf i -> symbol
    __shared__ uint32_t s_len[256];                     // by symbol
    __shared__ uint32_t s_lo[256];                      // by canonical rank: first 11-bit prefix of the code
    __shared__ uint32_t s_rsym[256];                    // by canonical rank: (len << 8) | symbol
    __shared__ uint32_t s_cnt[GLC_HD_MAX_LEN + 2];
    __shared__ uint32_t s_m;
    __shared__ unsigned long long s_bits;
    const uint32_t tid = threadIdx.x;
    if (tid < 256) { s_hist[tid] = hist[tid]; s_len[tid] = 0; }
    if (tid < GLC_HD_MAX_LEN + 2) s_cnt[tid] = 0;
    if (tid == 0) { s_m = 0; s_bits = 0; }
    __syncthreads();
    // stable sort by count = rank: smaller counts, then equal counts of lower symbols, go first
    if (tid < 256) {
        const unsigned long long h = s_hist[tid];
        if (h) {
            uint32_t r = 0;
            for (uint32_t s = 0; s < 256; s++) {
                const unsigned long long g = s_hist[s];
                r += (g && (g < h || (g == h && s < tid))) ? 1u : 0u;
            }
            s_leaf[r] = h;
            s_sym[r] = (uint8_t)tid;
            atomicAdd(&s_m, 1u);
        }
    }
    __syncthreads();
    const uint32_t m = s_m;
    if (m == 1 && tid == 0) s_len[s_sym[0]] = 1;
    if (m >= 2) {
        // L0 = the leaves
        if (tid < m) { s_w[0][tid] = s_leaf[tid]; s_ref[0][tid] = (uint16_t)tid; }
        uint32_t n = m;                                 // items of the level before
        int cur = 0;
        for (int k = 1; k < HT_LEVELS; k++) {
            const uint32_t np = n / 2;
            __syncthreads();
            if (tid < np) s_pk[tid] = s_w[cur][2 * tid] + s_w[cur][2 * tid + 1];
            __syncthreads();
            // merged position = own index + items of the other list ahead of it: packages lighter than a leaf,
            // leaves no heavier than a package (a leaf goes before a package of equal weight)
            if (tid < m) {
                const unsigned long long w = s_leaf[tid];
                uint32_t lo = 0, hi = np;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_pk[mid] < w) lo = mid + 1; else hi = mid; }
                s_w[cur ^ 1][tid + lo] = w;
                s_ref[k][tid + lo] = (uint16_t)tid;
            } else if (tid - m < np) {
                const uint32_t j = tid - m;
                const unsigned long long w = s_pk[j];
                uint32_t lo = 0, hi = m;
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_leaf[mid] <= w) lo = mid + 1; else hi = mid; }
                s_w[cur ^ 1][j + lo] = w;
                s_ref[k][j + lo] = (uint16_t)(HT_PKG | j);
            }
            cur ^= 1;
            n = m + np;
        }
        // code length of leaf i = its occurrences in the first 2m - 2 items of L10: push the multiplicities down
        if (tid < HT_MAXI) s_mult[0][tid] = (tid < 2 * m - 2 && tid < n) ? 1u : 0u;
        int mb = 0;
        for (int k = HT_LEVELS - 1; k >= 0; k--) {
            __syncthreads();
            if (tid < HT_MAXI) s_mult[mb ^ 1][tid] = 0;
            __syncthreads();
            if (tid < HT_MAXI) {                        // (items past a level's size carry multiplicity 0)
                const uint32_t mu = s_mult[mb][tid];
                if (mu) {
                    const uint32_t r = s_ref[k][tid];
                    if (r & HT_PKG) { const uint32_t j = r & 0x7FFFu; s_mult[mb ^ 1][2 * j] = mu; s_mult[mb ^ 1][2 * j + 1] = mu; }
                    else s_len[s_sym[r]] += mu;         // a leaf occurs once per level: no other lane adds to it here
                }
            }
            mb ^= 1;
        }
    }
    __syncthreads();
    // canonical codes by (length, symbol)
    if (tid < 256 && s_len[tid]) {
        atomicAdd(&s_cnt[s_len[tid]], 1u);
        atomicAdd(&s_bits, s_hist[tid] * s_len[tid]);
    }
    __syncthreads();
    const unsigned long long bits = s_bits;
    if (tid < 256) {
        const uint32_t l = s_len[tid];
        uint32_t code = 0, rank = 0;
        if (l) {
            // first code of length l (deflate's next_code; s_cnt[0] = 0), then this symbol's place among those of length l.
            // Equal to glcHdBuildTable's walk in (length, symbol) order: both start at 0 and shift by the length step.
            for (uint32_t b = 1; b <= l; b++) code = (code + s_cnt[b - 1]) << 1;
            uint32_t before = 0;
            for (uint32_t s = 0; s < tid; s++) before += s_len[s] == l ? 1u : 0u;
            for (uint32_t b = 1; b < l; b++) rank += s_cnt[b];
            code += before;
            rank += before;
            s_lo[rank] = code << (GLC_HD_MAX_LEN - l);
            s_rsym[rank] = (l << 8) | tid;
        }
        if (lens) lens[tid] = (uint8_t)l;
        if (codes) codes[tid] = (uint16_t)code;
    }
    if (!table2048) return bits;
    __syncthreads();
    // decoder table {num_bits, symbol}[2048]: entry e belongs to the last code (in canonical order) whose span starts at
    // or before e, if e lies inside that span; entries no codeword reaches are {0, 0}
    uint32_t nc = 0;
    for (int b = 1; b <= GLC_HD_MAX_LEN; b++) nc += s_cnt[b];
    for (uint32_t q = tid; q < 1024; q += HT_NT) {      // two entries per word: little-endian {bits, sym, bits, sym}
        uint32_t word = LUT16 ? 0x01000100u : 0u;
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t e = 2 * q + h;
            uint32_t lo = 0, hi = nc;                   // first rank whose span starts past e
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_lo[mid] <= e) lo = mid + 1; else hi = mid; }
            if (lo) {
                const uint32_t rs = s_rsym[lo - 1], l = rs >> 8;
                if (e < s_lo[lo - 1] + (1u << (GLC_HD_MAX_LEN - l))) {
                    if (LUT16) word = (word & ~(0xFFFFu << (16 * h))) | (rs << (16 * h));
                    else word |= ((l | ((rs & 0xFFu) << 8)) << (16 * h));
                }
            }
        }
        table2048[q] = word;
    }
    return bits;
}

// ---------------------------------------------------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HE_NT = 256;
constexpr int HE_SPT = 16;                              // symbols per lane: one 16-byte load
constexpr uint32_t HE_TILE = HE_NT * HE_SPT;            // 4096 symbols per tile
constexpr uint32_t HE_TPW = 4;                          // tiles per workgroup (the table arrives once)
constexpr uint32_t HE_BAD = 0xFFFFFFFFu;                // tile bits: a symbol without a usable code
constexpr int HE_MAXW = (HE_TILE * GLC_HD_MAX_LEN + 31) / 32 + 4;   // + the start offset inside the first word, rounded

// {code, length} of every symbol in one word: code in bits 0..15, length in 16..23; an unusable code becomes length 0x80
__device__ __forceinline__ void he_load_table(const uint8_t *__restrict__ lens, const uint16_t *__restrict__ codes, uint32_t *s_cl)
{
    const uint32_t t = threadIdx.x;
    const uint32_t l = lens[t];
    const uint32_t ok = l >= 1 && l <= GLC_HD_MAX_LEN;
    s_cl[t] = ok ? ((l << 16) | (codes[t] & ((1u << l) - 1u))) : (0x80u << 16);
}

__device__ __forceinline__ void he_load_syms(const uint8_t *__restrict__ in, size_t nsym, size_t s0, uint32_t (&w)[4])
{
    const uint8_t *p = in + s0;
    if (s0 + HE_SPT <= nsym && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {                                             // unaligned input or the ragged end: bytes (past the end: 0)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) { const size_t i = s0 + 4 * k + b; x |= (i < nsym ? (uint32_t)p[4 * k + b] : 0u) << (8 * b); }
            w[k] = x;
        }
    }
}

// One tile's bits (HE_BAD: a symbol of the tile has no usable code), valid in thread 0; every lane of the workgroup calls
// it.  s_tmp: HE_NT / WAVE + 1 words.
__device__ __forceinline__ uint32_t he_count_tile(const uint8_t *__restrict__ in, size_t nsym, size_t s0, const uint32_t *s_cl,
                                                  uint32_t *s_tmp)
{
    const uint32_t tid = threadIdx.x;
    uint32_t w[4];
    he_load_syms(in, nsym, s0, w);
    uint32_t bits = 0;
    bool mybad = false;
#pragma unroll
    for (int j = 0; j < HE_SPT; j++) {
        const uint32_t ln = s0 + j < nsym ? s_cl[(w[j >> 2] >> (8 * (j & 3))) & 0xFFu] >> 16 : 0u;
        bits += ln;
        mybad |= (ln & 0x80u) != 0;
    }
    const uint32_t wsum = wave_sum(bits);           // <= 64 * 16 * 0x80: no wrap
    __syncthreads();                                // thread 0 has read s_tmp of the previous tile
    if ((tid & 63) == 0) s_tmp[tid >> 6] = wsum;
    const bool anybad = __syncthreads_or((int)mybad) != 0;
    uint32_t tot = 0;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < HE_NT / WAVE; i++) tot += s_tmp[i];
    }
    return anybad ? HE_BAD : tot;
}

// One tile merged into s_words (HE_MAXW words of LDS, 16-byte aligned) from bit sh of word 0; s_tmp: HE_NT / WAVE + 1
// words.  Every lane of the workgroup calls it; returns the tile's bits.  The words are complete behind its last barrier.
__device__ __forceinline__ uint32_t he_merge_tile(const uint8_t *__restrict__ in, size_t nsym, size_t s0, uint32_t sh,
                                                  const uint32_t *s_cl, uint32_t *s_words, uint32_t *s_tmp)
{
    const uint32_t tid = threadIdx.x;
    uint32_t w[4];
    he_load_syms(in, nsym, s0, w);
    uint32_t cl[HE_SPT];
    uint32_t mybits = 0;
#pragma unroll
    for (int j = 0; j < HE_SPT; j++) {
        const uint32_t v = s0 + j < nsym ? s_cl[(w[j >> 2] >> (8 * (j & 3))) & 0xFFu] : 0u;
        cl[j] = (v & (0x80u << 16)) ? 0u : v;       // (the scan's verdict excludes these; kept in bounds regardless)
        mybits += cl[j] >> 16;
    }
    uint32_t total = 0;
    const uint32_t start = sh + block_excl_add<HE_NT>(mybits, s_tmp, &total);
    const uint32_t nw = (sh + total + 31) / 32;
    for (uint32_t i = tid; 4 * i < nw; i += HE_NT) reinterpret_cast<uint4 *>(s_words)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    // merge, two codes at a time (<= 22 bits): `hi` is the word being filled, MSB first (k_huff_pack's scheme)
    uint32_t wi = start >> 5, fill = start & 31u, hi = 0;
#pragma unroll
    for (int j = 0; j < HE_SPT; j += 2) {
        const uint32_t l1 = cl[j + 1] >> 16;
        const uint32_t ln = (cl[j] >> 16) + l1;
        const uint32_t cd = ((cl[j] & 0xFFFFu) << l1) | (cl[j + 1] & 0xFFFFu);
        const uint64_t V = (uint64_t)cd << ((64u - fill - ln) & 63u);
        hi |= (uint32_t)(V >> 32);
        const uint32_t nf = fill + ln;
        const bool full = nf >= 32;
        if (full) atomicOr(&s_words[wi], hi);
        wi += full ? 1u : 0u;
        hi = full ? (uint32_t)V : hi;
        fill = nf & 31u;
    }
    if (fill > 0 && mybits > 0) atomicOr(&s_words[wi], hi);
    __syncthreads();
    return total;
}

// units [dst, + nw) of a tile that starts at bit sh of dst[0] and holds `total` bits: a word the tile covers whole is
// stored; the first word when the tile starts inside it and the last when the tile ends inside it are shared with the
// neighbours and ORed onto zeros established before this kernel
__device__ __forceinline__ void he_store_tile(const uint32_t *s_words, uint32_t sh, uint32_t total, uint32_t *dst)
{
    const uint32_t nw = (sh + total + 31) / 32;
    const bool end_part = ((sh + total) & 31u) != 0;
    for (uint32_t i = threadIdx.x; i < nw; i += HE_NT) {
        const uint32_t v = s_words[i];
        if ((i == 0 && sh) || (i == nw - 1 && end_part)) { if (v) atomicOr(&dst[i], v); }
        else dst[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HD_SPAN   = 32;                    // units per lane
constexpr int HD_PITCH  = HD_SPAN + 1;           // LDS pitch (bank-conflict-free) + look-ahead unit
constexpr int HD_LANES  = 256;
constexpr int HD_WG_UNITS = HD_SPAN * HD_LANES;  // 8192 units = 32 KiB per workgroup
constexpr int HD_NOFF   = 11;                    // start offsets 0..10
constexpr int HD_TSTRIDE = 12;                   // words per stored table
constexpr int HD_SPAN_BITS = HD_SPAN * 32;
constexpr int HD_CHK_PITCH = 34;                 // u16 per lane (17 words: odd, conflict-free)

__device__ __forceinline__ void hd_stage(const uint32_t *__restrict__ units, size_t nunits, size_t base_unit,
                                         uint32_t *s_u, const uint16_t *__restrict__ lut, uint16_t *s_lut)
{
    const uint32_t tid = threadIdx.x;
    {   // batches of 8 independent loads, then the LDS stores (a load->store loop is one latency per trip)
        uint32_t q[8];
#pragma unroll
        for (int r = 0; r < 8; r++) q[r] = lut[r * HD_LANES + tid];        // two 16-bit entries per word are not
#pragma unroll                                                            // worth it: the table is read once
        for (int r = 0; r < 8; r++) s_lut[r * HD_LANES + tid] = (uint16_t)q[r];
        const bool full = base_unit + HD_WG_UNITS <= nunits;
#pragma unroll 1
        for (uint32_t i0 = 0; i0 < HD_WG_UNITS; i0 += 8 * HD_LANES) {
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t i = i0 + r * HD_LANES + tid;
                const size_t gu = base_unit + i;
                q[r] = units[full || gu < nunits ? gu : 0];
                if (!full && gu >= nunits) q[r] = 0u;
            }
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const uint32_t i = i0 + r * HD_LANES + tid;
                s_u[(i >> 5) * HD_PITCH + (i & 31)] = q[r];
            }
        }
    }
    __syncthreads();
    {   // look-ahead unit of every lane = first unit of the next lane / next workgroup
        const size_t gu = base_unit + HD_WG_UNITS;
        const uint32_t nxt = (tid + 1 < HD_LANES) ? s_u[(tid + 1) * HD_PITCH] : (gu < nunits ? units[gu] : 0u);
        s_u[tid * HD_PITCH + HD_SPAN] = nxt;
    }
    __syncthreads();
}

// Path from offset 0, recording for every unit the first codeword boundary inside it (every 32-bit
// unit holds at least two boundaries: codewords are <= 11 bits): chk[u] = symbols before it << 5 | bit.
__device__ __forceinline__ uint32_t hd_decode_ref(const uint32_t *U, const uint16_t *s_lut, uint16_t *chk)
{
    uint32_t pos = 0, cnt = 0, last_u = 0xFFFFFFFFu;
    uint64_t w = ((uint64_t)U[0] << 32) | U[1];
    uint32_t valid = 64, next = 2;
    while (pos < HD_SPAN_BITS) {
        const uint32_t u = pos >> 5;
        if (u != last_u) { chk[u] = (uint16_t)((cnt << 5) | (pos & 31)); last_u = u; }
        const uint32_t len = s_lut[(uint32_t)(w >> (64 - GLC_HD_MAX_LEN))] >> 8;
        w <<= len; pos += len; valid -= len; cnt++;
        if (valid <= 32 && next <= HD_SPAN) { w |= (uint64_t)U[next] << (32 - valid); valid += 32; next++; }
    }
    return (cnt << 4) | (pos - HD_SPAN_BITS);
}

// Path from offset o > 0: Huffman codes self-synchronise, so it usually falls onto the reference
// path within a few codewords; from there on the two are identical, and the result is the
// reference's (end offset, count) corrected by the symbols decoded so far.  Checked once per unit.
__device__ __forceinline__ uint32_t hd_decode_merge(const uint32_t *U, const uint16_t *s_lut, const uint16_t *chk,
                                                    uint32_t ref, uint32_t o)
{
    uint32_t pos = o, cnt = 0, last_u = 0;                     // unit 0 holds the start itself: no check there
    uint64_t w = (((uint64_t)U[0] << 32) | U[1]) << o;
    uint32_t valid = 64 - o, next = 2;
    while (pos < HD_SPAN_BITS) {
        const uint32_t u = pos >> 5;
        if (u != last_u) {
            const uint32_t c = chk[u];
            if ((c & 31u) == (pos & 31u)) return (((ref >> 4) - (c >> 5) + cnt) << 4) | (ref & 15u);
            last_u = u;
        }
        const uint32_t len = s_lut[(uint32_t)(w >> (64 - GLC_HD_MAX_LEN))] >> 8;
        w <<= len; pos += len; valid -= len; cnt++;
        if (valid <= 32 && next <= HD_SPAN) { w |= (uint64_t)U[next] << (32 - valid); valid += 32; next++; }
    }
    return (cnt << 4) | (pos - HD_SPAN_BITS);
}

// The span functions of a workgroup's 256 spans (units staged in s_u, table in s_lut), scanned inclusively across the
// lanes (Hillis-Steele, composition B(A(.))).  Returns which half of s_tab holds the result; every lane calls it.
__device__ __forceinline__ int hd_span_scan(const uint32_t *s_u, const uint16_t *s_lut, uint16_t *s_chk,
                                            uint32_t (*s_tab)[HD_LANES][HD_NOFF])
{
    const uint32_t tid = threadIdx.x;
    const uint32_t *U = s_u + tid * HD_PITCH;
    uint16_t *chk = s_chk + tid * HD_CHK_PITCH;
    const uint32_t ref = hd_decode_ref(U, s_lut, chk);
    s_tab[0][tid][0] = ref;
#pragma unroll 1
    for (uint32_t o = 1; o < HD_NOFF; o++) s_tab[0][tid][o] = hd_decode_merge(U, s_lut, chk, ref, o);
    int src = 0;
    for (uint32_t d = 1; d < HD_LANES; d <<= 1) {
        __syncthreads();
        for (uint32_t o = 0; o < HD_NOFF; o++) {
            uint32_t r = s_tab[src][tid][o];
            if (tid >= d) {
                const uint32_t a = s_tab[src][tid - d][o];            // earlier part, applied first
                const uint32_t bb = s_tab[src][tid][a & 15];
                r = (((a >> 4) + (bb >> 4)) << 4) | (bb & 15);
            }
            s_tab[src ^ 1][tid][o] = r;
        }
        src ^= 1;
    }
    __syncthreads();
    return src;
}

// A lane's span decoded from bit o, its first symbol being out[base]; out[nsym] and beyond are not written.  Four symbols
// per dword store once the output index is 4-aligned (the bytes before that belong to the previous lane's dword and go
// out one by one, as does the tail).
__device__ __forceinline__ void hd_emit_span(const uint32_t *U, const uint16_t *s_lut, uint32_t o, uint8_t *__restrict__ out,
                                             size_t base, size_t nsym)
{
    uint32_t pos = o;
    uint64_t w = (((uint64_t)U[0] << 32) | U[1]) << o;
    uint32_t valid = 64 - o, next = 2, acc = 0;
    size_t idx = base;
    const bool al = (reinterpret_cast<size_t>(out) & 3) == 0;
    while (pos < HD_SPAN_BITS && idx < nsym) {
        const uint32_t e = s_lut[(uint32_t)(w >> (64 - GLC_HD_MAX_LEN))];
        const uint32_t len = e >> 8, k = (uint32_t)idx & 3u;
        acc |= (e & 0xFFu) << (8 * k);
        if (k == 3) {
            if (al && idx - base >= 3) *reinterpret_cast<uint32_t *>(out + idx - 3) = acc;
            else for (uint32_t q = (idx - base >= 3) ? 0u : 3u - (uint32_t)(idx - base); q < 4; q++) out[idx - 3 + q] = (uint8_t)(acc >> (8 * q));
            acc = 0;
        }
        idx++;
        w <<= len; pos += len; valid -= len;
        if (valid <= 32 && next <= HD_SPAN) { w |= (uint64_t)U[next] << (32 - valid); valid += 32; next++; }
    }
    {   // tail: the bytes of an unfinished dword
        const uint32_t k = (uint32_t)idx & 3u;                 // bytes [idx - k, idx) pending, but not before `base`
        const uint32_t have = (uint32_t)((idx - base) < k ? (idx - base) : k);
        for (uint32_t q = k - have; q < k; q++) out[idx - k + q] = (uint8_t)(acc >> (8 * q));
    }
}

} // namespace glc
