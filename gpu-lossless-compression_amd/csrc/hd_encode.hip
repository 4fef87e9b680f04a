// hd_encode.hip -- device encoder of the CUHD-shaped Huffman-only stream (include/glc_hd.h).  gfx950 / wave64.
//
// The reference encodes on the host (cuhd-icpp/encoder/src/llhuffman_encoder.cc:200-238); so does glcHdEncodeHost.  Here
// every step runs on the device, enqueued on the caller's stream, with no host wait:
//   k_hd_hist         byte histogram: 16-byte loads, LDS counters in 16 copies, one u64 atomic per bin per workgroup
//   k_hd_table        one workgroup restates glcHdBuildTable: rank sort, package-merge as rank merges, multiplicities
//                     pushed down the package references, canonical codes, the reference's 2048-entry decoder table
//   k_hd_enc_count    bits of every 4096-symbol tile (0xFFFFFFFF: a symbol of the tile has no usable code)
//   k_hd_enc_scan     one workgroup: u64 bit offset of every tile, verdict, *d_nunits; zeroes the units two tiles share
//   k_hd_enc_pack     merges each tile's codes into LDS words from bit (tile offset & 31); interior words are stored,
//                     the first and last word of a tile are ORed onto the units the scan zeroed
#include "glc_device.h"
#include "../../include/glc_hd.h"

namespace glc {

// ---------------------------------------------------------------------------------------------------------------------
// histogram
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HH_NT = 256;
constexpr int HH_COPIES = 16;                           // lane & 15: 4 lanes of a wave share a copy
constexpr int HH_PITCH = 257;                           // copy c starts c banks further on
constexpr uint32_t HH_MAX_WG = 2048;
constexpr size_t HH_MIN_WG_BYTES = 64 << 10;

__global__ __launch_bounds__(HH_NT) void k_hd_hist(const uint8_t *__restrict__ in, size_t nsym, size_t head, size_t nvec,
                                                   size_t vec_per_wg, unsigned long long *__restrict__ hist)
{
    // head: bytes before the first 16-byte aligned address (< 16); nvec aligned 16-byte vectors follow; the tail
    // (< 16 bytes) after them.  Workgroup g counts vectors [g * vec_per_wg, +vec_per_wg): < 2^29 bytes for nsym < 2^40,
    // so no u32 counter of a copy can wrap.
    __shared__ uint32_t s_h[HH_COPIES * HH_PITCH];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < HH_COPIES * HH_PITCH; i += HH_NT) s_h[i] = 0;
    __syncthreads();
    uint32_t *H = s_h + (tid & (HH_COPIES - 1)) * HH_PITCH;
    const size_t v0 = (size_t)blockIdx.x * vec_per_wg, v1 = min(nvec, v0 + vec_per_wg);
    const uint4 *V = reinterpret_cast<const uint4 *>(in + head);
    auto count4 = [&](uint32_t w) {
        atomicAdd(&H[w & 0xFFu], 1u);
        atomicAdd(&H[(w >> 8) & 0xFFu], 1u);
        atomicAdd(&H[(w >> 16) & 0xFFu], 1u);
        atomicAdd(&H[w >> 24], 1u);
    };
    size_t v = v0 + tid;
    for (; v + 3 * HH_NT < v1; v += 4 * HH_NT) {      // four loads in flight per lane
        uint4 q[4];
#pragma unroll
        for (int r = 0; r < 4; r++) q[r] = V[v + r * HH_NT];
#pragma unroll
        for (int r = 0; r < 4; r++) { count4(q[r].x); count4(q[r].y); count4(q[r].z); count4(q[r].w); }
    }
    for (; v < v1; v += HH_NT) { const uint4 q = V[v]; count4(q.x); count4(q.y); count4(q.z); count4(q.w); }
    if (blockIdx.x == 0) {                             // the unaligned head and tail bytes
        if (tid < head) atomicAdd(&H[in[tid]], 1u);
        const size_t t0 = head + nvec * 16;
        if (t0 + tid < nsym && tid < 16) atomicAdd(&H[in[t0 + tid]], 1u);
    }
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < HH_COPIES; k++) c += s_h[k * HH_PITCH + tid];
    if (c) atomicAdd(&hist[tid], (unsigned long long)c);
}

// ---------------------------------------------------------------------------------------------------------------------
// table: glcHdBuildTable (hd_decode.hip) restated for one workgroup of 512 lanes
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HT_NT = 512;
constexpr int HT_MAXI = 512;                            // items of a level: at most 2m - 1 = 511
constexpr int HT_LEVELS = GLC_HD_MAX_LEN;               // L0 .. L10
constexpr uint16_t HT_PKG = 0x8000;                     // item reference: package j = HT_PKG | j, else leaf index

__global__ __launch_bounds__(HT_NT) void k_hd_table(const unsigned long long *__restrict__ hist, uint8_t *__restrict__ lens,
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
    const uint32_t tid = threadIdx.x;
    if (tid < 256) { s_hist[tid] = hist[tid]; s_len[tid] = 0; }
    if (tid < GLC_HD_MAX_LEN + 2) s_cnt[tid] = 0;
    if (tid == 0) s_m = 0;
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
    if (tid < 256 && s_len[tid]) atomicAdd(&s_cnt[s_len[tid]], 1u);
    __syncthreads();
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
        lens[tid] = (uint8_t)l;
        codes[tid] = (uint16_t)code;
    }
    if (!table2048) return;
    __syncthreads();
    // decoder table {num_bits, symbol}[2048]: entry e belongs to the last code (in canonical order) whose span starts at
    // or before e, if e lies inside that span; entries no codeword reaches are {0, 0}
    uint32_t nc = 0;
    for (int b = 1; b <= GLC_HD_MAX_LEN; b++) nc += s_cnt[b];
    for (uint32_t q = tid; q < 1024; q += HT_NT) {      // two entries per word: little-endian {bits, sym, bits, sym}
        uint32_t word = 0;
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t e = 2 * q + h;
            uint32_t lo = 0, hi = nc;                   // first rank whose span starts past e
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_lo[mid] <= e) lo = mid + 1; else hi = mid; }
            if (lo) {
                const uint32_t rs = s_rsym[lo - 1], l = rs >> 8;
                if (e < s_lo[lo - 1] + (1u << (GLC_HD_MAX_LEN - l))) word |= ((l | ((rs & 0xFFu) << 8)) << (16 * h));
            }
        }
        table2048[q] = word;
    }
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
constexpr int HS_NT = 1024;
constexpr int HS_TPT = 16;                              // tiles per scan lane and pass

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

__global__ __launch_bounds__(HE_NT) void k_hd_enc_count(const uint8_t *__restrict__ in, size_t nsym, size_t ntiles,
                                                        const uint8_t *__restrict__ lens, const uint16_t *__restrict__ codes,
                                                        uint32_t *__restrict__ tile_bits)
{
    __shared__ uint32_t s_cl[256];
    __shared__ uint32_t s_tmp[HE_NT / WAVE + 1];
    he_load_table(lens, codes, s_cl);
    __syncthreads();
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = 0; k < HE_TPW; k++) {
        const size_t t = (size_t)blockIdx.x * HE_TPW + k;
        if (t >= ntiles) break;
        const size_t s0 = t * HE_TILE + (size_t)tid * HE_SPT;
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
        if (tid == 0) {
            uint32_t tot = 0;
#pragma unroll
            for (int i = 0; i < HE_NT / WAVE; i++) tot += s_tmp[i];
            tile_bits[t] = anybad ? HE_BAD : tot;
        }
    }
}

// ws: {verdict (u32), pad}; off: ntiles + 1 bit offsets
__global__ __launch_bounds__(HS_NT) void k_hd_enc_scan(const uint32_t *__restrict__ tile_bits, size_t ntiles,
                                                       unsigned long long *__restrict__ off, uint32_t *__restrict__ verdict,
                                                       uint32_t *__restrict__ units, size_t cap_units,
                                                       unsigned long long *__restrict__ d_nunits)
{
    __shared__ uint32_t s_tmp[HS_NT / WAVE + 1];
    const uint32_t tid = threadIdx.x;
    unsigned long long run = 0;
    int bad = 0;
    for (size_t base = 0; base < ntiles; base += (size_t)HS_NT * HS_TPT) {
        const size_t t0 = base + (size_t)tid * HS_TPT;
        uint32_t b[HS_TPT];
        if (t0 + HS_TPT <= ntiles) {
            const uint4 *p = reinterpret_cast<const uint4 *>(tile_bits + t0);
#pragma unroll
            for (int r = 0; r < HS_TPT / 4; r++) { const uint4 q = p[r]; b[4 * r] = q.x; b[4 * r + 1] = q.y; b[4 * r + 2] = q.z; b[4 * r + 3] = q.w; }
        } else {
#pragma unroll
            for (int r = 0; r < HS_TPT; r++) b[r] = t0 + r < ntiles ? tile_bits[t0 + r] : 0u;
        }
        uint32_t sum = 0;
        bool mybad = false;
#pragma unroll
        for (int r = 0; r < HS_TPT; r++) { mybad |= b[r] == HE_BAD; sum += b[r] == HE_BAD ? 0u : b[r]; }
        bad |= __syncthreads_or((int)mybad);
        uint32_t total = 0;                             // <= 16384 * 45056 < 2^30
        const uint32_t ex = block_excl_add<HS_NT>(sum, s_tmp, &total);
        unsigned long long o = run + ex;
#pragma unroll
        for (int r = 0; r < HS_TPT; r++) {
            if (t0 + r < ntiles) off[t0 + r] = o;
            o += b[r] == HE_BAD ? 0u : b[r];
        }
        run += total;
    }
    const unsigned long long nunits = (run + 31) / 32 + 1;
    const bool ok = !bad && nunits <= cap_units;
    if (tid == 0) {
        off[ntiles] = run;
        *verdict = ok ? 1u : 0u;
        *d_nunits = ok ? nunits : 0ull;
    }
    if (!ok) return;                                    // nothing is written to units
    // zero the units a tile boundary falls inside (they are ORed into by both tiles), and the pad unit.  Each lane re-reads
    // only the offsets it wrote itself.
    for (size_t base = 0; base < ntiles; base += (size_t)HS_NT * HS_TPT) {
        const size_t t0 = base + (size_t)tid * HS_TPT;
#pragma unroll
        for (int r = 0; r < HS_TPT; r++) {
            if (t0 + r < ntiles && t0 + r > 0) { const unsigned long long o = off[t0 + r]; if (o & 31u) units[o >> 5] = 0u; }
        }
    }
    if (tid == 0) {
        if (run & 31u) units[run >> 5] = 0u;            // the last data unit: zero bits after the last code
        units[nunits - 1] = 0u;                         // the pad unit
    }
}

__global__ __launch_bounds__(HE_NT) void k_hd_enc_pack(const uint8_t *__restrict__ in, size_t nsym, size_t ntiles,
                                                       const uint8_t *__restrict__ lens, const uint16_t *__restrict__ codes,
                                                       const unsigned long long *__restrict__ off,
                                                       const uint32_t *__restrict__ verdict, uint32_t *__restrict__ units)
{
    __shared__ uint32_t s_cl[256];
    __shared__ __attribute__((aligned(16))) uint32_t s_words[HE_MAXW];
    __shared__ uint32_t s_tmp[HE_NT / WAVE + 1];
    if (*verdict == 0u) return;                         // failure: no store at all
    he_load_table(lens, codes, s_cl);
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = 0; k < HE_TPW; k++) {
        const size_t t = (size_t)blockIdx.x * HE_TPW + k;
        if (t >= ntiles) break;
        const unsigned long long tb = off[t], te = off[t + 1];
        const uint32_t sh = (uint32_t)tb & 31u;
        __syncthreads();                                // the table is in place / the previous tile's words have been read
        const size_t s0 = t * HE_TILE + (size_t)tid * HE_SPT;
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
        // the count pass and this one read the same bytes; if they disagree (the input changed in between) nothing of
        // the tile is stored, so no unit outside [tb, te) can be touched
        const bool same = (unsigned long long)total == te - tb;
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
        if (!same) continue;
        // units [tb >> 5, + nw): a word the tile covers whole is stored; the first word when the tile starts inside it
        // and the last when the tile ends inside it are shared with the neighbours and ORed onto the scan's zeros
        uint32_t *dst = units + (tb >> 5);
        const bool end_part = ((sh + total) & 31u) != 0;
        for (uint32_t i = tid; i < nw; i += HE_NT) {
            const uint32_t v = s_words[i];
            if ((i == 0 && sh) || (i == nw - 1 && end_part)) { if (v) atomicOr(&dst[i], v); }
            else dst[i] = v;
        }
    }
}

struct HeLayout { size_t ntiles, o_bits, o_off, o_verdict, total; };

static HeLayout he_layout(size_t nsym)
{
    HeLayout L;
    L.ntiles = (nsym + HE_TILE - 1) / HE_TILE;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = (o + bytes + 255) & ~(size_t)255; return r; };
    L.o_bits = take(L.ntiles * 4 + 16);
    L.o_off = take((L.ntiles + 1) * 8);
    L.o_verdict = take(16);
    L.total = o;
    return L;
}

} // namespace glc

using namespace glc;

extern "C" {

size_t glcHdEncodeBound(size_t nsym) { return (GLC_HD_MAX_LEN * nsym + 31) / 32 + 1; }

size_t glcHdEncodeWorkBytes(size_t nsym) { return he_layout(nsym).total; }

int glcHdHistogramDevice(const unsigned char *d_in, size_t nsym, unsigned long long *d_hist, void *stream)
{
    if (!d_hist || (!d_in && nsym) || nsym >= (1ull << 40)) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_hist, 0, 256 * sizeof(unsigned long long), st) != hipSuccess) return 0;
    if (nsym == 0) return 1;
    size_t head = (16 - (reinterpret_cast<uintptr_t>(d_in) & 15)) & 15;
    if (head > nsym) head = nsym;
    const size_t nvec = (nsym - head) / 16;
    size_t nwg = (nsym + HH_MIN_WG_BYTES - 1) / HH_MIN_WG_BYTES;  // >= 1 here
    if (nwg > HH_MAX_WG) nwg = HH_MAX_WG;
    const size_t vpw = nvec ? (nvec + nwg - 1) / nwg : 1;
    hipLaunchKernelGGL(k_hd_hist, dim3((unsigned)nwg), dim3(HH_NT), 0, st, d_in, nsym, head, nvec, vpw, d_hist);
    return hipGetLastError() == hipSuccess ? 1 : 0;
}

int glcHdBuildTableDevice(const unsigned long long *d_hist, unsigned char *d_lens, unsigned short *d_codes,
                          unsigned char *d_table2048, void *stream)
{
    if (!d_hist || !d_lens || !d_codes) return 0;
    if (d_table2048 && (reinterpret_cast<uintptr_t>(d_table2048) & 3)) return 0;
    hipLaunchKernelGGL(k_hd_table, dim3(1), dim3(HT_NT), 0, (hipStream_t)stream, d_hist, d_lens, d_codes,
                       reinterpret_cast<uint32_t *>(d_table2048));
    return hipGetLastError() == hipSuccess ? 1 : 0;
}

int glcHdEncodeDevice(const unsigned char *d_in, size_t nsym, const unsigned char *d_lens, const unsigned short *d_codes,
                      unsigned int *d_units, size_t cap_units, unsigned long long *d_nunits, void *d_work, void *stream)
{
    if ((!d_in && nsym) || !d_lens || !d_codes || !d_units || !d_nunits || !d_work || nsym >= (1ull << 40)) return 0;
    if (reinterpret_cast<uintptr_t>(d_units) & 3) return 0;
    const HeLayout L = he_layout(nsym);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *W = (uint8_t *)d_work;
    uint32_t *bits = (uint32_t *)(W + L.o_bits), *verdict = (uint32_t *)(W + L.o_verdict);
    unsigned long long *off = (unsigned long long *)(W + L.o_off);
    const unsigned nwg = (unsigned)((L.ntiles + HE_TPW - 1) / HE_TPW);
    if (L.ntiles)
        hipLaunchKernelGGL(k_hd_enc_count, dim3(nwg), dim3(HE_NT), 0, st, d_in, nsym, L.ntiles, d_lens, d_codes, bits);
    hipLaunchKernelGGL(k_hd_enc_scan, dim3(1), dim3(HS_NT), 0, st, bits, L.ntiles, off, verdict, d_units, cap_units, d_nunits);
    if (L.ntiles)
        hipLaunchKernelGGL(k_hd_enc_pack, dim3(nwg), dim3(HE_NT), 0, st, d_in, nsym, L.ntiles, d_lens, d_codes, off, verdict,
                           d_units);
    return hipGetLastError() == hipSuccess ? 1 : 0;
}

} // extern "C"
