// container_internal.h -- shared by container.hip (kernels), container_api.cpp and segments_api.cpp (host side of
// include/glc_container.h: the container over a plan, and the plan-less segment calls): the CRC-32 algebra, the BWT container's
// layout and the plan hooks cudpp_api.cpp exports to it.
#pragma once
#include "../../include/cudpp.h"
#include "glc_internal.h"
#include "ans_coder.h"
#include "auto_rule.h"
#include "choose_rule.h"
#include "class_rule.h"
#include "filter_rule.h"

#include <functional>

namespace glc {

// ---------------------------------------------------------------------------
// CRC-32/IEEE, reflected (zlib.crc32).  A register r is a polynomial with x^0 in bit 31; "raw" CRCs below start from 0
// and are not complemented, so they are linear: raw(A || B) = shift(raw(A), |B|) ^ raw(B), where shift(r, k) = r * x^(8k)
// mod P is what feeding k zero bytes does.  The standard CRC is raw(M) ^ shift(~0, |M|) ^ ~0, and two standard CRCs
// combine as crc(A || B) = shift(crc(A), |B|) ^ crc(B) (zlib's crc32_combine).
// ---------------------------------------------------------------------------
constexpr uint32_t CRC_POLY = 0xEDB88320u;

__host__ __device__ constexpr uint32_t crc_multmodp(uint32_t a, uint32_t b)
{   // a * b mod P, branch-free: 32 steps whatever a is
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= (0u - ((a >> (31 - i)) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & CRC_POLY);
    }
    return p;
}

struct CrcX2n { uint32_t v[32]; };                             // x^(2^k) mod P
constexpr CrcX2n crc_make_x2n()
{
    CrcX2n t{};
    uint32_t p = 1u << 30;                                     // x^1
    for (int k = 0; k < 32; k++) { t.v[k] = p; p = crc_multmodp(p, p); }
    return t;
}

// x^(8 n) mod P for a byte count n (zlib's x2nmodp(n, 3)); X2N is the table above, wherever it lives
template <class Tab>
__host__ __device__ constexpr uint32_t crc_x8n(unsigned long long n, const Tab &X2N)
{
    uint32_t p = 1u << 31;
    unsigned k = 3;
    while (n) {
        if (n & 1) p = crc_multmodp(X2N.v[k & 31], p);
        n >>= 1;
        k++;
    }
    return p;
}

// slice-by-16 tables of the raw register (T[0] = the bytewise table) and the four byte tables of "shift by 1024 bytes",
// one 64-lane row of 16-byte granules (k_crc_rows)
constexpr uint32_t CRC_ROW = 1024, CRC_TILE_ROWS = 16;
struct CrcTables { uint32_t t[16][256]; uint32_t row[4][256]; };
constexpr CrcTables crc_make_tables()
{
    CrcTables T{};
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((0u - (c & 1u)) & CRC_POLY);
        T.t[0][i] = c;
    }
    for (int j = 1; j < 16; j++)
        for (uint32_t i = 0; i < 256; i++) T.t[j][i] = (T.t[j - 1][i] >> 8) ^ T.t[0][T.t[j - 1][i] & 0xFF];
    const CrcX2n X = crc_make_x2n();
    const uint32_t sh = crc_x8n(CRC_ROW, X);
    for (int k = 0; k < 4; k++)
        for (uint32_t i = 0; i < 256; i++) T.row[k][i] = crc_multmodp(sh, i << (8 * k));
    return T;
}

uint32_t crc32_host(const void *data, size_t len, uint32_t crc = 0);     // standard CRC, continuing from `crc`

// CRC of `count` device segments [base + off[i], + len[i]) into d_crc[i].  base may be null with absolute addresses in off.
hipError_t crc32_segments(hipStream_t st, const uint8_t *base, const unsigned long long *d_off,
                          const unsigned long long *d_len, uint32_t count, uint32_t *d_crc);

// byte-plane shuffle (shuffle.hip): out[j q + i] = in[i elem + j] over the q = len / elem whole elements of a segment, the
// last len % elem bytes in place; elem 2, 4 or 8; in and out must not overlap.  The batched form takes one offset per
// segment for both bases.
hipError_t shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, bool inverse);
hipError_t shuffle_segments(hipStream_t st, const uint8_t *inBase, uint8_t *outBase, const unsigned long long *d_off,
                            const unsigned long long *d_len, uint32_t count, uint32_t elem, bool inverse);
// the shuffle of the differences of neighbouring elements, restarting every 2048 elements, and its inverse (delta.hip); one
// segment, the same rules
hipError_t delta_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, bool inverse);
// range forms of the two inverses: `in` is a filtered segment with plane stride q; elements [first, first + count) of what the
// whole-segment inverse would produce go to out[0 .. count * elem).  first + count <= q; the delta form wants first % 2048 == 0.
// Loads touch only the aligned 16-byte granules that hold a byte of one of the elem plane runs [j q + first, + count).
hipError_t unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                  unsigned long long first, unsigned long long count);
hipError_t undelta_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                          unsigned long long first, unsigned long long count);
// the lagged, folded delta + shuffle and its inverses (lag.hip): the predecessor is `lag` elements back (1..16), the difference's
// sign folded into bit 0 where fold = 1; the rules of the delta forms, which (lag, fold) = (1, 0) is handed to
hipError_t lag_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, uint32_t lag,
                              uint32_t fold, bool inverse);
hipError_t unlag_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                        uint32_t lag, uint32_t fold, unsigned long long first, unsigned long long count);
// the 2-D predictor + shuffle and its inverses (grid.hip): the delta at (1, fold) over the differences to the element `width`
// places back, the row above, within bands of ct_grid_period(width) elements; the rules of the delta forms, the range form's
// `first` a multiple of the period
hipError_t grid_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, uint32_t width,
                               uint32_t fold, bool inverse);
hipError_t ungrid_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                         uint32_t width, uint32_t fold, unsigned long long first, unsigned long long count);
// k_grid_vsum's walk with the caller's (W, P): every element at P-relative place W or beyond gains the element W places back, in
// place over `count` elements of v at `out`, the first of them the first of a band.  grid.hip calls it with (width, period),
// vol.hip with (plane, slab)
hipError_t grid_vsum_device(hipStream_t st, uint8_t *out, unsigned long long count, uint32_t elem, uint32_t W, uint32_t P);
// the 3-D predictor + shuffle and its inverses (vol.hip): the 2-D predictor over the differences to the element `plane` places
// back, the plane behind, within slabs of ct_vol_slab(width, plane) elements; the rules of the grid forms, the range form's
// `first` a multiple of the slab
hipError_t vol_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, uint32_t width,
                              uint32_t plane, uint32_t fold, bool inverse);
hipError_t unvol_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                        uint32_t width, uint32_t plane, uint32_t fold, unsigned long long first, unsigned long long count);
// the byte predictor and its inverses (byte_delta.hip): one-byte elements, the predecessor `lag` bytes back (1..16) over the
// differences to the byte `stride` back (0 = none, else 2..65536: the row above) within bands of ct_grid_period(stride) bytes; no
// planes, no fold: out has the length and the positions of in.  The range form gives bytes [first, first + count) of the inverse of
// the len bytes at `in`; `first` a multiple of ct_byte_step(stride)
hipError_t byte_delta_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t lag, uint32_t stride, bool inverse);
hipError_t unbyte_delta_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t lag, uint32_t stride,
                                     unsigned long long first, unsigned long long count);

// Carves typed arrays out of one allocation.  The same sequence of calls runs twice: on a null base it measures (bytes()), on
// the allocation it places, so the size and the pointers cannot disagree.
struct Carver {
    uint8_t *base;
    size_t off = 0;
    explicit Carver(void *b = nullptr) : base(static_cast<uint8_t *>(b)) {}
    template <class T> T *take(size_t count) { T *p = reinterpret_cast<T *>(base + off); off += count * sizeof(T); return base ? p : nullptr; }
    void round(size_t a) { off = (off + a - 1) & ~(a - 1); }      // the offset (the base is at least as aligned)
    void align(size_t a)                                          // the address; measuring counts the worst case
    {
        off = base ? (size_t)(((reinterpret_cast<uintptr_t>(base) + off + a - 1) & ~(uintptr_t)(a - 1)) - reinterpret_cast<uintptr_t>(base)) : off + a;
    }
    size_t bytes() const { return off; }
};

// the sparse passes (sparse.hip).  Segment i is `data` + data_off[i], min(data_len[i], max_len) bytes, cut into chunks of 64; its
// mask (bit c % 32 of word c / 32 = chunk c is kept, i.e. not all fill[i] & 255) is at mask + (mask_off ? mask_off[i] : i *
// mask_stride) words, its kept chunks K at kept + kept_off[i].  Either base may be null with absolute addresses in the offsets.
// skip (optional): segments whose entry is non-zero are left alone.  Everything only enqueues on `st`.
constexpr uint32_t SP_CHUNK = 64;
__host__ __device__ inline uint32_t sp_mask_words(uint32_t len) { return ((len + SP_CHUNK - 1) / SP_CHUNK + 31) / 32; }
struct SpSegs {
    uint8_t *data; const unsigned long long *data_off, *data_len;
    uint8_t *kept; const unsigned long long *kept_off;
    const uint32_t *fill;
    uint32_t *mask; const unsigned long long *mask_off; uint32_t mask_stride;
    const uint32_t *skip;
    uint32_t count, max_len;
};
hipError_t sparse_mask(hipStream_t st, const SpSegs &g);                                  // data -> mask
hipError_t sparse_count(hipStream_t st, const SpSegs &g, unsigned long long *d_klen);     // mask -> bytes of K
hipError_t sparse_compact(hipStream_t st, const SpSegs &g);                               // data, mask -> K
hipError_t sparse_join(hipStream_t st, const SpSegs &g);                                  // K, mask, fill -> data

// the dedup passes (dedup.hip; the hash and the rule are defined in INTEGRATION.md 4b).  The segments are the blocks of one frame
// in order: segment i is data + data_off[i], min(data_len[i], max_len) bytes, cut into chunks of 512; chunk c of it has the id
// i * nch + c, nch = ceil(max_len / 512).  hash[id] and the table (slots, a power of two >= 2 * count * nch, plus one slot for the
// key that equals the empty mark) are scratch of dedup_map; src[id] = the id of the chunk's source, or id itself for a kept chunk.
// data may be null with absolute addresses in data_off.  Everything only enqueues on `st`.
constexpr uint32_t DD_CHUNK = 512, DD_MAX_LEN = 1u << 20;
constexpr size_t DD_MAX_CHUNKS = (size_t)1 << 30;
struct DdSlot { uint64_t key; uint32_t id, pad; };
struct DdSegs {
    uint8_t *data; const unsigned long long *data_off, *data_len;
    uint64_t *hash; DdSlot *table; uint32_t slots;
    uint32_t *src;
    uint32_t count, max_len, nch;
};
size_t dedup_slots(size_t chunks);
hipError_t dedup_map(hipStream_t st, const DdSegs &g);       // data -> src (the writer's rule: the smallest id with equal hash, verified)
// src -> data, in place: a chunk whose entry is smaller than its id and names a chunk of its own length is copied from there;
// every other entry is skipped.  Nothing is read or written outside the segments.
// segments [first, first + count) only (count 0: all of them from `first` on); sources may lie in any segment
hipError_t dedup_fill(hipStream_t st, const DdSegs &g, uint32_t first = 0, uint32_t count = 0);

// the zero-run passes (zrun.hip; the split is defined in INTEGRATION.md 4b).  Segment i is x + x_off[i], min(x_len[i], max_len)
// bytes, cut into tiles of 256; A (the non-zero bytes and one 0 per run of zeros, a run ending at a tile edge) is at a + a_off[i],
// B (run length - 1 per run) at b + b_off[i], their byte counts in a_len[i] / b_len[i].  Any base may be null with absolute
// addresses in the offsets.  skip (optional): segments whose entry is non-zero are left alone.  Everything only enqueues on `st`.
constexpr uint32_t ZR_TILE = 256, ZR_MAX_LEN = 1u << 20;
struct ZrSegs {
    uint8_t *x; const unsigned long long *x_off, *x_len;
    uint8_t *a; const unsigned long long *a_off; unsigned long long *a_len;
    uint8_t *b; const unsigned long long *b_off; unsigned long long *b_len;
    const uint32_t *skip;
    uint32_t count, max_len;
};
hipError_t zrun_split(hipStream_t st, const ZrSegs &g);      // x -> A, B, a_len, b_len
// A, B (a_len / b_len are read, clamped to max_len) -> x.  Tolerant: a zero of A beyond B's end is a run of one, nothing is read
// outside A or B and nothing written outside the segment, whatever the streams hold
hipError_t zrun_join(hipStream_t st, const ZrSegs &g);

// the rANS passes (ans.hip; the coder is defined in INTEGRATION.md 4b).  Segment i is data + data_off[i], min(data_len[i], max_len)
// bytes (max_len <= ANS_MAX_LEN), cut into chunks of ANS_CHUNK; its byte counts are hist[i][256], its table (ans_tables makes it
// from the counts: 256 packed (q, cum, divisor shift), 256 divisor multipliers, 4096 slot -> symbol bytes) the ANS_TAB_BYTES at
// tab + i * ANS_TAB_BYTES, 16-byte aligned.  data may be null with absolute addresses in data_off.  skip (optional): segments
// whose entry is non-zero are left alone.  Everything only enqueues on `st`.
constexpr uint32_t ANS_TAB_BYTES = 2048 + ANS_M;
struct AnsSegs {
    uint8_t *data; const unsigned long long *data_off, *data_len;
    const uint32_t *hist; uint8_t *tab;
    const uint32_t *skip;
    uint32_t count, max_len;
};
struct AnsScratch {                                        // the encoder's: chunk c of segment i is slot i * nch_max + c
    uint16_t *units;                                       // [slots][ANS_CHUNK], a slot filled from its back
    uint32_t *states, *counts;                             // [slots][64]; [slots] units of the chunk
    uint32_t nch_max;                                      // ans_chunks(max_len)
};
// the words of a segment's record from its chunks' counts (counts clamped to a chunk's symbols)
__host__ __device__ inline unsigned long long ans_words_of(const uint32_t *counts, uint32_t nch)
{
    unsigned long long w = nch;
    for (uint32_t c = 0; c < nch; c++) w += ANS_LANES + ((counts[c] < ANS_CHUNK ? counts[c] : ANS_CHUNK) + 1) / 2;
    return w;
}
hipError_t ans_tables(hipStream_t st, const AnsSegs &g);                                   // hist -> tab
hipError_t ans_encode(hipStream_t st, const AnsSegs &g, const AnsScratch &sc);             // data, tab -> scratch
hipError_t ans_words(hipStream_t st, const AnsSegs &g, const AnsScratch &sc, unsigned long long *words);   // scratch -> record words
// scratch -> the record of segment i at rec_base + rec_off[i] (words); a record that would end past cap_words is not written
hipError_t ans_place(hipStream_t st, const AnsSegs &g, const AnsScratch &sc, uint32_t *rec_base, const unsigned long long *rec_off,
                     unsigned long long cap_words);
// records (rec_len[i] words each; null: rec_off[i + 1] - rec_off[i]), tab -> data.  Tolerant: a unit beyond a chunk's count or the
// record's end is 0, nothing is read outside the record and nothing written outside the segment, whatever the record holds
hipError_t ans_decode(hipStream_t st, const AnsSegs &g, const uint32_t *rec_base, const unsigned long long *rec_off,
                      const unsigned long long *rec_len);

// ---------------------------------------------------------------------------
// layout (little-endian; every section 8-byte aligned)
// ---------------------------------------------------------------------------
constexpr uint32_t CT_MAGIC_STREAM = 0x42434C47u;   // "GLCB"
constexpr uint32_t CT_MAGIC_FRAME  = 0x46434C47u;   // "GLCF"
constexpr uint32_t CT_MAGIC_END    = 0x45434C47u;   // "GLCE"
constexpr uint32_t CT_VERSION = 1, CT_VERSION_SHUFFLE = 2;   // 2: header word 3 = the shuffle's element size (2, 4, 8)
constexpr uint32_t CT_VERSION_CODEC = 3;                     // 3: kind 2 is legal; header word 3 = element size or 0 (no filter)
constexpr uint32_t CT_VERSION_DELTA = 4;                     // 4: version 3 with flags in the upper half of the version dword
constexpr uint32_t CT_FLAG_DELTA = 1;                        //    bit 0 (the only one): the filter is delta + shuffle; elem 2, 4 or 8
constexpr uint32_t CT_VERSION_SPARSE = 5;                    // 5: kind 3 is legal; flags 0 (elem 0, 2, 4, 8) or the delta flag (elem 2, 4, 8)
constexpr uint32_t CT_VERSION_RUNS = 6;                      // 6: kinds 0, 1, 2 and 4 are legal (not 3); the same triples as version 5
constexpr uint32_t CT_VERSION_ANS = 7;                       // 7: kinds 0, 1, 2 and 5 are legal (not 3, not 4); the same triples as version 5
constexpr uint32_t CT_VERSION_AUTO = 8;                      // 8: kinds 0, 1, 2, 3 and 5 are legal (not 4); the same triples as version 5
constexpr uint32_t CT_VERSION_DEDUP = 9;                     // 9: kinds 0, 1, 2 and 6 are legal (not 3, 4, 5); the same triples as version 5
// 10: version 8's kinds; the stream header's triple is (10, 0, 0) and every FRAME header's word 3 names that frame's filter,
// elem | flags << 16 (elem 0, 2, 4 or 8; flags 0 or the delta flag, which needs an elem)
constexpr uint32_t CT_VERSION_FILTER = 10;
// 11: version 8's stream (its kinds, frame word 0) behind the lagged, folded delta of lag.hip: elem 2, 4 or 8 and flags
// 1 | fold << 1 | (lag - 1) << 8 with the fold bit or the lag field non-zero (what flags 1 would say, version 8 says)
constexpr uint32_t CT_VERSION_LAG = 11;
constexpr uint32_t CT_FLAG_FOLD = 2, CT_LAG_SHIFT = 8, CT_LAG_MASK = 15u << CT_LAG_SHIFT;
__host__ __device__ inline bool ct_lag_flags_legal(uint32_t flags)
{
    return (flags & CT_FLAG_DELTA) && !(flags & ~(CT_FLAG_DELTA | CT_FLAG_FOLD | CT_LAG_MASK)) && (flags & (CT_FLAG_FOLD | CT_LAG_MASK));
}
// 12: version 8's stream behind the 2-D predictor of grid.hip: flags 1 | fold << 1 | 4 (bit 2 the grid flag, the lag field 0, no
// other bit) and the header's word 3 elem | width << 8 with elem 2, 4 or 8 and the row width 2..65536.  Word 3 is split under this
// version only: under every other it is the element size, whole
constexpr uint32_t CT_VERSION_GRID = 12;
constexpr uint32_t CT_FLAG_GRID = 4, CT_GRID_MIN_WIDTH = 2, CT_GRID_MAX_WIDTH = 65536, CT_WIDTH_SHIFT = 8;
__host__ __device__ inline bool ct_grid_width_ok(uint32_t width) { return width >= CT_GRID_MIN_WIDTH && width <= CT_GRID_MAX_WIDTH; }
// the period of the predictor: the row above is subtracted only inside a band of this many elements (about 32 rows, whole runs)
__host__ __device__ inline uint32_t ct_grid_period(uint32_t width) { return 2048u * ((width + 63) / 64); }
__host__ __device__ inline bool ct_grid_flags_legal(uint32_t flags) { return (flags & ~CT_FLAG_FOLD) == (CT_FLAG_DELTA | CT_FLAG_GRID); }
// 13: version 10 whose frame word may also name the lagged, folded delta: elem | flags << 16 with flags 0, 1, or a value that
// ct_lag_flags_legal() accepts (1 | fold << 1 | (lag - 1) << 8) with elem 2, 4 or 8; the stream header's triple is (13, 0, 0)
constexpr uint32_t CT_VERSION_FILTER_LAG = 13;
// 14: version 13 whose frame word may also name the 2-D predictor: a word with bit 31 set is elem | width << 8 | fold << 30 | 1 << 31
// (version 12's header word 3 with the fold in bit 30 -- elem 2, 4 or 8, width 2..65536, bits 25..29 zero); under version 13 every
// such word is illegal, so the two families cannot collide.  The stream header's triple is (14, 0, 0)
constexpr uint32_t CT_VERSION_FILTER_GRID = 14;
constexpr uint32_t CT_WORD_GRID = 1u << 31, CT_WORD_GRID_FOLD = 1u << 30, CT_WORD_GRID_WIDTH = 0x1FFFFu << CT_WIDTH_SHIFT;
// 15: version 8's stream (its kinds, frame word 0) behind the byte predictor of byte_delta.hip, for one-byte elements: flags
// 1 | (stride ? 4 : 0) | (lag - 1) << 8 (no fold bit: the fold permutes byte values) and the header's word 3 1 | stride << 8 with
// the row stride 0 (none) or 2..65536 bytes.  (lag 1, stride 0) is legal here: no older version can say it of bytes
constexpr uint32_t CT_VERSION_BYTE = 15;
constexpr uint32_t CT_BYTE_MAX_LAG = 16;
__host__ __device__ inline bool ct_byte_lag_ok(uint32_t lag) { return lag >= 1 && lag <= CT_BYTE_MAX_LAG; }
__host__ __device__ inline bool ct_byte_stride_ok(uint32_t stride) { return stride == 0 || ct_grid_width_ok(stride); }
// what a range read of the byte predictor's inverse starts at a multiple of: the run, with a stride the band
__host__ __device__ inline uint32_t ct_byte_step(uint32_t stride) { return stride ? ct_grid_period(stride) : 2048u; }
__host__ __device__ inline bool ct_byte_legal(uint32_t flags, uint32_t word3)
{
    const uint32_t stride = word3 >> CT_WIDTH_SHIFT;
    return (word3 & 0xFFu) == 1 && ct_byte_stride_ok(stride) && (flags & CT_FLAG_DELTA) && !(flags & ~(CT_FLAG_DELTA | CT_FLAG_GRID | CT_LAG_MASK)) &&
           ((flags & CT_FLAG_GRID) != 0) == (stride != 0);
}
constexpr uint32_t CT_VERSION_MAX = CT_VERSION_BYTE;
// 16: version 14 whose frame word may also name the byte predictor: a word with bit 31 set and the low byte 1 is
// 1 | stride << 8 | (lag - 1) << 25 | 1 << 31 (stride 0 or 2..65536, lag 1..16, bits 29 and 30 zero); under version 14 every such
// word is illegal (its elem is 1), so the families cannot collide.  The stream header's triple is (16, 0, 0).  It is no entry of
// ct_kinds()'s table, which tools/byte_format_check.cpp pins: CtFormat::kinds() answers version 8's kinds for it
constexpr uint32_t CT_VERSION_FILTER_BYTE = 16;
constexpr uint32_t CT_WORD_BYTE_LAG_SHIFT = 25, CT_WORD_BYTE_LAG = 15u << CT_WORD_BYTE_LAG_SHIFT;
// 17: version 12's stream behind the 3-D predictor of vol.hip: flags 1 | fold << 1 | 4 | 8 (bit 3 the volume flag), word 3 as
// under version 12 and the header's word 7 the plane stride S in elements, width < S <= 2^24.  Under this version alone word 7 is
// not 0 and word 6 is the CRC-32 of words 0..5 followed by word 7.  Like 16 it is no entry of ct_kinds()'s table: CtFormat::kinds()
// answers version 8's kinds for it
constexpr uint32_t CT_VERSION_VOL = 17;
constexpr uint32_t CT_FLAG_VOL = 8, CT_VOL_MAX_PLANE = 1u << 24, CT_VOL_PLANES = 16;
__host__ __device__ inline bool ct_vol_plane_ok(uint32_t width, uint32_t plane) { return plane > width && plane <= CT_VOL_MAX_PLANE; }
// the slab of the predictor: the plane behind is subtracted only inside a slab of this many elements (about 16 planes, whole
// bands).  At most 2^28 + 2^21; the product is taken in 64 bits
__host__ __device__ inline uint32_t ct_vol_slab(uint32_t width, uint32_t plane)
{
    const unsigned long long P = ct_grid_period(width);
    return (uint32_t)(P * (((unsigned long long)CT_VOL_PLANES * plane + P - 1) / P));
}
__host__ __device__ inline bool ct_vol_legal(uint32_t flags, uint32_t word3, uint32_t word7)
{
    const uint32_t e = word3 & 0xFFu, w = word3 >> CT_WIDTH_SHIFT;
    return (flags & ~CT_FLAG_FOLD) == (CT_FLAG_DELTA | CT_FLAG_GRID | CT_FLAG_VOL) && (e == 2 || e == 4 || e == 8) && ct_grid_width_ok(w) &&
           ct_vol_plane_ok(w, word7);
}
// what a reading plan speaks beyond versions 1 to 4 (ct_walk's `reader`): its sparse mode reads version 5, its runs mode version 6,
// its rANS mode version 7, its auto mode version 8 (and, the sparse and rANS bits implied, versions 5 and 7), its dedup mode version 9,
// its filter-auto setting version 10, its delta-lag setting version 11, its grid setting version 12, its filter-lag setting
// version 13, its filter-grid setting version 14, its byte-delta setting version 15 and its filter-byte setting version 16 (each is
// only ever on with the auto mode, so that mode's bits come with it; filter-lag only with filter-auto, filter-grid only with
// filter-lag, filter-byte only with filter-grid); its volume setting version 17 (only ever on with the grid setting)
constexpr uint32_t CT_READS_SPARSE = 1, CT_READS_RUNS = 2, CT_READS_ANS = 4, CT_READS_AUTO = 8, CT_READS_DEDUP = 16, CT_READS_FILTER = 32;
constexpr uint32_t CT_READS_LAG = 64, CT_READS_GRID = 128, CT_READS_FILTER_LAG = 256, CT_READS_FILTER_GRID = 512;
constexpr uint32_t CT_READS_BYTE = 1024, CT_READS_FILTER_BYTE = 2048, CT_READS_VOL = 4096;
// the one description of a version's record kinds: bit k = kind k is legal under it (0 = no such version)
__host__ __device__ inline uint32_t ct_kinds(uint32_t version)
{
    constexpr uint32_t K[CT_VERSION_MAX + 1] = {0, 0x03, 0x03, 0x07, 0x07, 0x0F, 0x17, 0x27, 0x2F, 0x47, 0x2F, 0x2F, 0x2F, 0x2F, 0x2F, 0x2F};
    return version <= CT_VERSION_MAX ? K[version] : 0u;
}
// A stream's format is its header's triple.  It says the two things that differ between streams: the filter a frame's bytes
// went through before its blocks were cut (none / shuffle / delta + shuffle over elements of `elem` bytes) and whether record
// kind 2 is legal.  The legal triples are one table in container_api.cpp, read by the writer and the reader alike (version 11's
// are a family of flags over it: the delta's lag and fold; version 12's a family of row widths, which ride in the element word).
struct CtFormat {
    uint32_t version = CT_VERSION, flags = 0, elem = 0;
    uint32_t width = 0;                                       // the 2-D predictor's row width: 0 but under version 12 and in a grid FRAME's format under versions 14 and 16
    uint32_t plane = 0;                                       // the 3-D predictor's plane stride: 0 but under version 17
    __host__ __device__ bool filtered() const { return elem != 0; }
    __host__ __device__ bool delta() const { return (flags & CT_FLAG_DELTA) != 0; }
    // the delta's lag and fold: (1, 0) below version 11; under version 13 a FRAME's format (ct_frame_format) carries them
    __host__ __device__ bool frame_filters() const { return version == CT_VERSION_FILTER || version == CT_VERSION_FILTER_LAG || version == CT_VERSION_FILTER_GRID || version == CT_VERSION_FILTER_BYTE; }
    // the byte predictor: version 15's streams, and under version 16 the format of a frame whose word names it (no other frame
    // has elem 1); elem is 1, `width` the row stride in bytes (0 = none), the lag in the flags
    __host__ __device__ bool bytes() const { return version == CT_VERSION_BYTE || (version == CT_VERSION_FILTER_BYTE && elem == 1); }
    __host__ __device__ bool lag_flags() const { return version == CT_VERSION_LAG || version == CT_VERSION_FILTER_LAG || version == CT_VERSION_FILTER_GRID || version == CT_VERSION_FILTER_BYTE || bytes(); }
    __host__ __device__ uint32_t lag() const { return lag_flags() ? ((flags & CT_LAG_MASK) >> CT_LAG_SHIFT) + 1 : 1u; }
    __host__ __device__ uint32_t fold() const { return (lag_flags() || version == CT_VERSION_GRID || version == CT_VERSION_VOL) && (flags & CT_FLAG_FOLD) ? 1u : 0u; }
    // the 2-D predictor: version 12's streams, and under versions 14 and 16 the format of a frame whose word names it
    __host__ __device__ bool grid() const { return version == CT_VERSION_GRID || (version == CT_VERSION_FILTER_GRID && width != 0) || (version == CT_VERSION_FILTER_BYTE && width != 0 && elem != 1); }
    // the 3-D predictor: version 17's streams (grid() is false of them: whoever asks both asks this first)
    __host__ __device__ bool vol() const { return version == CT_VERSION_VOL; }
    // the stream header's word 3: the element size, under versions 12 and 17 with the row width above it
    __host__ __device__ uint32_t word3() const { return elem | width << CT_WIDTH_SHIFT; }
    __host__ __device__ uint32_t kinds() const { return ct_kinds(version == CT_VERSION_FILTER_BYTE || version == CT_VERSION_VOL ? CT_VERSION_AUTO : version); }      // (version 6: all but 3; 7: all but 3 and 4; 8: all but 4; 16, 17: version 8's)
    __host__ __device__ bool kind2_legal() const { return (kinds() >> 2 & 1u) != 0; }
    __host__ __device__ bool kind3_legal() const { return (kinds() >> 3 & 1u) != 0; }
    __host__ __device__ bool kind4_legal() const { return (kinds() >> 4 & 1u) != 0; }
    __host__ __device__ bool kind5_legal() const { return (kinds() >> 5 & 1u) != 0; }
    __host__ __device__ bool kind6_legal() const { return (kinds() >> 6 & 1u) != 0; }
    // the CT_READS_* bit a plan must have to speak this version (0: every plan does)
    __host__ __device__ uint32_t reads() const
    {
        return version == CT_VERSION_SPARSE ? CT_READS_SPARSE : version == CT_VERSION_RUNS ? CT_READS_RUNS :
               version == CT_VERSION_ANS ? CT_READS_ANS : version == CT_VERSION_AUTO ? CT_READS_AUTO :
               version == CT_VERSION_DEDUP ? CT_READS_DEDUP : version == CT_VERSION_FILTER ? CT_READS_FILTER :
               version == CT_VERSION_LAG ? CT_READS_LAG : version == CT_VERSION_GRID ? CT_READS_GRID :
               version == CT_VERSION_FILTER_LAG ? CT_READS_FILTER_LAG : version == CT_VERSION_FILTER_GRID ? CT_READS_FILTER_GRID :
               version == CT_VERSION_BYTE ? CT_READS_BYTE : version == CT_VERSION_FILTER_BYTE ? CT_READS_FILTER_BYTE :
               version == CT_VERSION_VOL ? CT_READS_VOL : 0u;
    }
};
// a frame header's word 3.  Versions 1 to 9, 11, 12 and 15 keep it 0; under versions 10, 13, 14 and 16 it is the frame's filter.  ct_frame_word_legal() is the
// header's range check on it, ct_frame_format() the format whose filter a frame with a legal word went through: the stream's
// below version 10, the word's under it
__host__ __device__ inline uint32_t ct_frame_word(const CtFormat &f)
{
    if (f.version == CT_VERSION_FILTER_BYTE && f.elem == 1)   // version 16's byte word
        return 1u | f.width << CT_WIDTH_SHIFT | (f.lag() - 1) << CT_WORD_BYTE_LAG_SHIFT | CT_WORD_GRID;
    if (f.width) return f.elem | f.width << CT_WIDTH_SHIFT | (f.fold() ? CT_WORD_GRID_FOLD : 0u) | CT_WORD_GRID;
    return f.elem | (f.flags << 16);
}
__host__ __device__ inline bool ct_frame_word_legal(const CtFormat &stream, uint32_t word)
{
    if (!stream.frame_filters()) return word == 0;
    if (word & CT_WORD_GRID) {                                // version 14's grid word, version 16's byte word
        const uint32_t e = word & 0xFFu;
        if (stream.version == CT_VERSION_FILTER_BYTE && e == 1)
            return !(word & ~(0xFFu | CT_WORD_GRID_WIDTH | CT_WORD_BYTE_LAG | CT_WORD_GRID)) && ct_byte_stride_ok((word & CT_WORD_GRID_WIDTH) >> CT_WIDTH_SHIFT);
        return (stream.version == CT_VERSION_FILTER_GRID || stream.version == CT_VERSION_FILTER_BYTE) && !(word & ~(0xFFu | CT_WORD_GRID_WIDTH | CT_WORD_GRID_FOLD | CT_WORD_GRID)) &&
               (e == 2 || e == 4 || e == 8) && ct_grid_width_ok((word & CT_WORD_GRID_WIDTH) >> CT_WIDTH_SHIFT);
    }
    const uint32_t elem = word & 0xFFFFu, flags = word >> 16;
    if (elem == 0) return flags == 0;
    if (elem != 2 && elem != 4 && elem != 8) return false;
    return flags <= CT_FLAG_DELTA || (stream.version != CT_VERSION_FILTER && ct_lag_flags_legal(flags));
}
__host__ __device__ inline CtFormat ct_frame_format(const CtFormat &stream, uint32_t word)
{
    CtFormat f = stream;
    if (!stream.frame_filters()) return f;
    if (word & CT_WORD_GRID) {                                // (legal under versions 14 and 16 alone: version 12's filter for this frame)
        if (stream.version == CT_VERSION_FILTER_BYTE && (word & 0xFFu) == 1) {     // (version 15's filter for this frame, its flags)
            f.elem = 1;
            f.width = (word & CT_WORD_GRID_WIDTH) >> CT_WIDTH_SHIFT;
            f.flags = CT_FLAG_DELTA | (f.width ? CT_FLAG_GRID : 0u) | ((word & CT_WORD_BYTE_LAG) >> CT_WORD_BYTE_LAG_SHIFT) << CT_LAG_SHIFT;
            return f;
        }
        f.elem = word & 0xFFu;
        f.width = (word & CT_WORD_GRID_WIDTH) >> CT_WIDTH_SHIFT;
        f.flags = CT_FLAG_DELTA | CT_FLAG_GRID | (word & CT_WORD_GRID_FOLD ? CT_FLAG_FOLD : 0u);
        return f;
    }
    f.elem = word & 0xFFFFu; f.flags = word >> 16;
    return f;
}
// a format's filter over one segment, or its inverse
inline hipError_t filter_device(hipStream_t st, const CtFormat &f, const uint8_t *in, uint8_t *out, unsigned long long len, bool inverse)
{
    if (f.bytes()) return byte_delta_device(st, in, out, len, f.lag(), f.width, inverse);
    if (f.vol()) return vol_shuffle_device(st, in, out, len, f.elem, f.width, f.plane, f.fold(), inverse);
    if (f.grid()) return grid_shuffle_device(st, in, out, len, f.elem, f.width, f.fold(), inverse);
    if (f.delta()) return lag_shuffle_device(st, in, out, len, f.elem, f.lag(), f.fold(), inverse);   // ((1, 0): delta.hip's kernels)
    return shuffle_device(st, in, out, len, f.elem, inverse);
}
constexpr uint32_t CT_HDR = 32, CT_FRAME_HDR = 32, CT_TRAILER = 16;
// the format rule: the legal (version, flags) pairs, lowest version first, and the element sizes each takes (bit e = elem e)
constexpr uint32_t CT_NO_FILTER = 1u << 0, CT_ELEMS = 1u << 2 | 1u << 4 | 1u << 8;
struct CtLegal { uint32_t version, flags, elems; };
constexpr uint32_t CT_NLEGAL = 15;
__host__ __device__ inline CtLegal ct_legal(uint32_t i)
{
    constexpr CtLegal L[CT_NLEGAL] = {
        {CT_VERSION, 0, CT_NO_FILTER}, {CT_VERSION_SHUFFLE, 0, CT_ELEMS}, {CT_VERSION_CODEC, 0, CT_NO_FILTER | CT_ELEMS},
        {CT_VERSION_DELTA, CT_FLAG_DELTA, CT_ELEMS}, {CT_VERSION_SPARSE, 0, CT_NO_FILTER | CT_ELEMS},
        {CT_VERSION_SPARSE, CT_FLAG_DELTA, CT_ELEMS}, {CT_VERSION_RUNS, 0, CT_NO_FILTER | CT_ELEMS},
        {CT_VERSION_RUNS, CT_FLAG_DELTA, CT_ELEMS}, {CT_VERSION_ANS, 0, CT_NO_FILTER | CT_ELEMS},
        {CT_VERSION_ANS, CT_FLAG_DELTA, CT_ELEMS}, {CT_VERSION_AUTO, 0, CT_NO_FILTER | CT_ELEMS},
        {CT_VERSION_AUTO, CT_FLAG_DELTA, CT_ELEMS}, {CT_VERSION_DEDUP, 0, CT_NO_FILTER | CT_ELEMS},
        {CT_VERSION_DEDUP, CT_FLAG_DELTA, CT_ELEMS}, {CT_VERSION_FILTER, 0, CT_NO_FILTER}};
    return L[i];
}
__host__ __device__ inline bool format_legal(const CtFormat &f)
{
    // (version 11 is a family of flags, not rows: every lag and fold over the three element sizes)
    if (f.version == CT_VERSION_LAG) return ct_lag_flags_legal(f.flags) && f.elem <= 8 && (CT_ELEMS >> f.elem & 1) && !f.width;
    // (so is version 12: either fold and every row width over the three element sizes)
    if (f.version == CT_VERSION_GRID) return ct_grid_flags_legal(f.flags) && f.elem <= 8 && (CT_ELEMS >> f.elem & 1) && ct_grid_width_ok(f.width);
    if (f.width) return false;
    for (uint32_t i = 0; i < CT_NLEGAL; i++) {
        const CtLegal l = ct_legal(i);
        if (l.version == f.version && l.flags == f.flags && f.elem <= 8 && (l.elems >> f.elem & 1)) return true;
    }
    return false;
}
constexpr uint32_t CT_KIND_HUFF = 0, CT_KIND_RAW = 1;
constexpr uint32_t CT_KIND_HUFF0 = 2;                        // order-0 Huffman record (hd_batch.hip), versions 3 and 4
constexpr uint32_t CT_KIND_SPARSE = 3;                       // sparse order-0 record (sparse.hip): mask, then the kind-2 stream of the kept chunks; version 5
constexpr uint32_t CT_KIND_RUNS = 4;                         // zero-run BWT record (zrun.hip): B's counts, then the kind-2 streams of A and B; version 6
constexpr uint32_t CT_KIND_ANS = 5;                          // rANS order-0 record (ans.hip): chunk unit counts, then every chunk's 64 states and units; version 7
constexpr uint32_t CT_KIND_DEDUP = 6;                        // dedup order-0 record (dedup.hip): mask, source ids of the elided chunks, then the kind-2 stream of the kept chunks; version 9
constexpr uint32_t CT_CODEC_BWT = 0, CT_CODEC_HUFF0 = 1;     // GlcContainerCodec
// CHOOSE: the writer gives each block to one of the two codecs (choose_rule.h) and cuts a frame wherever the choice changes.  It
// takes no mode (each belongs to one codec) and no filter (a filter is per frame, and the choice would be made on filtered bytes)
constexpr uint32_t CT_CODEC_CHOOSE = 4;                      // (2 and 3 stay refused: callers and tests have long used them as the bad value)
// the writer's mode: which record kinds beyond its codec's plain ones it may emit (3; 4; 5; 3 and 5; 6).  At most one is on, and
// each belongs to one codec: runs to the BWT codec, sparse, rANS, auto and dedup to the order-0 codec
enum CtMode : uint32_t { CT_MODE_PLAIN = 0, CT_MODE_SPARSE, CT_MODE_RUNS, CT_MODE_ANS, CT_MODE_AUTO, CT_MODE_DEDUP };
__host__ __device__ inline bool ct_mode_fits(CtMode mode, uint32_t codec)
{
    return mode == CT_MODE_PLAIN || codec == (mode == CT_MODE_RUNS ? CT_CODEC_BWT : CT_CODEC_HUFF0);   // (none fits CHOOSE)
}

// failure classes of glcContainerLastError (out[0])
enum CtWhat : uint32_t { CT_OK = 0, CT_STREAM_HEADER = 1, CT_FRAME_TABLE = 2, CT_RECORD_CRC = 3, CT_DECODED_CRC = 4,
                         CT_TRUNCATED = 5, CT_CAPACITY = 6 };

struct CtTables {                                    // word offsets of the sections of a frame's tables (from the tables' start)
    uint32_t nb, nsub;
    unsigned long long kind, bwt, crc_raw, crc_rec, hist, enc_off, pay_off, words;
};
__host__ __device__ inline CtTables ct_tables(uint32_t nb, uint32_t blk_len)
{
    CtTables t{};
    t.nb = nb;
    t.nsub = (blk_len + HUFF_BLOCK - 1) / HUFF_BLOCK;
    const unsigned long long a = nb + (nb & 1u), e = (unsigned long long)nb * t.nsub + (((unsigned long long)nb * t.nsub) & 1u);
    t.kind = 0; t.bwt = a; t.crc_raw = 2 * a; t.crc_rec = 3 * a; t.hist = 4 * a;
    t.enc_off = t.hist + 256ull * nb; t.pay_off = t.enc_off + e; t.words = t.pay_off + 2ull * (nb + 1);
    return t;
}
__host__ __device__ inline uint32_t ct_raw_words(uint32_t blk_len) { return (blk_len + 3) / 4; }
// the record rule: a block whose coded record of `words` words would not be smaller than its bytes is stored raw
__host__ __device__ inline bool ct_stored_raw(unsigned long long words, uint32_t blk_len) { return 4 * words >= blk_len; }
__host__ __device__ inline unsigned long long frame_bytes(uint32_t nb, uint32_t blk_len, unsigned long long payload_words)
{
    return CT_FRAME_HDR + 4 * ct_tables(nb, blk_len).words + 4 * (payload_words + (payload_words & 1));
}

// ---------------------------------------------------------------------------
// The walk over a stream's headers: stream header -> frame header -> frame_bytes(nb, bl, pw) -> next frame header -> trailer.
// One function for the host (the decoder's walk and the index of a host buffer or a file) and for the device (k_ct_index), so
// that all of them refuse the same streams with the same class and the same frame.  C: the CRC tables of the side that runs.
// ---------------------------------------------------------------------------
__host__ __device__ inline uint32_t crc32_bytes(const CrcTables &C, const void *data, size_t len)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    uint32_t r = ~0u;
    for (size_t i = 0; i < len; i++) r = C.t[0][(r ^ p[i]) & 255] ^ (r >> 8);
    return ~r;
}

// the reader's format: header words 1 (version, flags in the upper half) and 3 (elem; under version 12 elem | width << 8)
__host__ __device__ inline bool parse_format(const uint32_t h[8], CtFormat *f)
{
    f->version = h[1] & 0xFFFFu; f->flags = h[1] >> 16; f->elem = h[3]; f->width = 0;
    if (f->version == CT_VERSION_GRID) { f->elem = h[3] & 0xFFu; f->width = h[3] >> CT_WIDTH_SHIFT; }
    return format_legal(*f);
}

// a stream header's format: parse_format()'s, or version 13's one triple (13, 0, 0).  Version 13 is no row of ct_legal():
// format_legal() and parse_format() stay the rule of versions 1 to 12, which the checkers of versions 11 and 12 pin version by
// version (tools/lag_format_check.cpp, tools/grid_format_check.cpp); tools/filter_lag_rule_check.cpp pins this one
__host__ __device__ inline bool parse_stream_format(const uint32_t h[8], CtFormat *f)
{
    if (parse_format(h, f)) return true;
    return f->version == CT_VERSION_FILTER_LAG && f->flags == 0 && f->elem == 0 && f->width == 0;
}
// version 14's one triple (14, 0, 0) beside it, accepted the way 13 was: parse_stream_format() is pinned up to version 15 by
// tools/filter_lag_rule_check.cpp, so this is the function the readers call; tools/filter_grid_rule_check.cpp pins it
__host__ __device__ inline bool parse_header_format(const uint32_t h[8], CtFormat *f)
{
    if (parse_stream_format(h, f)) return true;
    return f->version == CT_VERSION_FILTER_GRID && f->flags == 0 && f->elem == 0 && f->width == 0;
}

// version 15's family beside it, accepted the way 13 and 14 were: parse_header_format() is pinned up to version 16 by
// tools/filter_grid_rule_check.cpp, so this is the function the readers call; tools/byte_format_check.cpp pins it.  Word 3 is
// split as under version 12: the element size 1 below the row stride
__host__ __device__ inline bool parse_container_format(const uint32_t h[8], CtFormat *f)
{
    if (parse_header_format(h, f)) return true;
    if (f->version != CT_VERSION_BYTE || !ct_byte_legal(f->flags, h[3])) return false;
    f->elem = 1; f->width = h[3] >> CT_WIDTH_SHIFT;
    return true;
}

// version 16's one triple (16, 0, 0) beside it, accepted the way 13, 14 and 15 were: parse_container_format() is pinned up to
// version 17 by tools/byte_format_check.cpp, so this is the function the readers call; tools/filter_byte_rule_check.cpp pins it
__host__ __device__ inline bool parse_frame_filter_format(const uint32_t h[8], CtFormat *f)
{
    if (parse_container_format(h, f)) return true;
    if (f->version != CT_VERSION_FILTER_BYTE || f->flags != 0 || h[3] != 0) return false;
    f->elem = 0; f->width = 0;
    return true;
}

// version 17's family beside it, accepted the way 13 to 16 were: parse_frame_filter_format() is pinned up to version 18 by
// tools/filter_byte_rule_check.cpp, so this is the function the readers call; tools/vol_format_check.cpp pins it.  Word 3 is
// split as under version 12, word 7 is the plane stride
__host__ __device__ inline bool parse_volume_format(const uint32_t h[8], CtFormat *f)
{
    f->plane = 0;
    if (parse_frame_filter_format(h, f)) return true;
    if (f->version != CT_VERSION_VOL || !ct_vol_legal(f->flags, h[3], h[7])) return false;
    f->elem = h[3] & 0xFFu; f->width = h[3] >> CT_WIDTH_SHIFT; f->plane = h[7];
    return true;
}

// a stream header's word 6: the CRC-32 of words 0..5, under version 17 of words 0..5 followed by word 7 (28 bytes), so that the
// plane stride is covered
template <class Crc>
__host__ __device__ inline uint32_t ct_header_crc(const uint32_t h[8], Crc crc)
{
    if ((h[1] & 0xFFFFu) != CT_VERSION_VOL) return crc(h, 24);
    const uint32_t t[7] = {h[0], h[1], h[2], h[3], h[4], h[5], h[7]};
    return crc(t, 28);
}

// the checks on a stream header; false = refused.  Word 7 is 0 under every version but 17
__host__ __device__ inline bool check_stream_header(const CrcTables &C, const uint32_t h[8], CtFormat *fmt, uint32_t *block_len,
                                                    unsigned long long *total)
{
    if (h[0] != CT_MAGIC_STREAM || ((h[1] & 0xFFFFu) != CT_VERSION_VOL && h[7] != 0)) return false;
    if (h[6] != ct_header_crc(h, [&](const uint32_t *w, size_t n) { return crc32_bytes(C, w, n); }) || !parse_volume_format(h, fmt)) return false;
    if (h[2] == 0 || h[2] > MAX_BLOCK_ELEMS) return false;
    *block_len = h[2];
    *total = (unsigned long long)h[4] | ((unsigned long long)h[5] << 32);
    return true;
}

// the range checks on a frame header, `left` output bytes still to come; false = refused
__host__ __device__ inline bool check_frame_header(const uint32_t h[8], const CtFormat &fmt, uint32_t block_len, unsigned long long left,
                                                   unsigned long long *pw)
{
    const uint32_t nb = h[1], bl = h[2];
    *pw = (unsigned long long)h[4] | ((unsigned long long)h[5] << 32);
    if (h[0] != CT_MAGIC_FRAME || !ct_frame_word_legal(fmt, h[3]) || h[7] != 0 || nb == 0 || bl == 0 || bl > block_len) return false;
    if ((nb > 1 && bl != block_len) || (unsigned long long)nb * bl > left) return false;
    return *pw <= (unsigned long long)nb * ct_raw_words(bl);
}

__host__ __device__ inline bool check_trailer(const CrcTables &C, const uint32_t t[4], uint32_t frames)
{
    return t[0] == CT_MAGIC_END && t[1] == frames && t[3] == crc32_bytes(C, t, 12);
}

struct CtFrameRef {                                        // a frame whose header has passed the walk's checks
    unsigned long long pos, out_off, pw;                   // where it starts in the stream; the output offset of its first byte
    uint32_t nb, bl;
    uint32_t filter, pad;                                  // its header's word 3: 0 below version 10, the frame's filter under it
};
// what a walk ends with beyond CtWhat: the plan's n is below a frame's blk_len; a callback stopped it (the reason is the caller's)
constexpr uint32_t CT_WALK_CONFIG = 0x100, CT_WALK_STOPPED = 0x101;
struct CtWalkEnd { uint32_t what; unsigned long long frame; };            // frame: the index a failure names (~0 = none)

// fetch(dst, pos, bytes, frame) -> bool brings 32 or 16 header bytes into dst; on_header(h, fmt, block_len, total),
// on_frame(fi, fh, ref) and on_trailer(tr, frames) -> bool see what has passed its checks.  `reader` (CT_READS_*) is the plan's
// sparse, runs, rANS and auto modes (a plan with all off is a version-4 reader), plan_n its block length.
template <class Fetch, class OnHeader, class OnFrame, class OnTrailer>
__host__ __device__ inline CtWalkEnd ct_walk(const CrcTables &C, unsigned long long len, uint32_t plan_n, uint32_t reader, Fetch fetch,
                                             OnHeader on_header, OnFrame on_frame, OnTrailer on_trailer)
{
    const unsigned long long none = ~0ull;
    if (len < CT_HDR + CT_TRAILER) return {CT_TRUNCATED, none};
    uint32_t hdr[8], block_len = 0;
    unsigned long long total = 0;
    CtFormat fmt;
    if (!fetch(hdr, 0ull, CT_HDR, none)) return {CT_WALK_STOPPED, none};
    if (!check_stream_header(C, hdr, &fmt, &block_len, &total)) return {CT_STREAM_HEADER, none};
    if (fmt.reads() && !(reader & fmt.reads())) return {CT_STREAM_HEADER, none};
    if (!on_header(hdr, fmt, block_len, total)) return {CT_WALK_STOPPED, none};
    unsigned long long pos = CT_HDR, done = 0;
    uint32_t fi = 0;
    while (done < total) {
        if (pos + CT_FRAME_HDR + CT_TRAILER > len) return {CT_TRUNCATED, fi};
        uint32_t fh[8];
        if (!fetch(fh, pos, CT_FRAME_HDR, (unsigned long long)fi)) return {CT_WALK_STOPPED, fi};
        CtFrameRef ref{pos, done, 0, fh[1], fh[2], fh[3], 0};
        if (!check_frame_header(fh, fmt, block_len, total - done, &ref.pw)) return {CT_FRAME_TABLE, fi};
        if (ref.bl > plan_n) return {CT_WALK_CONFIG, fi};
        const unsigned long long fb = frame_bytes(ref.nb, ref.bl, ref.pw);
        if (pos + fb + CT_TRAILER > len) return {CT_TRUNCATED, fi};
        if (!on_frame(fi, fh, ref)) return {CT_WALK_STOPPED, fi};
        pos += fb; done += (unsigned long long)ref.nb * ref.bl; fi++;
    }
    uint32_t tr[4];
    if (pos + CT_TRAILER > len) return {CT_TRUNCATED, fi};
    if (!fetch(tr, pos, CT_TRAILER, (unsigned long long)fi)) return {CT_WALK_STOPPED, fi};
    if (!check_trailer(C, tr, fi) || pos + CT_TRAILER != len) return {CT_STREAM_HEADER, fi};
    if (!on_trailer(tr, fi)) return {CT_WALK_STOPPED, fi};
    return {CT_OK, none};
}

// what k_ct_index leaves in front of its entries: how the walk ended, the frames it passed, the header and the trailer
struct CtIndexHead {
    uint32_t what, frames;
    unsigned long long frame;
    uint32_t hdr[8], trailer[4];
};
constexpr uint32_t CT_INDEX_FIRST = 1022;                  // entries the one readback brings along with the head (40 KiB in all)
// the walk over a container in device memory (8-byte aligned), one launch: head and up to `cap` entries into `scratch`
hipError_t ct_index_device(hipStream_t st, const uint8_t *in, unsigned long long len, uint32_t plan_n, uint32_t reader,
                           CtIndexHead *head, CtFrameRef *entries, unsigned long long cap);

// ---------------------------------------------------------------------------
// plan hooks (cudpp_api.cpp): the container path drives a COMPRESS plan through its internals
// ---------------------------------------------------------------------------
struct ContainerHooks {
    uint32_t *status = nullptr;                              // replaces the plan's status word for this call's encode
    const uint32_t *pack_only = nullptr;                     // blocks the packer writes (the Huffman ones)
    std::function<hipError_t(hipStream_t)> before_offsets;   // after the last k_huff_build, before the payload offsets
    std::function<hipError_t(hipStream_t)> after_pack;       // behind the packer, on the same stream
};
// glcCompressBatchCompact with the hooks above
CUDPPResult plan_compress_hooked(CUDPPHandle plan, CompressCall c, ContainerHooks &hk);
// 1 = a COMPRESS plan; n, rows, its stream, and the parity of its next compress call (which half of double-buffered scratch
// that call may reuse once the plan's own ordering lets it)
bool plan_info(CUDPPHandle plan, uint32_t *n, uint32_t *rows, hipStream_t *st, uint32_t *next_parity);
void plan_join(CUDPPHandle plan);                          // the plan's stream waits for its internal one
// the container settings of a COMPRESS plan's encoder (glcPlanSetContainer*): the filter's element size (0 = off), its delta
// mode (only ever on with the shuffle on), the codec (CT_CODEC_*) and the mode (only ever one that ct_mode_fits() the codec).
// The CHOOSE codec is only ever on with the shuffle off.  The set_*() are the whole rule of the public setters: false = refused,
// nothing changed.
inline bool shuffle_elem_ok(uint32_t elem) { return elem <= 8 && (CT_ELEMS >> elem & 1); }
struct CtSettings {
    uint32_t shuffle = 0; bool delta = false; uint32_t codec = CT_CODEC_BWT; CtMode mode = CT_MODE_PLAIN;
    // filter-auto: the writer picks every frame's filter itself (filter_rule.h) and writes version 10.  Only ever on with the order-0
    // codec, the auto mode on and the shuffle off; whatever ends one of the three switches it off
    bool filter_auto = false;
    // filter-lag: filter-auto also weighs the lagged, folded delta at the lag it finds per frame (lag_rule.h) and writes version
    // 13.  Only ever on with filter-auto on; whatever switches that off switches this off
    bool filter_lag = false;
    // filter-grid: filter-lag also weighs the 2-D predictor at the row width it finds per frame (grid_rule.h) and writes version
    // 14.  Only ever on with filter-lag on; whatever switches that off switches this off
    bool filter_grid = false;
    // filter-byte: filter-grid also weighs the byte predictor at the lag and the row stride it finds per frame (byte_rule.h) and
    // writes version 16.  Only ever on with filter-grid on; whatever switches that off switches this off
    bool filter_byte = false;
    void filter_keep()
    {
        if (mode != CT_MODE_AUTO) filter_auto = false;
        if (!filter_auto) filter_lag = false;
        if (!filter_lag) filter_grid = false;
        if (!filter_grid) filter_byte = false;
    }
    // delta-lag: the delta's predecessor is `lag` elements back and its sign is folded where fold = 1 (lag.hip; the writer writes
    // version 11).  Anything but (1, 0) is only ever on with the order-0 codec, the auto mode, the shuffle and the delta on and
    // filter-auto off; whatever ends one of them puts it back to (1, 0)
    uint32_t lag = 1, fold = 0;
    bool lag_on() const { return lag != 1 || fold != 0; }
    bool lag_fits() const { return codec == CT_CODEC_HUFF0 && mode == CT_MODE_AUTO && shuffle && delta && !filter_auto; }
    // grid: the delta is the 2-D predictor of row width grid_width (0 = off), its sign folded where grid_fold = 1 (grid.hip; the
    // writer writes version 12).  Only ever on with the lag's prerequisites and the lag itself at (1, 0); whatever ends one of
    // them puts it back to off
    uint32_t grid_width = 0, grid_fold = 0;
    bool grid_on() const { return grid_width != 0; }
    // volume: the 2-D predictor runs over the differences to the element vol_plane places back (0 = off; vol.hip; the writer
    // writes version 17).  Only ever on with the grid setting on at a width below it; whatever switches that off switches this off
    uint32_t vol_plane = 0;
    bool vol_on() const { return vol_plane != 0; }
    // byte-delta: every frame goes through the byte predictor at (byte_lag, byte_stride) (byte_delta.hip; the writer writes
    // version 15); byte_lag 0 = off.  Only ever on with the order-0 codec, the auto mode on, the shuffle off and filter-auto off;
    // a codec or mode change that ends one of them switches it off, and while it is on the shuffle and filter-auto are refused
    uint32_t byte_lag = 0, byte_stride = 0;
    bool byte_on() const { return byte_lag != 0; }
    bool byte_fits() const { return codec == CT_CODEC_HUFF0 && mode == CT_MODE_AUTO && !shuffle && !filter_auto; }
    void lag_keep()
    {
        if (!lag_fits()) { lag = 1; fold = 0; grid_width = 0; grid_fold = 0; vol_plane = 0; }
        if (!byte_fits()) { byte_lag = 0; byte_stride = 0; }
    }
    bool set_byte_delta(uint32_t l, uint32_t s)
    {
        if (l && (!ct_byte_lag_ok(l) || !ct_byte_stride_ok(s) || !byte_fits())) return false;
        byte_lag = l; byte_stride = l ? s : 0;
        return true;
    }
    bool set_shuffle(uint32_t elem)
    {
        if (elem > 1 && (!shuffle_elem_ok(elem) || codec == CT_CODEC_CHOOSE || filter_auto || byte_on())) return false;
        shuffle = elem > 1 ? elem : 0;
        if (elem <= 1) delta = false;                         // (no delta without the shuffle)
        lag_keep();
        return true;
    }
    bool set_delta(uint32_t on)
    {
        if (on > 1 || (on && !shuffle)) return false;
        delta = on != 0;
        lag_keep();
        return true;
    }
    bool set_delta_lag(uint32_t l, uint32_t f)
    {
        if (l < 1 || l > 16 || f > 1 || ((l != 1 || f) && (!lag_fits() || grid_on()))) return false;
        lag = l; fold = f;
        return true;
    }
    bool set_delta_grid(uint32_t w, uint32_t f)
    {
        if (f > 1 || (w && (!ct_grid_width_ok(w) || !lag_fits() || lag_on())) || (w && vol_on() && w >= vol_plane)) return false;
        grid_width = w; grid_fold = w ? f : 0;
        if (!w) vol_plane = 0;
        return true;
    }
    bool set_delta_volume(uint32_t p)
    {
        if (p && (!grid_on() || !ct_vol_plane_ok(grid_width, p))) return false;
        vol_plane = p;
        return true;
    }
    // choose-filters: the CHOOSE codec's order-0 frames take the auto mode (level 1) and the filter-auto ladder up to filter-auto,
    // filter-lag, filter-grid, filter-byte (levels 2 to 5), and the writer cuts its frames by class_rule.h; the stream is version 8,
    // 10, 13, 14 or 16.  A field of its own: mode, filter_auto and the rest stay what they are under CHOOSE (off), and so do their
    // getters and refusals.  Only ever non-zero with the CHOOSE codec; every codec call, one that sets CHOOSE again included, puts
    // it back to 0
    uint32_t choose_filters = 0;
    bool set_choose_filters(uint32_t level)
    {
        if (level > CLASS_MAX_LEVEL || codec != CT_CODEC_CHOOSE) return false;
        choose_filters = level;
        return true;
    }
    bool set_codec(uint32_t c)
    {
        if (c != CT_CODEC_BWT && c != CT_CODEC_HUFF0 && (c != CT_CODEC_CHOOSE || shuffle)) return false;
        codec = c;
        choose_filters = 0;
        if (!ct_mode_fits(mode, codec)) mode = CT_MODE_PLAIN;  // (no mode without its codec)
        filter_keep();
        lag_keep();
        return true;
    }
    // on: refused when the mode does not fit the codec or another mode is on (the modes exclude each other); off: clears the
    // mode if it is the one that is on
    bool set_mode(CtMode m, uint32_t on)
    {
        if (on > 1 || (on && (!ct_mode_fits(m, codec) || (mode != CT_MODE_PLAIN && mode != m)))) return false;
        if (on) mode = m;
        else if (mode == m) mode = CT_MODE_PLAIN;
        filter_keep();
        lag_keep();
        return true;
    }
    bool set_filter_auto(uint32_t on)
    {
        if (on > 1 || (on && (codec != CT_CODEC_HUFF0 || mode != CT_MODE_AUTO || shuffle || byte_on()))) return false;
        filter_auto = on != 0;
        filter_keep();
        lag_keep();                                           // (it needs the shuffle off and the lag needs it on: already (1, 0))
        return true;
    }
    bool set_filter_lag(uint32_t on)
    {
        if (on > 1 || (on && !filter_auto)) return false;
        filter_lag = on != 0;
        filter_keep();
        return true;
    }
    bool set_filter_grid(uint32_t on)
    {
        if (on > 1 || (on && !filter_lag)) return false;
        filter_grid = on != 0;
        filter_keep();
        return true;
    }
    bool set_filter_byte(uint32_t on)
    {
        if (on > 1 || (on && !filter_grid)) return false;
        filter_byte = on != 0;
        return true;
    }
    // what the plan speaks as a reader: its mode's version, and with the auto mode the sparse and rANS modes' as well
    uint32_t reader() const
    {
        if (choose_filters)                                   // (the order-0 plan's with the level's settings; under CHOOSE every mode is off)
            return CT_READS_AUTO | CT_READS_SPARSE | CT_READS_ANS | (choose_filters >= 2 ? CT_READS_FILTER : 0u) | (choose_filters >= 3 ? CT_READS_FILTER_LAG : 0u) |
                   (choose_filters >= 4 ? CT_READS_FILTER_GRID : 0u) | (choose_filters >= 5 ? CT_READS_FILTER_BYTE : 0u);
        return mode == CT_MODE_SPARSE ? CT_READS_SPARSE : mode == CT_MODE_RUNS ? CT_READS_RUNS : mode == CT_MODE_ANS ? CT_READS_ANS :
               mode == CT_MODE_AUTO ? CT_READS_AUTO | CT_READS_SPARSE | CT_READS_ANS | (filter_auto ? CT_READS_FILTER : 0u) | (filter_lag ? CT_READS_FILTER_LAG : 0u) | (filter_grid ? CT_READS_FILTER_GRID : 0u) | (filter_byte ? CT_READS_FILTER_BYTE : 0u) |
                                      (lag_on() ? CT_READS_LAG : 0u) | (grid_on() ? CT_READS_GRID : 0u) | (vol_on() ? CT_READS_VOL : 0u) | (byte_on() ? CT_READS_BYTE : 0u) :
               mode == CT_MODE_DEDUP ? CT_READS_DEDUP : 0u;
    }
    // the record kinds the writer may emit (bit k = kind k, as ct_kinds())
    uint32_t kinds() const
    {
        const bool k3 = mode == CT_MODE_SPARSE || mode == CT_MODE_AUTO || choose_filters, k5 = mode == CT_MODE_ANS || mode == CT_MODE_AUTO || choose_filters;
        return 1u << CT_KIND_RAW | (codec != CT_CODEC_HUFF0 ? 1u << CT_KIND_HUFF : 0u) | (codec != CT_CODEC_BWT ? 1u << CT_KIND_HUFF0 : 0u) |
               (k3 ? 1u << CT_KIND_SPARSE : 0u) |
               (mode == CT_MODE_RUNS ? 1u << CT_KIND_RUNS : 0u) | (k5 ? 1u << CT_KIND_ANS : 0u) |
               (mode == CT_MODE_DEDUP ? 1u << CT_KIND_DEDUP : 0u);
    }
};
// the writer's format: the lowest legal version whose kinds include every kind the settings may write
inline CtFormat format_of(const CtSettings &s)
{
    CtFormat f;
    if (s.choose_filters) { f.version = class_version(s.choose_filters); return f; }      // (that version's own triple: (v, 0, 0))
    if (s.filter_auto) { f.version = s.filter_byte ? CT_VERSION_FILTER_BYTE : s.filter_grid ? CT_VERSION_FILTER_GRID : s.filter_lag ? CT_VERSION_FILTER_LAG : CT_VERSION_FILTER; return f; }   // (the filter is each frame's own)
    if (s.byte_on()) {
        f.version = CT_VERSION_BYTE;
        f.flags = CT_FLAG_DELTA | (s.byte_stride ? CT_FLAG_GRID : 0u) | (s.byte_lag - 1) << CT_LAG_SHIFT;
        f.elem = 1; f.width = s.byte_stride;
        return f;
    }
    f.elem = s.shuffle;
    f.flags = s.shuffle && s.delta ? CT_FLAG_DELTA : 0;
    if (s.lag_on()) {                                         // (what (1, 0) does, version 8 says)
        f.version = CT_VERSION_LAG;
        f.flags |= (s.fold ? CT_FLAG_FOLD : 0u) | (s.lag - 1) << CT_LAG_SHIFT;
        return f;
    }
    if (s.grid_on()) {
        f.version = s.vol_on() ? CT_VERSION_VOL : CT_VERSION_GRID;
        f.flags |= (s.grid_fold ? CT_FLAG_FOLD : 0u) | CT_FLAG_GRID | (s.vol_on() ? CT_FLAG_VOL : 0u);
        f.width = s.grid_width; f.plane = s.vol_plane;
        return f;
    }
    for (uint32_t i = 0; i < CT_NLEGAL; i++) {
        f.version = ct_legal(i).version;
        if (format_legal(f) && (f.kinds() & s.kinds()) == s.kinds()) break;
    }
    return f;                                                 // (the setters accept only what some row takes)
}
CtSettings &plan_container_settings(CUDPPHandle plan);
// what the glcContainerLast* entries report, kept with the plan and gone with it
struct CtReports {
    unsigned long long error[3] = {0, ~0ull, ~0ull};       // {CtWhat, frame, block} of the last container call (~0 = none)
    unsigned long long range[3] = {};                      // {frames, blocks decoded, container bytes fetched} of the last successful range read
    unsigned long long choice[3] = {};                     // {blocks given to the BWT codec, to the order-0 codec, frames} of the last successful compress
    unsigned long long filters[FILTER_CANDS + 1] = {};     // frames per candidate of filter_rule.h, then all frames, of the last successful compress
    unsigned long long lag_filters[4] = {};                // frames that took the lag candidate of elem 2, 4, 8 (lag_rule.h) and their sum, of the same compress
    unsigned long long grid_filters[4] = {};               // frames that took the grid candidate of elem 2, 4, 8 (grid_rule.h) and their sum, of the same compress
    unsigned long long byte_filters[3] = {};               // frames that took byte (lag, 0), byte (lag, stride) (byte_rule.h) and their sum, of the same compress
};
CtReports &plan_container_reports(CUDPPHandle plan);
// the plan's two frame staging buffers for the filter (grown on demand, never shrunk, freed with the plan; encoder: one per
// call parity, decoder: buffer 0)
bool plan_pipelined(CUDPPHandle plan);
hipError_t plan_stage(CUDPPHandle plan, uint32_t which, size_t bytes, uint8_t **out);
// the plan's stream waits until the encode call that last used the next call's parity has released its input (pipelining:
// that call's Huffman stages and container kernels read their input from the side stream)
void plan_wait_released(CUDPPHandle plan);
// what the order-0 codec keeps with the plan: device
// scratch (which = 0 the encoder's, 1 the decoder's, 2 the entries of the frame index walk; grown on demand, never shrunk, freed with the plan, never allocated
// by a plan that only uses the BWT codec), the plan's live kernel profile, and its stage events (i = 0 .. 3: the marks of
// glcPlanLastTiming's four spans, recorded on the plan's stream; a no-op while timing is off)
hipError_t plan_codec_scratch(CUDPPHandle plan, uint32_t which, size_t bytes, uint8_t **out);
// Grow-only memory the plan keeps for what a container call needs beside the codecs' scratch: a call that has run once on
// inputs of its size allocates and frees nothing.  Device slots continue plan_codec_scratch's numbering; pinned slots are
// plan_pinned_scratch's.  The encoder and the decoder never share a slot (a range read decodes while an index lives), the
// host-pointer / file forms' staging is shared between the two directions (one call at a time on a plan).
enum CtDevSlot : uint32_t { CT_DEV_ENC_TABLES = 3, CT_DEV_DEC_TABLES, CT_DEV_DEC_STATE, CT_DEV_IN0, CT_DEV_IN1, CT_DEV_OUT, CT_DEV_SLOTS };
enum CtPinSlot : uint32_t { CT_PIN_STATS = 0, CT_PIN_COSTS, CT_PIN_VERDICT, CT_PIN_IN0, CT_PIN_IN1, CT_PIN_OUT, CT_PIN_SLOTS };
hipError_t plan_pinned_scratch(CUDPPHandle plan, uint32_t which, size_t bytes, void **out);
KernelProf *plan_prof(CUDPPHandle plan);
void plan_stage_mark(CUDPPHandle plan, int i);
// the runs mode's two ends of the plan's BWT codec, wholly on the plan's stream (the side stream is joined first).  Encode: the
// suffix sort and the MTF of nb blocks of n bytes at `in` -- bwt_index[b] and the MTF bytes, block b at *mtf + b * *stride.
// Decode: *mtf / *stride are the decoder's MTF rows (allocated on first use); rows [first_row, + nblk) of them -> inverse MTF ->
// inverse BWT with bwt_index[0 .. nblk) -> out, blocks of n bytes back to back
hipError_t plan_bwt_mtf(CUDPPHandle plan, const uint8_t *in, uint32_t n, uint32_t nb, int *bwt_index, const uint8_t **mtf, size_t *stride);
hipError_t plan_decode_rows(CUDPPHandle plan, uint8_t **mtf, size_t *stride);
hipError_t plan_decode_from_mtf(CUDPPHandle plan, uint32_t first_row, const int *bwt_index, uint8_t *out, uint32_t n, uint32_t nblk);

// ---------------------------------------------------------------------------
// kernels of container.hip
// ---------------------------------------------------------------------------
struct CtEncState {                                        // device: the running state of one container encode
    unsigned long long cursor;                             // bytes written (or that would have been) so far
    uint32_t crc_all, frames;
    uint32_t frame_acc, pad;                               // the frame's CRC, summed from its blocks' terms
};
struct CtEncFrame {                                        // device scratch of one frame (double-buffered by call parity)
    uint32_t *kind, *size, *only, *hist, *enc_off, *crc;   // crc: [2 nb] raw bytes, then records
    int *bwt;
    unsigned long long *boff, *seg_off, *seg_len, *start;  // boff: nb + 1 absolute word offsets; segs: 2 nb + 2
    uint32_t *tcrc;                                        // [2]
};
// what every kind kernel ends with: block b's kind and record words under the record rule (also_raw: the kernel's own further
// reason to store it raw), and from block 0's thread where the frame's payload starts; true = stored raw
__device__ inline bool ct_put_record(const CtEncFrame &f, uint32_t b, uint32_t kind, unsigned long long words, uint32_t blk_len,
                                     unsigned long long table_bytes, const CtEncState *state, bool also_raw = false)
{
    if (b == 0) *f.start = (state->cursor + CT_FRAME_HDR + table_bytes) / 4;
    const bool raw = also_raw || ct_stored_raw(words, blk_len);
    f.kind[b] = raw ? CT_KIND_RAW : kind;
    f.size[b] = raw ? ct_raw_words(blk_len) : (uint32_t)words;
    return raw;
}
struct CtEncHuff0 {                                        // device scratch of the order-0 codec's frame (plan_codec_scratch 0)
    unsigned long long *nun;                               // [rows] units of each block's stream
    unsigned long long *blk_off, *blk_len;                 // [rows] the blocks as segments of the frame
    // [rows] what the tables and the Huffman encoder read where that is not the block itself (absolute addresses: the block
    // or its kept bytes); the sparse and the auto mode's, with their scratch
    unsigned long long *in_off, *in_len;
    uint8_t *lens;                                         // [rows][256]
    uint16_t *codes;                                       // [rows][256]
    void *work;                                            // hdb_encode_work_bytes(rows)
};
struct CtEncSparse {                                       // device scratch of the sparse mode, behind CtEncHuff0's (allocated once it is on)
    uint32_t *mask; uint32_t mask_stride;                  // [rows][mask_stride] words
    uint32_t *fill, *is3, *skip_move, *skip_table;         // [rows]: fill byte; kind 3 chosen; 1 = not compacted; 1 = no table of K
    unsigned long long *klen, *kept_off, *unit_off;        // [rows]: bytes of K; K's place in `kept`; where the block's stream starts
    uint8_t *kept; uint32_t kept_stride;                   // [rows][kept_stride] bytes: the compaction space
};
struct CtEncRuns {                                         // device scratch of the runs mode (plan_codec_scratch 0; allocated once it is on)
    unsigned long long *x_off, *x_len;                     // [rows] the MTF rows as segments
    unsigned long long *seg_off, *seg_len;                 // [2 rows] A of the frame's nb blocks, then B of them: addresses, byte counts
    unsigned long long *nun, *unit_off;                    // [2 rows] units of each stream; where it starts in the payload
    uint32_t *skip_enc;                                    // [2 rows] 1 = not encoded (a raw block; an empty B)
    uint32_t *skip_b, *nz;                                 // [rows] 1 = B is empty (no table); non-zero counts of B
    uint32_t *hist_b;                                      // [rows][256] B's counts
    uint8_t *lens; uint16_t *codes;                        // [2 rows][256]
    void *work;                                            // hdb_encode_work_bytes(2 rows)
    uint8_t *a, *b; uint32_t stride;                       // [rows][stride] each
};
struct CtEncAns {                                          // device scratch of the rANS mode, behind CtEncHuff0's (allocated once it is on)
    uint8_t *tab;                                          // [rows] ANS_TAB_BYTES
    AnsScratch sc;                                         // [rows * ans_chunks(n)] slots: about 2 * rows * n bytes
    // [rows] behind the kinds: 1 = no kind-5 record to place (not kind 5, or raw); in the auto mode before them: 1 = not rANS-coded
    uint32_t *skip_ans;
};
struct CtEncAuto {                                         // device scratch of the auto mode, behind CtEncSparse's and CtEncAns's (allocated once it is on)
    uint32_t *uniform;                                     // [rows][256] the probe's chunk counts
    uint32_t *hist_s;                                      // [rows][256] candidate S's counts: the block's, or K's where S is kind 3
    uint32_t *wa, *pick5;                                  // [rows] the estimate wA; 1 = the block is coded as kind 5
};
struct CtEncDedup {                                        // device scratch of the dedup mode, behind CtEncSparse's (allocated once it is on)
    uint32_t *src, *refs; uint32_t nch;                    // [rows][nch]: the frame's map; each block's refs in chunk order
    uint32_t *mask; uint32_t mask_stride;                  // [rows][mask_stride] words: the 512-byte-chunk masks (sp.mask holds them widened to 64-byte chunks)
    uint32_t *E, *lo;                                      // [rows] elided chunks; the lowest block a source lies in
    DdSlot *table; uint64_t *hash; uint32_t slots;         // the map's scratch: slots + 1 slots, rows * nch hashes
};
// the dedup mode's steps (dedup.hip), in order, behind dedup_map: kind 6 or 2 per block from its row of the map (mask, refs, E,
// lo; for a kind-6 block sp's fields as the sparse mode leaves them, the mask widened for sparse_compact, and zero counts where
// nothing is kept); the mode's ct_enc_kind; and behind the payload offsets mask and refs into the records and sp.unit_off
hipError_t ct_enc_dedup_decide(hipStream_t st, const CtEncDedup &dd, const CtEncSparse &sp, const unsigned long long *blk_off, const uint8_t *d_in,
                               uint32_t nb, uint32_t blk_len, uint32_t *hist, unsigned long long *in_off, unsigned long long *in_len);
hipError_t ct_enc_dedup_kind(hipStream_t st, const CtEncFrame &f, const CtEncHuff0 &h, const CtEncSparse &sp, const CtEncDedup &dd, uint32_t nb,
                             uint32_t blk_len, const CtEncState *state);
hipError_t ct_enc_dedup_place(hipStream_t st, const CtEncFrame &f, const CtEncSparse &sp, const CtEncDedup &dd, uint32_t nb, uint32_t blk_len,
                              uint32_t *out, unsigned long long cap_words);
hipError_t ct_enc_header(hipStream_t st, uint8_t *out, unsigned long long cap, const uint32_t hdr[8], CtEncState *state);
hipError_t ct_block_offsets(hipStream_t st, unsigned long long *off, unsigned long long *len, uint32_t nb, uint32_t blk_len);   // off[b] = b * blk_len
// the order-0 codec's ct_enc_kind in every mode of that codec (the scratch of a mode that is off is not touched).  A block is
// kind 5 in the rANS mode and where au.pick5 says so in the auto mode, its words from the chunks' unit counts; else kind 3 where
// sp.is3 says so in the sparse and auto modes (the mask and, when anything is kept, the stream h.nun counts; the fill into f.bwt);
// else kind 2 (h.nun); and raw under the record rule whichever it was.  f.only = 1 where the Huffman encoder has nothing to write
// (raw, kind 5, kind 3 with nothing kept); an.skip_ans (rANS and auto modes) = 1 where ans_place has not (not kind 5, or raw)
hipError_t ct_enc_kind0(hipStream_t st, CtMode mode, const CtEncFrame &f, const CtEncHuff0 &h, const CtEncSparse &sp, const CtEncAns &an,
                        const CtEncAuto &au, uint32_t nb, uint32_t blk_len, const CtEncState *state);
hipError_t ct_enc_kind(hipStream_t st, const CtEncFrame &f, uint32_t nb, uint32_t blk_len, const CtEncState *state);
// the sparse mode's steps (sparse.hip), in order: the fill byte of every block from its histogram; kind 3 or 2 from the mask,
// with the histogram corrected to K's and (in_off, in_len) made what the tables and the encoder read; and behind the payload
// offsets the masks into the records and sp.unit_off = where each block's stream starts
hipError_t ct_enc_sparse_fill(hipStream_t st, const uint32_t *hist, uint32_t nb, uint32_t *fill);
hipError_t ct_enc_sparse_decide(hipStream_t st, const SpSegs &g, const CtEncSparse &sp, uint32_t *hist, unsigned long long *in_off,
                                unsigned long long *in_len);
hipError_t ct_enc_sparse_place(hipStream_t st, const CtEncFrame &f, const CtEncSparse &sp, uint32_t nb, uint32_t blk_len, uint32_t *out,
                               unsigned long long cap_words);
// the runs mode's steps (zrun.hip), in order: the MTF rows and the A / B spaces as segments; behind the split, which B is empty;
// the runs mode's ct_enc_kind (nz, record sizes under the record rule, skip masks); and behind the payload offsets nz and the
// pairs into the records and r.unit_off = where each stream starts
hipError_t ct_enc_runs_segs(hipStream_t st, const CtEncRuns &r, const uint8_t *mtf, size_t mtf_stride, uint32_t nb, uint32_t blk_len);
hipError_t ct_enc_runs_empty(hipStream_t st, const CtEncRuns &r, uint32_t nb);
hipError_t ct_enc_runs_kind(hipStream_t st, const CtEncFrame &f, const CtEncRuns &r, uint32_t nb, uint32_t blk_len, const CtEncState *state);
hipError_t ct_enc_runs_place(hipStream_t st, const CtEncFrame &f, const CtEncRuns &r, uint32_t nb, uint32_t *out, unsigned long long cap_words);
// the probe (auto.hip): hist[i][256] and uniform[i][256] of segment i = data + data_off[i], min(data_len[i], max_len) bytes
// (max_len <= 2^20), uniform[i][v] = its 64-byte chunks, counted from the segment's start, that hold byte v alone (the short last
// chunk included when it does).  The rows need not be zeroed.  Everything only enqueues on `st`.
hipError_t probe_segments(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                          uint32_t count, uint32_t max_len, uint32_t *hist, uint32_t *uniform);
// the bigram probe (choose.hip): row i of stats = {S2, SR, SC, M} of segment i (choose_rule.h), the segments as above.  Every row
// is written whole.  Everything only enqueues on `st`.
hipError_t bigram_probe_segments(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                                 uint32_t count, uint32_t max_len, unsigned long long *stats);
// the filter probe (filter_probe.hip, filter_rule.h): row i of planes = the 22 histograms of the first L - L % 8 bytes of segment i
// (L = min(data_len[i], max_len), max_len <= 2^31), row i of costs = the seven candidates' costs.  planes is 16-byte aligned and
// need not be zeroed.  Everything only enqueues on `st`.
hipError_t filter_probe_segments(hipStream_t st, const uint8_t *data, const unsigned long long *data_off,
                                 const unsigned long long *data_len, uint32_t count, uint32_t max_len, uint32_t *planes,
                                 unsigned long long *costs);
// the lag probe (lag_probe.hip, lag_rule.h), the segments as the filter probe's: row i of sums = the 48 sums S[e][l] of segment i
// and row i of lags its three winners; row i of planes = the 14 histograms of segment i at the lags of row i of `lags` (device
// memory, each word used as ((v - 1) & 15) + 1), row i of costs their three costs.  planes is 16-byte aligned; nothing need be
// zeroed.  Everything only enqueues on `st`.
hipError_t lag_probe_sums(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                          uint32_t count, uint32_t max_len, unsigned long long *sums, uint32_t *lags);
hipError_t lag_probe_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                            uint32_t count, uint32_t max_len, const uint32_t *lags, uint32_t *planes, unsigned long long *costs);
// the costs alone, of `count` segments' 14 rows; widths: null, or three width words a segment (device memory): an element size whose
// word is outside 2..65536 costs GRID_NO_COST
hipError_t lag_probe_cost(hipStream_t st, const uint32_t *planes, uint32_t count, const uint32_t *widths, unsigned long long *costs);
// the grid probe (grid_probe.hip, grid_rule.h), the segments as the filter probe's: row i of sums = the 3 * 65537 sums S_e[W] of
// segment i (0xFFFFFFFF where W is no candidate) and row i of widths its three winners (0: no candidate); row i of planes = the 14
// histograms of segment i at the widths of row i of `widths` (device memory; a word outside 2..65536 names no width: zero rows,
// GRID_NO_COST), row i of costs their three costs.  planes is 16-byte aligned; nothing need be zeroed.  Everything only enqueues.
hipError_t grid_probe_sums(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                           uint32_t count, uint32_t max_len, uint32_t *sums, uint32_t *widths);
hipError_t grid_probe_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                             uint32_t count, uint32_t max_len, const uint32_t *widths, uint32_t *planes, unsigned long long *costs);
// the byte probe (byte_probe.hip, byte_rule.h), the segments as the filter probe's: row i of lag_sums = the 16 sums A[l] of segment
// i, row i of stride_sums its 65537 sums S[W] (0xFFFFFFFF where W is no candidate) and row i of winners {lag, stride} (stride 0: no
// candidate); row i of planes = the two histograms of segment i at the {lag, stride} words of row i of `words` (device memory; the
// lag used as ((v - 1) & 15) + 1, a stride outside 17..65536 names none: a zero row, GRID_NO_COST), row i of costs their two
// costs (both GRID_NO_COST below 1024 counted bytes).  planes is 16-byte aligned; nothing need be zeroed.  Everything only enqueues.
hipError_t byte_probe_sums(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                           uint32_t count, uint32_t max_len, unsigned long long *lag_sums, uint32_t *stride_sums, uint32_t *winners);
// the lag sums alone and row i of words = {their winner, 0}: what byte_probe_planes takes to probe byte (best lag, stride 0) of
// every segment without the stride search (class_rule.h's eighth candidate)
hipError_t byte_probe_lags(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                           uint32_t count, uint32_t max_len, unsigned long long *lag_sums, uint32_t *words);
hipError_t byte_probe_planes(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                             uint32_t count, uint32_t max_len, const uint32_t *words, uint32_t *planes, unsigned long long *costs);
// the auto mode's steps (auto.hip), in order.  Behind the probe, the fill bytes and the blocks' rANS tables: candidate S of every
// block from the statistics (kind 3 when 32 E >= nch, K's bytes, its counts into au.hist_s, the segment its table and encoder would
// read into (in_off, in_len), sp.skip_table) and wA into au.wa.  Behind the tables of au.hist_s: wS, the choice (au.pick5), the
// skip masks of the mask / compaction passes (sp.skip_move) and of the rANS coder (an.skip_ans), and f.hist made K's where a
// block stays kind 3 (sp.is3 stays the candidate's: a block is kind 3 when it is set and au.pick5 is not).  Behind the passes,
// ct_enc_kind0 gives the actual sizes
hipError_t ct_enc_auto_candidates(hipStream_t st, const SpSegs &g, const CtEncSparse &sp, const CtEncAuto &au, const uint32_t *hist,
                                  const uint8_t *ans_tab, unsigned long long *in_off, unsigned long long *in_len);
hipError_t ct_enc_auto_choose(hipStream_t st, const CtEncFrame &f, const CtEncHuff0 &h, const CtEncSparse &sp, const CtEncAns &an,
                              const CtEncAuto &au, uint32_t nb, uint32_t blk_len);
// in: the frame as the blocks are cut from it (the shuffled frame with the filter on); orig: the frame's input bytes where
// they differ from `in` (else null) -- the stream's crc_all is theirs
// frame_word: the frame header's word 3 (0 below version 10)
hipError_t ct_enc_after_pack(hipStream_t st, const CtEncFrame &f, const uint8_t *in, const uint8_t *orig, uint32_t nb,
                             uint32_t blk_len, uint8_t *out, unsigned long long cap, CtEncState *state, uint32_t frame_word = 0);
hipError_t ct_enc_trailer(hipStream_t st, uint8_t *out, unsigned long long cap, CtEncState *state, unsigned long long *d_len);

struct CtDecFrame {                                        // device scratch of one frame's checks
    unsigned long long *seg_off, *seg_len;                 // [nb + 2]
    uint32_t *crc;                                         // [nb + 2]
    unsigned long long *verdict;                           // [2 + ceil(nb / 2)]: table verdict, block verdict, kinds (u32)
};
struct CtDecState { uint32_t crc_all, frame_acc; unsigned long long err; };   // err: (frame << 32 | block) + 1 of the first decoded-CRC miss
struct CtDecHuff0 {                                        // device scratch of a version-3 frame (plan_codec_scratch 1)
    uint32_t *skip;                                        // [nb] 1 = not kind 2
    unsigned long long *nun;                               // [nb] units the block's hist asks for (kind 2)
    uint16_t *lut;                                         // [nb][2048]
    void *work;                                            // hdb_decode_work_bytes(chunk, blk_len)
    uint32_t chunk;                                        // blocks one hdb_decode call may take
    // version 5 (kind 3 legal; version 8 as well): what the verdict leaves for the kind-3 blocks -- K's place in `kept` (block b in slot b % chunk)
    // and length, where the stream starts behind the mask, and 1 = nothing to decode (not kind 3, or nothing kept)
    uint32_t kinds;                                        // the format's legal kinds (ct_kinds)
    unsigned long long *k_off, *k_len, *u_off;             // [nb]
    uint32_t *skip3;                                       // [nb]
    uint8_t *kept; uint32_t kept_stride;                   // [chunk][kept_stride]
    // version 6 (kind 4 legal): the fields above serve A of the kind-4 blocks (k_off / k_len / u_off / skip3 / kept: A's place,
    // length, stream start, 1 = not kind 4); these are B's, the tables of B (built from the counts in the record before the
    // verdict: hist_b, skip_tb) and the decoder's MTF rows the join writes (block b in row b % chunk)
    unsigned long long *b_off, *b_len, *ub_off, *nun_b;    // [nb]
    uint32_t *skip_b, *skip_tb;                            // [nb] 1 = no B to decode; 1 = no table of B to build
    uint32_t *hist_b;                                      // [nb][256]
    uint16_t *lut_b;                                       // [nb][2048]
    uint8_t *kept_b;                                       // [chunk][kept_stride]
    unsigned long long *m_off, *m_len;                     // [nb]
    uint8_t *mtf; size_t mtf_stride;
    // version 7 (kind 5 legal; version 8 as well): the tables of the kind-5 blocks of one decoder chunk (block b in slot b % chunk), built from the
    // verified histograms behind the verdict
    uint8_t *ans_tab;                                      // [chunk] ANS_TAB_BYTES
};
struct CtDecDedup {                                        // device scratch of a version-9 frame, beside CtDecHuff0's (k_off / k_len / u_off / skip3 / kept serve K)
    uint32_t *src;                                         // [nb][nch] the frame's map: own ids, refs at the elided chunks of kind-6 blocks
    uint32_t *mask64; uint32_t stride64, chunk;            // [chunk][stride64] a kind-6 block's mask widened to 64-byte chunks (block b in row b % chunk)
};
// version 9 (dedup.hip): the tables of the kind-6 blocks join those k_cd_segs asks for; the verdict of a frame of kinds 0, 1, 2
// and 6 (ct_dec_verify calls both); src rows (masks = false) or widened masks (true) of blocks [first, first + count) of a
// verified frame
hipError_t ct_dec_dedup_skip(hipStream_t st, const uint8_t *frame, uint32_t nb, uint32_t *skip0);
hipError_t ct_dec_dedup_verdict(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                                unsigned long long payload_words, const CtDecHuff0 &h0);
hipError_t ct_dec_dedup_expand(hipStream_t st, const uint8_t *frame, uint32_t nb, uint32_t blk_len, uint32_t first, uint32_t count,
                               const CtDecDedup &dd, bool masks);
// the counts of B of every kind-4 block from its record's pairs (zeros where the record does not hold well-formed pairs), and
// whose table is built from them
hipError_t ct_dec_runs_hist(hipStream_t st, const uint8_t *frame, uint32_t nb, uint32_t blk_len, unsigned long long payload_words,
                            const CtDecHuff0 &h0);
// h0 (version 3 and later, else null): kind 2 is legal, and kinds 3 to 5 where h0->kinds says so; its blocks' tables are built from the unverified histograms first, and the
// units they ask for are one of the block's field checks
hipError_t ct_dec_verify(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                         unsigned long long payload_words, const CtDecHuff0 *h0 = nullptr, KernelProf *prof = nullptr);
// blocks [first, first + count) of the frame (count 0: all of them from `first` on)
hipError_t ct_dec_raw(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len, uint8_t *out,
                      uint32_t first = 0, uint32_t count = 0);
// fold = false: the blocks are checked but the stream's crc_all is left to ct_dec_fold (the filter's frames); a subset of
// the blocks (first, count as above) is never folded
hipError_t ct_dec_check(hipStream_t st, const CtDecFrame &f, const uint8_t *frame, uint32_t nb, uint32_t blk_len,
                        const uint8_t *out, uint32_t frame_index, CtDecState *state, bool fold = true, uint32_t first = 0,
                        uint32_t count = 0);
// the frame's nb * blk_len bytes at `bytes` (the unshuffled output) enter the stream's crc_all
hipError_t ct_dec_fold(hipStream_t st, const CtDecFrame &f, const uint8_t *bytes, uint32_t nb, uint32_t blk_len, CtDecState *state);

hipError_t ct_put_u64(hipStream_t st, unsigned long long *p, unsigned long long v);

} // namespace glc
