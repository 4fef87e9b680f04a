// bwt_bucket.hip -- the fast suffix sorter: ONE bucketing pass over HBM, then every bucket is
// sorted to the end inside LDS.  gfx950 / wave64.
//
// Replaces (result-for-result, same SA / BWT bytes / index) the reference's
//   cudppSuffixArrayDispatch / ComputeSA     (cudpp-inpar/src/cudpp/app/sa_app.cu:125-298,365-391)
//   bwt_compute_final_kernel                 (kernel/compress_kernel.cuh:55-74)
// for data whose suffixes separate within a few dozen symbols (i.i.d. bytes, float data: configs 2 and 4).
// Blocks it cannot finish are flagged and go on to the second tier, a string sample sort for text-like data
// (bwt_sample.hip); what that cannot finish either goes through the general sorter in bwt_sa.hip.  What the two tiers
// share on the device -- the layout of a suffix word, suffix comparison in the text -- is in fs_words.h.
//
// Idea.  A suffix is mapped to X = the arithmetic code of its first FS_DEPTH = 8 symbols under the block's own
// order-0 symbol statistics:
//      y7 = C[s7];   y_d = C[s_d] + floor(p[s_d] * y_{d+1} / 2^32)  (d = 6..1);   X = C[s0] * 2^32 + p[s0] * y1
// (Six symbols until round 5: the word keeps 36 bits of X, ~six Zipf symbols' worth -- but the pairs that share six symbols are
//  the FREQUENT prefixes, whose interval in 36 bits is wide enough for a 7th and an 8th symbol to be told apart: equal codes went
//  from 0.4 % to 0.03 % of a block, and with them most of what k_fs_sort_bwt's rare path and k_fs_ties cost.)
// (C = exclusive cumulative frequency, p = frequency, both scaled to 2^32; symbols past the end of the
// block contribute C = p = 0).  Two properties carry the whole design:
//   * X is monotone: suffix a < suffix b lexicographically  =>  X(a) <= X(b)   (each step maps the
//     sub-intervals of smaller symbols below those of larger ones, and floor() is monotone), so
//     DIFFERENT codes are always in the right order and only EQUAL codes need a look at the text;
//   * for i.i.d. data X is uniformly distributed whatever the symbol distribution is (Zipf included),
//     so "top 9 bits of X" cuts a 1 MiB block into 512 buckets of 2048 +- 7 % suffixes WITHOUT any
//     histogram of the buckets, and "next 12 bits" cuts a bucket into bins of ~0.5 suffixes.
// One word per suffix = [top 36 bits of X | suffix index : 20 | T[i-1] : 8]: the BWT byte rides along, so
// nothing is gathered afterwards.
//
//   k_fs_hist / k_fs_tables   symbol histogram of the block -> {C, p} table                 1 B read / suffix
//   k_fs_part2                text tile -> words -> bucketed in LDS -> appended to the bucket's slot
//                             (space reserved with one global atomic per (tile, bucket))      1 B R + 8 B W
//   k_fs_scan                 bucket fill -> rank base of every bucket, overflow -> flag (fs_scan: the sample sorter's launcher)
//   k_fs_sort / k_fs_sort_bwt one workgroup per bucket: counting sort on 12 more bits with LDS atomics
//                             (no stability needed: the index is not a tie-breaker), direct ranking inside
//                             the tiny bins; writes BWT bytes (+ SA) straight to their final rows;
//                             runs of equal codes go to a work list                             8 B R + 1 B W
//   k_fs_ties                 one thread per member of such a run: rank by comparing the suffixes in the
//                             text (0.4 % of the suffixes of a Zipf block)
//   k_fs_finish / k_fs_clear  flagged blocks -> live counts and the sample sorter's list; the pass's counters cleared
// = 19 B of HBM traffic per input byte (23 with the suffix array) where the 5-pass LSD sorter moves ~105.
#include "glc_device.h"
#include "glc_internal.h"
#include "fs_words.h"

namespace glc {

constexpr int      FSS_NT    = 512;                 // k_fs_sort: threads
constexpr int      FSS_ITEMS = FS_CAP / FSS_NT;     // slots per thread
#ifndef GLC_FS_BIN_BITS
#define GLC_FS_BIN_BITS 12
#endif
constexpr uint32_t FS_BIN_BITS = GLC_FS_BIN_BITS, FS_BINS = 1u << FS_BIN_BITS;
#ifndef GLC_FSS_LOOK
#define GLC_FSS_LOOK 4
#endif
constexpr uint32_t FSS_LOOK = GLC_FSS_LOOK;         // k_fs_sort_bwt's rank step: words from a bin's start compared in straight-line code
constexpr uint32_t FS_MAX_GROUP = 512;              // longest run of equal codes ranked by direct count
// k_fs_sort_bwt: a bin start is a 16-bit entry that holds at most FS_FILLMAX: the bits above FS_START_MASK are free, and the
// top one says "this bin has more than FSS_LOOK words" (set by the words that arrived as its fifth and later)
constexpr uint32_t FS_START_MASK = 0x0FFFu, FS_BIG_BIN = 0x8000u;
static_assert(FS_FILLMAX <= FS_START_MASK, "a bin start and the end of the last bin fit below the big-bin flag");
// k_fs_sort_bwt, what a workgroup pays once (profiles/sort_entry.md; 0 builds the form before, for the A/B):
#ifndef GLC_FSS_ENTRY
#define GLC_FSS_ENTRY 1                              // the entry: workgroup order without a division, one batch of scalar loads
#endif
#ifndef GLC_FSS_SCAN
#define GLC_FSS_SCAN 1                               // bin_starts(): packed halves, scalar wave number, one barrier
#endif
constexpr uint32_t FSS_SENT = 2 * FSS_LOOK;         // k_fs_sort_bwt: sentinels behind the last word (the rare case looks at 2 FSS_LOOK keys from a bin's start)

// at least 16 buckets: k_fs_sort compares bits 28..59 of the words, so the four bits above must be bucket number
uint32_t fs_bucket_log2(uint32_t n)
{
    uint32_t l = 4;
    while (((uint64_t)FS_AVG << l) < n && l < FS_MAXNB_LOG2) l++;
    return l;
}

// ---------------------------------------------------------------------------
// symbol histogram: 8 copies per workgroup (copy = lane & 7, stride 257 words so equal symbols of
// different copies sit in different banks): equal symbols inside a wave serialise on an LDS atomic,
// and Zipf data puts 10 lanes of 64 on the same symbol
// ---------------------------------------------------------------------------
constexpr uint32_t FSH_SLICE = 32768;
// Text-likeness probe, free of charge inside the histogram pass: two of a thread's eight 16-byte vectors give a
// 6-gram each (512 samples per 32 KB slice); a sample whose 6-gram another sample of the slice has already put into a
// 2048-slot LDS table is a REPEAT.  I.i.d. bytes (Zipf(1.0), float data, random) repeat ~0 times per 1 MiB block, text and
// log lines hundreds to thousands of times: exactly the blocks whose order-0 code is lumpy (a frequent 6-gram = one code
// shared by thousands of suffixes), which the bucket sorter would flag after a wasted attempt.  k_fs_tables flags a block
// with FS_DUP_FLAG repeats or more up front: its tiles leave k_fs_part2 / k_fs_sort / k_fs_ties at once and the sample sorter
// takes it.  A wrong guess costs time, never correctness (the other way round, the attempt flags the block as before).
constexpr uint32_t FSH_SLOTS = 2048, FS_DUP_FLAG = 48;

// {C, p} scaled to 2^32.  floor() on both keeps C[s] + p[s] <= C[s+1], which is what makes the code monotone.
constexpr uint32_t FS_DONE = 8u;                    // flag value: the block is finished (a constant block: k_fs_tables wrote its rows)

__global__ __launch_bounds__(256) void k_fs_tables(const uint32_t *__restrict__ hist, uint32_t n,
                                                   uint2 *__restrict__ tab, const uint32_t *__restrict__ dup,
                                                   uint32_t *__restrict__ flag, const uint8_t *__restrict__ text, size_t stride,
                                                   uint8_t *__restrict__ bwt_out, size_t bwt_stride, int *__restrict__ d_index,
                                                   uint32_t *__restrict__ sa_out, size_t sa_stride, uint32_t step)
{
    __shared__ uint32_t s_tmp[5];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t hraw = hist[(size_t)b * 256 + tid];
    // step > 1: the counts are those of every step-th 32 KB slice of the block (k_fs_hist).  The code is monotone whatever the
    // table is as long as C[s] + p[s] <= C[s + 1] holds for every symbol THAT OCCURS; a SAMPLE'S statistics cut the block into
    // buckets as evenly as the block's own, within the sampling noise.  Every symbol gets one count on top of the sample's
    // (0.1 % of the code space): a symbol the sample missed keeps a positive width and its place in the order -- with width 0
    // the symbols above the sample's last one would sit at C = 2^32, clamped BELOW the end of that last symbol's interval
    // (fuzz seed 2: a block whose sampled slices held two symbols, 79 196 bytes of 254 others in between).
    const uint32_t h = hraw + (step > 1 ? 1u : 0u);
    uint32_t ns = 0;
    const uint32_t c = block_excl_add<256>(h, s_tmp, &ns);
    // A block of ONE symbol (zero pages, padding) has nothing to sort: SA = n-1 .. 0, every BWT byte is the symbol, the
    // index row is n - 1.  Left to the tiers it is their worst case -- every suffix ties with every other for the whole
    // block: bucket overflow, the sample sorter's depth cap, then ~20 prefix-doubling rounds of the general sorter (1.3 ms
    // where a Zipf block takes 0.012).  FS_DONE overrides whatever the flag was (text-likeness, a caller's "sample sorter
    // first"): every tier skips a flagged block, and k_fs_finish does not list this one for anybody.  Its rows are written
    // right here, by this workgroup (a kernel of its own was one more launch in every call's chain).
    bool constant = __syncthreads_or((int)(hraw == ns - (step > 1 ? 256u : 0u))) != 0;
    if (constant && step > 1) {                                // (uniform) one symbol in the SAMPLE: look at the whole block
        const uint8_t *T = text + (size_t)b * stride;
        const uint32_t sym = T[0];
        bool other = false;
        for (uint32_t i = tid; i < n && !other; i += 256) other = T[i] != sym;
        constant = __syncthreads_or((int)other) == 0;
    }
    if (tid == 0) {
        if (constant) flag[b] = FS_DONE;
        else if (dup[b] >= (FS_DUP_FLAG + step - 1) / step) flag[b] = 1u;   // text-like (see k_fs_hist): straight to the sample sorter
    }
    if (constant) {
        const uint32_t sym = text[(size_t)b * stride];
        const uint32_t v = sym * 0x01010101u;
        if (bwt_out) {
            uint8_t *O = bwt_out + (size_t)b * bwt_stride;
            const uint32_t head = min(n, (uint32_t)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(O) & 15u)) & 15u));
            const uint32_t nvec = (n - head) / 16;
            for (uint32_t i = tid; i < head; i += 256) O[i] = (uint8_t)sym;
            for (uint32_t i = tid; i < nvec; i += 256) reinterpret_cast<uint4 *>(O + head)[i] = make_uint4(v, v, v, v);
            for (uint32_t i = head + nvec * 16 + tid; i < n; i += 256) O[i] = (uint8_t)sym;
        }
        if (sa_out) for (uint32_t i = tid; i < n; i += 256) sa_out[(size_t)b * sa_stride + i] = n - 1 - i;
        if (d_index && tid == 0) d_index[b] = (int)(n - 1);
        return;                                                // (uniform; the table of a flagged block is never read)
    }
    const uint64_t C32 = ((uint64_t)c << 32) / ns, P32 = ((uint64_t)h << 32) / ns;
    tab[(size_t)b * 256 + tid] = make_uint2((uint32_t)(C32 > 0xFFFFFFFFull ? 0xFFFFFFFFull : C32),
                                            (uint32_t)(P32 > 0xFFFFFFFFull ? 0xFFFFFFFFull : P32));
}

#ifndef GLC_FSH_COPIES
#define GLC_FSH_COPIES 16
#endif
constexpr int FSH_COPIES = GLC_FSH_COPIES;             // LDS copies of the histogram (same-symbol atomics of a wave spread over them)
__global__ __launch_bounds__(256) void k_fs_hist(const uint8_t *__restrict__ text, size_t stride, uint32_t n,
                                                 uint32_t *__restrict__ hist, uint32_t *__restrict__ dup, uint32_t step)
{
    __shared__ uint32_t s_h[FSH_COPIES * 257];
    __shared__ uint32_t s_fp[FSH_SLOTS];
    __shared__ uint32_t s_dup;
    const uint32_t b = blockIdx.y, tid = threadIdx.x;
    const uint32_t lo = blockIdx.x * step * FSH_SLICE;        // (step > 1: every step-th slice -- see k_fs_tables)
    if (lo >= n) return;
    const uint32_t hi = min(n, lo + FSH_SLICE);
    for (uint32_t i = tid; i < FSH_COPIES * 257; i += 256) s_h[i] = 0;
    for (uint32_t i = tid; i < FSH_SLOTS; i += 256) s_fp[i] = 0;
    if (tid == 0) s_dup = 0;
    __syncthreads();
    const uint8_t *T = text + (size_t)b * stride;
    uint32_t *H = s_h + (tid & (FSH_COPIES - 1)) * 257;
    uint32_t done = lo;
    if ((reinterpret_cast<uintptr_t>(T + lo) & 15) == 0) {
        const uint32_t nvec = (hi - lo) / 16;                       // <= 2048 = 8 per thread
        const uint4 *V = reinterpret_cast<const uint4 *>(T + lo);
        uint4 q[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t i = r * 256 + tid;
            q[r] = i < nvec ? V[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 8; r += 4) {
            if (r * 256 + tid < nvec) {
                // fingerprint of the vector's first six bytes (never 0); equal 6-grams give equal fingerprints and slots
                const uint32_t fp = (q[r].x * 0x9E3779B1u + (q[r].y & 0xFFFFu) * 0x85EBCA6Bu) | 1u;
                const uint32_t old = atomicCAS(&s_fp[(fp * 0xC2B2AE35u) >> 21], 0u, fp);
                if (old == fp) atomicAdd(&s_dup, 1u);
            }
        }
#pragma unroll
        for (int r = 0; r < 8; r++) {
            if (r * 256 + tid < nvec) {
                const uint32_t wd[4] = {q[r].x, q[r].y, q[r].z, q[r].w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    atomicAdd(&H[wd[k] & 0xFF], 1u);
                    atomicAdd(&H[(wd[k] >> 8) & 0xFF], 1u);
                    atomicAdd(&H[(wd[k] >> 16) & 0xFF], 1u);
                    atomicAdd(&H[wd[k] >> 24], 1u);
                }
            }
        }
        done = lo + nvec * 16;
    }
    for (uint32_t i = done + tid; i < hi; i += 256) atomicAdd(&H[T[i]], 1u);
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < FSH_COPIES; k++) c += s_h[k * 257 + tid];
    if (c) atomicAdd(&hist[(size_t)b * 256 + tid], c);
    if (tid == 0 && s_dup) atomicAdd(&dup[b], s_dup);
}

// ---------------------------------------------------------------------------
// bucketing pass
// ---------------------------------------------------------------------------
// FSP2_T consecutive tiles of a block per workgroup.  The counters put the one-tile form of this pass (round 3's k_fs_part,
// which lives on as the sample sorter's k_ss_part) at 0.45 of the VALU issue rate, 0.19 of the scalar one and the LDS 0.38 busy -- nothing is saturated: a
// tile's 12.7 us are a chain  flag + table + text from memory -> codes -> scan -> 512 global atomics with return -> scatter
// -> stores, and four workgroups per CU do not cover its waits.  The loop over tiles lets
//   * the symbol table and the block's flag arrive once per workgroup;
//   * the text of tile t + 1 be requested before tile t is touched (six dwords per thread in registers), so it has the
//     whole of tile t to arrive;
//   * the global atomic of a (tile, bucket) be ISSUED before the words are scattered in LDS and CONSUMED after (the
//     scatter needs the tile-local ranks only), with LDS-only barriers in between so that nobody waits for it early;
//   * the stores of tile t retire under tile t + 1 (the prefetched text is taken out of its registers before they are issued:
//     loads and stores share one counter, in order).  That holds only where the compiler's counter model sees no load in
//     flight at the loop's header: one loop over edge and inner tiles alike, entered with the first request pending and left
//     by `return` behind a request (a return inside a loop is routed through its latch), had `s_waitcnt vmcnt(0)` at the
//     latch and in front of the stg -> LDS writes, so every tile drained its 64 KB of scattered stores with all waves
//     behind a barrier.  Hence the shape below: the run of inner tiles is a loop of its own, entered behind an explicit wait
//     for its first tile's text, the block's flag is looked at BEFORE the next request is issued, and the edge tiles stay
//     outside.  On the way round that loop the only wait on the memory counter is the vmcnt(0) that takes in the tile's
//     own fill atomic, half a tile behind the stores of the tile before (profiles/part2_waits.md).
#ifndef GLC_FSP2_T
#define GLC_FSP2_T 4
#endif
constexpr int FSP2_T = GLC_FSP2_T;
#ifndef GLC_FSP2_WAVES
#define GLC_FSP2_WAVES 5
#endif
#ifndef GLC_FSP2_NT
#define GLC_FSP2_NT 512
#endif
#ifndef GLC_FSP2_TILE
#define GLC_FSP2_TILE 4096
#endif
constexpr int FSP2_TILE = GLC_FSP2_TILE;                       // suffixes per tile of k_fs_part2
constexpr int FSP2_NT = GLC_FSP2_NT;                           // threads per workgroup; a thread takes 4096 / FSP2_NT consecutive suffixes
#ifndef GLC_FSP2_PHASES
#define GLC_FSP2_PHASES 1                                      // (A/B: 0 = the batch instance's inner tile item-major like the others)
#endif

__device__ __forceinline__ void lds_only_barrier()
{
    // __syncthreads() carries a workgroup-scope fence: every wave would wait for ALL its outstanding memory operations,
    // the prefetched text and the atomic in flight included
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// block_excl_add_lds over the first FS_MAXNB threads only (one per bucket; the others pass through the barrier and get a
// value nobody uses), with the wave number read as a uniform value: the "waves below mine" test is scalar instead of
// sixteen lane masks kept in SGPRs across the tile loop
template <int NT>
__device__ __forceinline__ uint32_t bucket_excl_add_lds(uint32_t x, uint32_t *s_tmp)
{
    constexpr uint32_t NW = (NT < (int)FS_MAXNB ? NT : FS_MAXNB) / WAVE;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t inc = wave_incl_add(x);
    if ((threadIdx.x & 63) == 63 && w < NW) s_tmp[w] = inc;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    uint32_t base = 0;
#pragma unroll
    for (uint32_t i = 0; i < NW; i++)
        if (i < w) base += s_tmp[i];
    return base + inc - x;
}

template <int NT, int ITEMS, int WPE>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_fs_part2(const uint8_t *__restrict__ text, size_t stride, uint32_t n, uint32_t nbl,
                                                     const uint2 *__restrict__ tab, uint64_t *__restrict__ keys, size_t kstride,
                                                     uint32_t *__restrict__ fill, uint32_t *__restrict__ flag,
                                                     uint32_t *__restrict__ zero_bucket, uint32_t tiles_per_wg)
{
    constexpr uint32_t TILE = NT * ITEMS;                      // suffixes per tile
    // one block of LDS with the tile's words LAST: everything else sits below 64 KB, where a per-thread or zero address
    // register plus the instruction's 16-bit offset reaches it (no address register per array held across the tile loop)
    __shared__ struct {
        uint32_t cnt[FS_MAXNB];
        uint16_t start[FS_MAXNB], gbase[FS_MAXNB];
        uint2 tab[256];
        uint32_t tmp[NT / 64 + 1];
        uint32_t flagged;
        uint64_t w[NT * ITEMS];
    } sh;
    uint32_t *s_cnt = sh.cnt, *s_tmp = sh.tmp;
    uint16_t *s_start = sh.start, *s_gbase = sh.gbase;
    uint2 *s_tab = sh.tab;
    uint64_t *s_w = sh.w;
    uint32_t &s_flagged = sh.flagged;
    uint8_t *s_txt = reinterpret_cast<uint8_t *>(s_w);         // s_txt[k] = T[base - 1 + k]: dead before the first word is bucketed
    uint32_t bx, by;
    xcd_order(bx, by);                                         // a block's tiles on ONE XCD, back to back
    const uint32_t b = by, tid = threadIdx.x;
    const uint32_t ntiles = (n + TILE - 1) / TILE, tile0 = bx * tiles_per_wg;
    if (tile0 >= ntiles) return;
    const uint8_t *T = text + (size_t)b * stride;
    if (tid == 0) s_flagged = flag[b];                         // flagged up front as text-like, or by a tile that ran before
    if (tid < 256) s_tab[tid] = tab[(size_t)b * 256 + tid];
    // text of a tile as the dwords of T[base - 1 ...] (unaligned 4-byte loads: global memory takes any alignment): dword
    // q = r NT + tid of the 4112 staged bytes.  Only for inner tiles; the first and the last tile of a block take the byte loop.
    constexpr int NSTG = ((TILE + 16) / 4 + NT - 1) / NT;      // staged dwords per thread
    uint32_t stg[NSTG] = {};
    auto inner = [&](uint32_t tile) { const uint32_t base = tile * TILE; return base > 0 && base + TILE + 16 <= n; };
    auto request = [&](uint32_t tile) {
        const uint8_t *D = T + (size_t)tile * TILE - 1;
#pragma unroll
        for (int r = 0; r < NSTG; r++) {
            const uint32_t q = r * NT + tid;
            const uint32_t qq = q < (TILE + 16) / 4 ? q : 0u;   // (every load is issued: a conditional one may sink to its use)
            uint32_t v;
            __builtin_memcpy(&v, D + 4 * (size_t)qq, 4);
            stg[r] = v;
        }
    };
    const uint32_t tend = min(ntiles, tile0 + tiles_per_wg);
    uint64_t *K = keys + (size_t)b * kstride;
    static_assert(TILE <= (1u << 20), "a rank inside (tile, bucket) rides in the index field of the word until the scatter");
    constexpr uint32_t LOW = (uint32_t)FS_LOW_MASK;            // the word's low dword: [4 code bits | index : 20 | bwt : 8]
    // bucket of a word = its top nbl bits, from the high dword (nbl <= 9; a field of width 0 is 0)
    auto bucket_of = [&](uint32_t hi) { return __builtin_amdgcn_ubfe(hi, 32u - nbl, nbl); };
    // One tile: codes -> ranks inside (tile, bucket) -> scan + global atomics -> LDS scatter -> stores.  false: the block is
    // flagged.  EDGE: the tile holds suffixes past n or its 16 bytes behind reach past the block (its last tile, or its only
    // one): the per-suffix guards below exist in this instance only.
    auto tile_body = [&](auto edge_t, uint32_t base, bool next_inner) __attribute__((always_inline)) -> bool {
        constexpr bool EDGE = decltype(edge_t)::value;
        // the inner tile of the instance with four waves per SIMD (128 VGPRs to spend) keeps all of a thread's table entries,
        // ranks and bucket starts in registers and asks LDS for each kind in one go
        constexpr bool PHASES = !EDGE && WPE <= 4 && GLC_FSP2_PHASES;
        // thread = 8 consecutive suffixes gi0 .. gi0+7; byte j of its 16 staged bytes is T[gi0 - 1 + j]
        const uint32_t k0 = tid * ITEMS, gi0 = base + k0;
        constexpr int NBY = (ITEMS + FS_DEPTH + 3) / 4;       // dwords that hold the thread's ITEMS + FS_DEPTH staged bytes (k0 is a multiple of ITEMS)
        uint32_t by4[NBY];
        if (ITEMS % 8 == 0) {
#pragma unroll
            for (int q = 0; q < NBY; q += 2) {
                const uint2 v = *reinterpret_cast<const uint2 *>(s_txt + k0 + 4 * q);
                by4[q] = v.x;
                if (q + 1 < NBY) by4[q + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int q = 0; q < NBY; q++) by4[q] = *reinterpret_cast<const uint32_t *>(s_txt + k0 + 4 * q);
        }
#define FS_BYTE(j) ((by4[(j) >> 2] >> (8 * ((j) & 3))) & 0xFFu)
        // table entry of the symbol at byte 1 + k (past the end of the block: C = p = 0)
        uint2 e[ITEMS + FS_DEPTH - 1];
        auto entry = [&](int k) {
            const uint2 t = s_tab[FS_BYTE(1 + k)];
            if constexpr (EDGE) return gi0 + k >= n ? make_uint2(0u, 0u) : t;
            else return t;
        };
        auto code = [&](int j) {
            uint32_t y = e[j + FS_DEPTH - 1].x;
#pragma unroll
            for (int d = FS_DEPTH - 2; d >= 1; d--) y = e[j + d].x + __umulhi(e[j + d].y, y);
            return ((uint64_t)e[j].x << 32) + (uint64_t)e[j].y * y;
        };
        // the words leave this phase as [high dword | low dword with the RANK inside (tile, bucket) in the index field]: the
        // bucket is the high dword's top bits and the index is gi0 + j, both re-derived at the scatter
        uint32_t xh[ITEMS], xl[ITEMS];
        if constexpr (PHASES) {
            // phase-major: every table read is in flight before the first code is computed, and the rank atomics leave as
            // the codes complete -- the first returned rank is looked at behind the last atomic (item-major, each code sat
            // behind its own table read AND the rank atomic of the code before: eight LDS round trips per thread)
#pragma unroll
            for (int k = 0; k < ITEMS + FS_DEPTH - 1; k++) e[k] = entry(k);
            __builtin_amdgcn_sched_barrier(0);
            uint32_t rk[ITEMS];
#pragma unroll
            for (int j = 0; j < ITEMS; j++) {
                const uint64_t X = code(j);
                xh[j] = (uint32_t)(X >> 32);
                xl[j] = (uint32_t)X & ~LOW;
                rk[j] = atomicAdd(&s_cnt[bucket_of(xh[j])], 1u);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < ITEMS; j++) xl[j] |= rk[j] << 8;
        } else {
            // item-major: entry k is dead behind code k, so the entries come in as the codes need them (a window of FS_DEPTH in
            // registers rather than all ITEMS + FS_DEPTH - 1)
#pragma unroll
            for (int k = 0; k < FS_DEPTH - 1; k++) e[k] = entry(k);
#pragma unroll
            for (int j = 0; j < ITEMS; j++) {
                e[j + FS_DEPTH - 1] = entry(j + FS_DEPTH - 1);
                // (the edge tile: a word's low half in ONE register from here, not the code bits and the rank apart until the scatter)
                if constexpr (EDGE) if (j > 0) asm volatile("" : "+v"(xl[j - 1]));
                const uint64_t X = code(j);
                const uint32_t hi = (uint32_t)(X >> 32), bk = bucket_of(hi);
                uint32_t r = 0;
                if (!EDGE || gi0 + j < n) r = atomicAdd(&s_cnt[bk], 1u);
                xh[j] = hi;
                xl[j] = ((uint32_t)X & ~LOW) | (r << 8);
                // where the word of suffix 0 goes: k_fs_sort_bwt looks for the BWT index there only (a block's first tile is an edge tile)
                if constexpr (EDGE) if (j == 0 && gi0 == 0) zero_bucket[b] = bk;
            }
        }
        lds_only_barrier();
        uint32_t g = 0, c = 0;
        {
            c = tid < FS_MAXNB ? s_cnt[tid] : 0u;
            const uint32_t start = bucket_excl_add_lds<NT>(c, s_tmp);
            if (c) g = atomicAdd(&fill[(size_t)b * FS_MAXNB + tid], c);     // issued here, looked at behind the scatter
            if (tid < FS_MAXNB) s_start[tid] = (uint16_t)start;
        }
        // the BWT bytes go in from the staged text, read again here rather than kept through the code phase
        {
            const uint2 v = *reinterpret_cast<const uint2 *>(s_txt + k0);
            by4[0] = v.x;
            by4[1] = v.y;
#pragma unroll
            for (int j = 0; j < ITEMS; j++) xl[j] |= FS_BYTE(j);
        }
#undef FS_BYTE
        lds_only_barrier();                                    // (the staged text and the table reads are done: s_w takes the words)
        if constexpr (PHASES) {
            uint32_t at[ITEMS];                                 // the eight bucket starts asked for together, then the eight words written
#pragma unroll
            for (int j = 0; j < ITEMS; j++) at[j] = s_start[bucket_of(xh[j])];
#pragma unroll
            for (int j = 0; j < ITEMS; j++) {
                const uint32_t lo = (xl[j] & ~(LOW ^ 0xFFu)) | ((gi0 + j) << 8);
                s_w[at[j] + ((xl[j] >> 8) & 0xFFFFFu)] = ((uint64_t)xh[j] << 32) | lo;
            }
        } else {
#pragma unroll
            for (int j = 0; j < ITEMS; j++) {
                asm volatile("" : "+v"(xh[j]), "+v"(xl[j]));    // two registers per word across the scan, not the code phase's bucket, rank and index
                if (!EDGE || gi0 + j < n) {
                    const uint32_t lo = (xl[j] & ~(LOW ^ 0xFFu)) | ((gi0 + j) << 8);
                    s_w[s_start[bucket_of(xh[j])] + ((xl[j] >> 8) & 0xFFFFFu)] = ((uint64_t)xh[j] << 32) | lo;
                }
            }
        }
        if (c && g + c > FS_FILLMAX) { atomicOr(&flag[b], 1u); s_flagged = 1; }
        if (tid < FS_MAXNB) s_gbase[tid] = (uint16_t)(g < FS_CAP ? g : FS_CAP);
        if (next_inner) {                                      // the next tile's text has arrived before this tile's stores are issued
#pragma unroll                                                 // (loads and stores share one in-order counter)
            for (int r = 0; r < NSTG; r++) asm volatile("" : "+v"(stg[r]));
        }
        lds_only_barrier();
        if constexpr (EDGE) {
            const uint32_t tile_n = min((uint32_t)TILE, n - base);
#pragma unroll
            for (int r = 0; r < ITEMS; r++) {
                const uint32_t p = r * NT + tid;
                if (p < tile_n) {
                    const uint64_t ww = s_w[p];
                    const uint32_t d = bucket_of((uint32_t)(ww >> 32));
                    const uint32_t off = (uint32_t)s_gbase[d] + (p - (uint32_t)s_start[d]);
                    if (off < FS_CAP) K[(size_t)d * FS_CAP + off] = ww;
                }
            }
        } else {
            // A bucket this tile's words would carry past FS_CAP has set s_flagged above (g + c > FS_FILLMAX): a tile that is not
            // flagged stores every word inside its bucket's slot, and a flagged block's slots are read by nobody
            if (__builtin_amdgcn_readfirstlane(s_flagged)) return false;
#pragma unroll
            for (int r = 0; r < ITEMS; r++) {
                const uint32_t p = r * NT + tid;
                const uint64_t ww = s_w[p];
                const uint32_t d = bucket_of((uint32_t)(ww >> 32));
                K[d * FS_CAP + (uint32_t)s_gbase[d] + (p - (uint32_t)s_start[d])] = ww;
            }
        }
        return true;
    };
    // The tile proper comes in two instances: an INNER tile (every suffix of it and the 16 bytes behind it inside the block, and
    // not the block's first) takes its text from stg and runs without a per-suffix guard; an edge tile (the first of a block:
    // the byte in front of suffix 0 is the block's last; the last one or two: suffixes past n, symbols past the end
    // contributing C = p = 0) fetches its text byte by byte and keeps the guards.  A workgroup's tiles are at most one edge
    // tile, a run of inner tiles, and one or two edge tiles; the run is a loop of its own, entered with its first tile's text
    // arrived, so that on the way round it no path brings a load in flight to its header.
    uint32_t tile = tile0;
    if (inner(tile)) request(tile);
#pragma clang loop unroll(disable)
    while (tile < tend) {
        if (!inner(tile)) {
            const uint32_t base = tile * TILE;
            if (tid < FS_MAXNB) s_cnt[tid] = 0;
            for (uint32_t k = tid; k < TILE + 16; k += NT) {
                const int64_t g = (int64_t)base - 1 + k;
                s_txt[k] = g < 0 ? T[n - 1] : (g < (int64_t)n ? T[g] : (uint8_t)0);
            }
            lds_only_barrier();
            if (s_flagged) return;
            const bool next_inner = tile + 1 < tend && inner(tile + 1);
            if (next_inner) request(tile + 1);                 // in flight until this tile's words are in LDS
            tile_body(std::true_type{}, base, next_inner);
            lds_only_barrier();                               // s_w is free for the next tile's text
            tile++;
            continue;
        }
#pragma unroll
        for (int r = 0; r < NSTG; r++) asm volatile("" : "+v"(stg[r]));   // the run's first tile has arrived
#pragma clang loop unroll(disable)
        for (;;) {
            if (tid < FS_MAXNB) s_cnt[tid] = 0;
#pragma unroll
            for (int r = 0; r < NSTG; r++) {
                const uint32_t q = r * NT + tid;
                if (q < (TILE + 16) / 4) reinterpret_cast<uint32_t *>(s_txt)[q] = stg[r];
            }
            lds_only_barrier();                                // (stg is in LDS: its registers take the next tile's request)
            if (s_flagged) return;                             // (ahead of the request: no way out of the loop with a load in flight)
            const bool more = tile + 1 < tend && inner(tile + 1);
            if (more) request(tile + 1);                       // in flight until this tile's words are in LDS
            if (!tile_body(std::false_type{}, tile * TILE, more)) return;
            lds_only_barrier();                               // s_w is free for the next tile's text
            tile++;
            if (!more) break;
        }
    }
}

// rank base of every bucket (exclusive scan of the fills); a bucket past its slot flags the block
__global__ __launch_bounds__(FS_MAXNB) void k_fs_scan(const uint32_t *__restrict__ fill, uint32_t *__restrict__ fbase,
                                                      uint32_t *__restrict__ flag, const uint32_t *__restrict__ list)
{
    __shared__ uint32_t s_tmp[FS_MAXNB / 64 + 1];
    const uint32_t b = list ? list[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
    const uint32_t f = fill[(size_t)b * FS_MAXNB + tid];
    if (f > FS_FILLMAX) atomicOr(&flag[b], 1u);
    fbase[(size_t)b * FS_MAXNB + tid] = block_excl_add<FS_MAXNB>(f, s_tmp);
}

// ---------------------------------------------------------------------------
// one workgroup sorts one bucket in LDS and writes its rows of the result.  Runs of equal codes (a few
// per bucket on Zipf data) are not resolved here -- that needs the text, and a global-memory round trip on
// the critical path of every workgroup cost more than the whole sort -- but appended to a work list that
// k_fs_ties resolves with one thread per member afterwards.
// ---------------------------------------------------------------------------
// LDS diet (40.7 KB: FOUR workgroups per CU, 8 waves per SIMD, where 52 KB allowed three): the bin counters are
// 16-bit pairs (a bucket holds < 4096 words), the sorted words are capped at FS_FILLMAX (a fuller bucket flags its
// block), and the BWT bytes are staged in the counter array once the bin starts are dead.
__global__ __launch_bounds__(FSS_NT) void k_fs_sort(uint32_t n, uint32_t nbl, const uint64_t *__restrict__ keys,
                                                    size_t kstride, const uint32_t *__restrict__ fill,
                                                    const uint32_t *__restrict__ fbase, uint32_t *__restrict__ flag,
                                                    uint8_t *__restrict__ bwt_out, size_t bwt_stride,
                                                    int *__restrict__ d_index, uint32_t *__restrict__ sa_out,
                                                    size_t sa_stride, uint4 *__restrict__ wl, uint32_t wl_cap,
                                                    uint32_t *__restrict__ wl_count)
{
    __shared__ uint64_t s_w[FS_FILLMAX + 4];                   // + 4 sentinels behind the last word
    __shared__ uint32_t s_cp[FS_BINS / 2 + 1];                 // bin counters, then bin starts (two 16-bit values per word), then BWT bytes
    __shared__ uint32_t s_tmp[FSS_NT / 64 + 1];
    __shared__ uint32_t s_deep, s_wl;
    uint16_t *s16 = reinterpret_cast<uint16_t *>(s_cp);
    uint8_t *s_cb = reinterpret_cast<uint8_t *>(s_cp);
    uint32_t gx, gy;
    xcd_order(gx, gy);
    const uint32_t b = gy, bk = gx, tid = threadIdx.x;
    if (tid == 0) { s_deep = flag[b]; s_wl = 0; }              // (one read: another bucket may flag the block meanwhile)
    for (uint32_t i = tid; i < FS_BINS / 2; i += FSS_NT) s_cp[i] = 0;
    const uint32_t c = fill[(size_t)b * FS_MAXNB + bk];
    const uint32_t R0 = fbase[(size_t)b * FS_MAXNB + bk];
    const uint64_t *K = keys + (size_t)b * kstride + (size_t)bk * FS_CAP;
    uint64_t w[FSS_ITEMS];
#pragma unroll
    for (int r = 0; r < FSS_ITEMS; r++) {
        const uint32_t i = r * FSS_NT + tid;
        w[r] = ~0ull;
        if (r * FSS_NT < c && c <= FS_FILLMAX && i < c) w[r] = K[i];
    }
    if (tid < 4 && c <= FS_FILLMAX) s_w[c + tid] = ~0ull;      // what the rank step reads past the last bin compares as larger
    __syncthreads();
    if (s_deep || c == 0) return;                              // flagged: the block goes through the general sorter
    // 1. counting sort on the 12 bits below the bucket number (arrival order inside a bin: any order will do)
    const uint32_t bshift = 64 - nbl - FS_BIN_BITS;
    uint32_t rk[FSS_ITEMS];
#pragma unroll
    for (int r = 0; r < FSS_ITEMS; r++) {
        rk[r] = 0;
        if (r * FSS_NT >= c) continue;                         // (uniform: a bucket fills half of the slots on average)
        const uint32_t i = r * FSS_NT + tid;
        const uint32_t bin = (uint32_t)(w[r] >> bshift) & (FS_BINS - 1), sh = 16 * (bin & 1);
        if (i < c) rk[r] = (atomicAdd(&s_cp[bin >> 1], 1u << sh) >> sh) & 0xFFFFu;
    }
    __syncthreads();
    {
        constexpr int PW = FS_BINS / 2 / FSS_NT;               // packed words per thread
        uint32_t v[PW], sum = 0;
#pragma unroll
        for (int k = 0; k < PW; k++) { v[k] = s_cp[tid * PW + k]; sum += (v[k] & 0xFFFFu) + (v[k] >> 16); }
        uint32_t run = block_excl_add<FSS_NT>(sum, s_tmp);
#pragma unroll
        for (int k = 0; k < PW; k++) {
            const uint32_t lo = run, hi = run + (v[k] & 0xFFFFu);
            s_cp[tid * PW + k] = lo | (hi << 16);
            run = hi + (v[k] >> 16);
        }
        if (tid == FSS_NT - 1) s_cp[FS_BINS / 2] = c;          // end of the last bin
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < FSS_ITEMS; r++) {
        if (r * FSS_NT >= c) continue;
        const uint32_t i = r * FSS_NT + tid;
        if (i < c) s_w[s16[(uint32_t)(w[r] >> bshift) & (FS_BINS - 1)] + rk[r]] = w[r];
    }
    __syncthreads();
    // 2. final position = bin start + number of smaller codes in the bin (thread = the words at positions r NT + tid
    //    of the bin-sorted array).  A bin holds ~1.5 words seen from one of them: the four words from the bin start
    //    are compared in straight-line code with no bounds at all -- what lies behind the bin's end is a larger code
    //    or a sentinel -- and only a bin of more than four walks the rest in a loop.  Words with EQUAL codes form a
    //    group [gp, gp + gs) whose internal order is not known yet: they take a second, exact look (rare).
    uint32_t *SAo = sa_out ? sa_out + (size_t)b * sa_stride + R0 : nullptr;
    uint32_t pos[FSS_ITEMS], grp[FSS_ITEMS];                   // grp = group start << 16 | group size (0: not tied)
#pragma unroll
    for (int r = 0; r < FSS_ITEMS; r++) {
        const uint32_t p = r * FSS_NT + tid;
        pos[r] = 0xFFFFFFFFu; grp[r] = 0;
        if (r * FSS_NT >= c) continue;
        if (p < c) {
            const uint64_t wv = s_w[p];
            w[r] = wv;
            const uint32_t key = (uint32_t)(wv >> 28);         // inside a bin only the low 32 bits of the code can differ
            const uint32_t bin = (uint32_t)(wv >> bshift) & (FS_BINS - 1);
            const uint32_t gs = s16[bin], ge = s16[bin + 1];
            if (ge - gs > FS_MAX_GROUP) { s_deep = 1; }
            else {
                uint32_t less = 0, eqt = 0;
                const uint2 *B = reinterpret_cast<const uint2 *>(s_w) + gs;
#pragma unroll
                for (uint32_t t = 0; t < 4; t++) {
                    const uint2 wq = B[t];
                    const uint32_t kq = __builtin_amdgcn_alignbit(wq.y, wq.x, 28);
                    less += kq < key ? 1u : 0u;
                    eqt += kq == key ? 1u : 0u;
                }
                if (ge - gs > 4) {
#pragma clang loop unroll(disable)
                    for (uint32_t q = gs + 4; q < ge; q++) {
                        const uint2 wq = reinterpret_cast<const uint2 *>(s_w)[q];
                        const uint32_t kq = __builtin_amdgcn_alignbit(wq.y, wq.x, 28);
                        less += kq < key; eqt += kq == key;
                    }
                }
                const uint32_t idx = (uint32_t)(wv >> 8) & 0xFFFFFu;
                uint32_t at = gs + less;
                if (eqt > 1) {                                 // exact: members of my group inside the bin, and those before me
                    uint32_t eqb = 0; eqt = 0;
#pragma clang loop unroll(disable)
                    for (uint32_t q = gs; q < ge; q++) {
                        const uint2 wq = reinterpret_cast<const uint2 *>(s_w)[q];
                        const bool e = __builtin_amdgcn_alignbit(wq.y, wq.x, 28) == key;
                        eqt += e; eqb += e & (q < p);
                    }
                    if (eqt > 1) { grp[r] = (at << 16) | eqt; at += eqb; }
                }
                pos[r] = at;
                if (!grp[r]) {
                    if (SAo) SAo[at] = idx;
                    if (idx == 0 && d_index) d_index[b] = (int)(R0 + at);
                }
            }
        }
    }
    __syncthreads();                                           // s_cp (bin starts) is dead from here: it takes the BWT bytes
    if (s_deep) { if (tid == 0) atomicOr(&flag[b], 2u); return; }
    // rows R0 .. R0 + c of the block's BWT are staged so that aligned dwords of LDS are aligned dwords of the output
    uint8_t *O = bwt_out ? bwt_out + (size_t)b * bwt_stride + R0 : nullptr;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(O) & 3u);
    // 3. tied groups -> the block's work list.  Entries are reserved with ONE global atomic per workgroup
    //    (an atomic per group on a shared counter serialised the whole kernel: +2.4 ms per 256 blocks).
    bool any = false;
#pragma unroll
    for (int r = 0; r < FSS_ITEMS; r++) {
        if (pos[r] != 0xFFFFFFFFu) s_cb[shift + pos[r]] = (uint8_t)w[r];      // (rows of tied groups are rewritten by k_fs_ties)
        if (grp[r]) {
            any = true;
            const uint32_t gp = grp[r] >> 16, gs = grp[r] & 0xFFFFu;
            if (pos[r] == gp) reinterpret_cast<uint32_t *>(s_w)[2 * gp + 1] = atomicAdd(&s_wl, gs);   // (the codes are dead)
        }
    }
    if (__syncthreads_or((int)any)) {
        if (tid == 0) {
            const uint32_t tot = s_wl;
            uint32_t base = atomicAdd(&wl_count[b], tot);
            if (base + tot > wl_cap) { atomicOr(&flag[b], 4u); base = 0xFFFFFFFFu; }   // list full: block flagged
            s_deep = base;
        }
        __syncthreads();
        const uint32_t base = s_deep;
        uint4 *WL = wl + (size_t)b * wl_cap;
        if (base != 0xFFFFFFFFu) {
#pragma unroll
            for (int r = 0; r < FSS_ITEMS; r++) {
                if (grp[r]) {
                    const uint32_t gp = grp[r] >> 16, gs = grp[r] & 0xFFFFu, slot0 = base + reinterpret_cast<const uint32_t *>(s_w)[2 * gp + 1];
                    WL[slot0 + (pos[r] - gp)] = make_uint4((uint32_t)(w[r] & FS_LOW_MASK), R0 + gp, slot0, gs);
                }
            }
        }
    }
    // 4. the rows
    if (O) {
        const uint32_t end = shift + c;                        // staged bytes [shift, end)
        for (uint32_t q = tid; 4 * q < end; q += FSS_NT) {
            const uint32_t v = s_cp[q];
            if (4 * q >= shift && 4 * q + 4 <= end) *reinterpret_cast<uint32_t *>(O - shift + 4 * q) = v;
            else {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    if (4 * q + k >= shift && 4 * q + k < end) O[4 * q + k - shift] = (uint8_t)(v >> (8 * k));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// k_fs_sort_bwt: k_fs_sort for the BWT-only path (no suffix array asked for), on a scalar-instruction diet.  The counters
// put k_fs_sort at 109 VALU + 93.5 SALU + 14.7 LDS instructions per suffix with the scalar pipe 0.66 busy, and nearly
// all of the scalar work is exec-mask bookkeeping of per-item conditions, eight items per thread.  Here
//   * the ONE partial round of a bucket (c mod 512 words) is round 0 and carries the only per-lane predicate; rounds
//     1 .. c / 512 are full and run under a uniform branch alone (k_fs_sort: `i < c` in every round of every loop);
//   * the rare cases of the rank step -- a bin of more than four words, another word with the same code -- are found
//     per wave with ONE ballot and handled behind a wave-uniform branch (k_fs_sort: three nested divergent branches per
//     item, executed or not).  "More than four words" is a flag in the bin's start entry, set by the words that arrived
//     fifth and later (3e-4 of them), so the rank step reads a bin's start only; behind the branch a word reads the
//     bin's end and the next four keys with one wait and finishes a bin of up to eight in straight-line code -- the
//     serial walk of the bin, one dependent LDS read per member in front of the workgroup's barrier, is left to bins of
//     nine and more (profiles/sort_rank_tail.md);
//   * whether the workgroup has work-list entries to write is its own counter s_wl read behind the barrier that is
//     there anyway, not a workgroup-wide OR;
//   * the row of suffix 0 (the BWT index) is looked for in the ONE bucket k_fs_part2 saw it go to (zero_bucket), not in
//     every word of every bucket -- behind a branch the compiler cannot fold into the words' own conditions (it did: the
//     compares ran for every slot of every workgroup and the bucket test was ANDed in last);
//   * the bin of a word is a field of its HIGH dword (bshift = 52 - nbl >= 43): one 32-bit shift, no 64-bit temporaries.
// Instances by the number of FULL rounds.  A bucket of an i.i.d.-like block holds 2048 +- 7 % words: c / 512 is 3 or 4, and
// eight slots per thread (a slot may hold 4032 words) meant three to four slots initialised, tested per lane in every loop
// and guarded in every phase for nothing.  After the common prologue -- the flag exit, the counters cleared, three rounds
// of words requested before the fill is known -- ONE wave-uniform branch picks
//   * rounds<3> / rounds<4>: FULL + 1 slots, slots 1 .. FULL unconditional, slot 0 under `tid < part`, nothing else; and
//     PHASE-MAJOR: every slot's LDS requests of a step are issued before the first answer is waited for (all counting
//     atomics, all bin starts, and in the rank step all words, then all bin bounds, then all keys), the rare case is ORed
//     over the thread's slots into ONE ballot and ONE branch per wave.  Item-major, a thread walked ~25 dependent LDS round
//     trips where the data ask for ~5.  (`pos == ~0` comes with s_deep = 1 only, and the kernel leaves on s_deep before
//     anything is staged: the staging and work-list loops test no position.)
//   * everything else (small and skewed blocks, c / 512 in {0, 1, 2, 5, 6, 7}): the eight-slot guarded body.
// Same LDS layout and access pattern in all of them (a word is ranked AT ITS POSITION of the bin-sorted array: bin bounds,
// neighbours and the staged row of neighbouring lanes share banks -- the owner-ranked form measured in round 4 lost more to
// LDS bank conflicts than it saved in instructions, tools/exp/attic), same rank rule, same work list, entry for entry.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(FSS_NT) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fs_sort_bwt(uint32_t nbl, const uint64_t *__restrict__ keys, size_t kstride,
                                                        const uint32_t *__restrict__ fill, const uint32_t *__restrict__ fbase,
                                                        uint32_t *__restrict__ flag, uint8_t *__restrict__ bwt_out,
                                                        size_t bwt_stride, int *__restrict__ d_index, uint4 *__restrict__ wl,
                                                        uint32_t wl_cap, uint32_t *__restrict__ wl_count,
                                                        const uint32_t *__restrict__ zero_bucket)
{
    __shared__ uint64_t s_w[FS_FILLMAX + FSS_SENT];            // + sentinels behind the last word
    __shared__ uint32_t s_cp[FS_BINS / 2 + 1];                 // bin counters, then bin starts (two 16-bit values per word), then BWT bytes
    __shared__ uint32_t s_tmp[FSS_NT / 64 + 1];
    __shared__ uint32_t s_deep, s_wl;
    uint16_t *s16 = reinterpret_cast<uint16_t *>(s_cp);
    uint8_t *s_cb = reinterpret_cast<uint8_t *>(s_cp);
    uint32_t gx, gy;
#if GLC_FSS_ENTRY
    xcd_order_pow2(gx, gy, nbl);                               // (the grid's x size is the bucket count, 1 << nbl)
#else
    xcd_order(gx, gy);
#endif
    const uint32_t b = gy, bk = gx, tid = threadIdx.x;
    // A block flagged BEFORE this kernel started -- text-like (k_fs_tables), a bucket past its slot (k_fs_part2), constant -- is
    // another sorter's: its 512 workgroups leave on a scalar load, before the table of counters is cleared and three rounds of
    // words are asked for (0.25 ms per batch of 256 text blocks were spent leaving).  Bits 1 and 8 only: nobody sets those while
    // this kernel runs, so every wave of the workgroup sees the same (what k_fs_sort_bwt itself sets, 2 and 4, goes through s_deep)
#if GLC_FSS_ENTRY
    // What a workgroup does once is spread over four or five words per thread, so the entry is kept short: one batch of
    // arguments; the flag by a scalar load, and the exit; then the word requests, with nothing waited for in front of them
    // but that flag.  The bucket's fill and rank base and the block's zero bucket -- like the flag's bits 1 and 8, nobody writes
    // them while this kernel runs -- are scalar loads too (const_load_u32), which the compiler issues beside the word
    // requests and waits for where the fill is first used.  The offsets into the per-block tables (b * FS_MAXNB + bk, one
    // dword per bucket of a call) and into a block's slots (bk * FS_CAP <= 2^21) are 32-bit products; b * kstride, b * bwt_stride and b * wl_cap stay 64-bit: a block's words
    // are 16 MiB, its work list entries 16 bytes, and neither the strides nor the number of blocks have a bound that keeps a
    // byte offset below 2^32 (2048 blocks of words are 32 GiB).
    // The flag's two uses want different things.  The exit wants bits 1 and 8, which are final before the launch: the scalar
    // load gives them.  s_deep's initial value wants bits 2 and 4 as well, which OTHER workgroups of this launch set (a bin
    // of more than FS_MAX_GROUP words, a full work list).  No result depends on seeing them: a block so flagged is sorted again
    // by the next tier whatever this bucket writes, a full list refuses every later reservation by its count, and the flag is
    // only ever ORed.  But a workgroup that sees them leaves behind the first barrier instead of sorting a bucket for nothing,
    // and data with runs (zero pages in float data) flag most blocks of a call this way.  The scalar cache is not coherent with
    // the other workgroups' atomics, so that value takes a second, vector read.  Wave 0 asks for it BEFORE the words and
    // stores it behind them: the wait is for that one dword (vmcnt counts the word requests as still in flight), and no
    // lane mask is held across the requests.
    // (The empty statement wants every argument in a register HERE: the compiler otherwise fetches them where they are used,
    // four batches with a wait each in front of the first word request.  A plain load of flag[b] under a uniform branch
    // becomes a scalar load too, hence the atomic one: agent scope, so it is answered by the L2 the other workgroups' atomics
    // went to.  Both are a compiler's choices, not the language's: after a toolchain change the entry's machine code is
    // looked at again -- the list of what to find there is in profiles/sort_entry.md, "After a compiler change".)
    asm volatile("" :: "s"(keys), "s"(kstride), "s"(fill), "s"(fbase), "s"(bwt_out), "s"(bwt_stride), "s"(d_index), "s"(wl),
                 "s"(wl_cap), "s"(wl_count), "s"(zero_bucket));
    const uint32_t bo = b * FS_MAXNB + bk;
    const uint32_t f0 = const_load_u32(flag + b);
    const uint32_t c = const_load_u32(fill + bo), R0 = const_load_u32(fbase + bo);
    const bool zb = const_load_u32(zero_bucket + b) == bk;     // (uniform) suffix 0 is one of this bucket's words
    if (f0 & (1u | FS_DONE)) return;
    const bool wave0 = __builtin_amdgcn_readfirstlane(tid >> 6) == 0;
    uint32_t f1 = 0;
    if (wave0) f1 = __hip_atomic_load(flag + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t *K = keys + (size_t)b * kstride + bk * FS_CAP;
#else
    if (scalar_load_u32(flag + b) & (1u | FS_DONE)) return;
    if (tid == 0) { s_deep = flag[b]; s_wl = 0; }              // (one read: another bucket may flag the block meanwhile)
    for (uint32_t i = tid; i < FS_BINS / 2; i += FSS_NT) s_cp[i] = 0;
    const uint64_t *K = keys + (size_t)b * kstride + (size_t)bk * FS_CAP;
#endif
    // The first FSS_SPEC full rounds are requested BEFORE the bucket's fill is known: a bucket of an i.i.d.-like block holds
    // 2048 +- 7 % words, so words 0 .. 1535 are (nearly) always there, and fill -> words was two memory latencies in a row at
    // the head of every workgroup's chain.  A slot has FS_CAP words whatever its fill: reading past the fill is harmless, and
    // such a round is never looked at (r <= full guards every use).
    constexpr int FSS_SPEC = 3;
    uint64_t ws[FSS_SPEC + 1];
#pragma unroll
    for (int r = 1; r <= FSS_SPEC; r++) ws[r] = K[(r - 1) * FSS_NT + tid];
#if GLC_FSS_ENTRY
    static_assert(FS_BINS / 2 % FSS_NT == 0, "every thread clears the same number of counter words");
#pragma unroll
    for (uint32_t k = 0; k < FS_BINS / 2 / FSS_NT; k++) s_cp[k * FSS_NT + tid] = 0;
    if (wave0) { s_deep = f1; s_wl = 0; }                      // (every lane of the wave writes the same two values)
#else
    const uint32_t c = fill[(size_t)b * FS_MAXNB + bk];
    const uint32_t R0 = fbase[(size_t)b * FS_MAXNB + bk];
    const bool zb = zero_bucket[b] == bk;                      // (uniform) suffix 0 is one of this bucket's words
#endif
    const uint32_t cc = c <= FS_FILLMAX ? c : 0u;              // (a fuller bucket has flagged its block in k_fs_scan)
    // item r of a thread: r = 0 -> word full * 512 + tid of the partial round (lanes tid < part), r >= 1 -> word
    // (r - 1) * 512 + tid of a full round (all lanes, r <= full)
    const uint32_t full = cc / FSS_NT, part = cc % FSS_NT;
    const bool v0 = tid < part;
    const uint32_t i0 = full * FSS_NT + tid;
    const uint32_t bshift = 64 - nbl - FS_BIN_BITS;            // >= 43: the bin lies in a word's high dword
    const uint32_t hshift = bshift - 32, kshift = bshift - 28; // ... at hshift there, at kshift in a sorted word's key
    // rows R0 .. R0 + c of the block's BWT are staged so that aligned dwords of LDS are aligned dwords of the output
    uint8_t *O = bwt_out + (size_t)b * bwt_stride + R0;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(O) & 3u);

    // bin counters -> bin starts (both 16-bit pairs), between the count and the scatter step of every instance
    auto bin_starts = [&]() __attribute__((always_inline)) {
        constexpr int PW = FS_BINS / 2 / FSS_NT;               // packed words per thread
#if GLC_FSS_SCAN
        // On packed halves: a bucket holds at most FS_FILLMAX < 2^16 words, so any sum of its counters fits one half and no
        // carry crosses into the other.  P = [run : 16 | run : 16] walks the thread's words: the starts of word k are
        // P + (v[k] << 16) (low bin at run, high bin at run + low count) and P moves on by v[k] + rot16(v[k]), the word's
        // total in both halves.  Across the waves, as in bucket_excl_add_lds: the wave's number is uniform and s_tmp is
        // written here only, once per workgroup, so ONE barrier; the "waves below mine" sum is three row shifts over the
        // eight totals, one lane each, not eight lane-mask selects per thread.
        static_assert(FSS_NT / WAVE == 8 && FS_FILLMAX < 0x10000u, "eight wave totals in lanes 0 .. 7 of a row; sums stay inside a half");
        const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6), l8 = tid & 7u;
        uint32_t v[PW], t = 0;
#pragma unroll
        for (int k = 0; k < PW; k++) { v[k] = s_cp[tid * PW + k]; t += v[k]; }
        const uint32_t sum = (t & 0xFFFFu) + (t >> 16);
        const uint32_t inc = wave_incl_add(sum);
        if ((tid & 63u) == 63u) s_tmp[wv] = inc;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        uint32_t x = s_tmp[l8];
        x = l8 < wv ? x : 0u;
        x += GLC_DPP(x, 0x111, 0xf);       // row_shr:1
        x += GLC_DPP(x, 0x112, 0xf);       // row_shr:2
        x += GLC_DPP(x, 0x114, 0xf);       // row_shr:4: lane 7 = the totals of the waves below mine
        const uint32_t run = (uint32_t)__builtin_amdgcn_readlane((int)x, 7) + inc - sum;
        uint32_t P = run | (run << 16);
#pragma unroll
        for (int k = 0; k < PW; k++) {
            s_cp[tid * PW + k] = P + (v[k] << 16);
            P += v[k] + __builtin_amdgcn_alignbit(v[k], v[k], 16);
        }
#else
        uint32_t v[PW], sum = 0;
#pragma unroll
        for (int k = 0; k < PW; k++) { v[k] = s_cp[tid * PW + k]; sum += (v[k] & 0xFFFFu) + (v[k] >> 16); }
        uint32_t run = block_excl_add<FSS_NT>(sum, s_tmp);
#pragma unroll
        for (int k = 0; k < PW; k++) {
            const uint32_t lo = run, hi = run + (v[k] & 0xFFFFu);
            s_cp[tid * PW + k] = lo | (hi << 16);
            run = hi + (v[k] >> 16);
        }
#endif
        if (tid == FSS_NT - 1) s_cp[FS_BINS / 2] = c;          // end of the last bin
    };
    // in LDS a word is [code bits 28..59 : 32 | the word's low dword (code bits 28..31, index, BWT byte) : 32]: the rank step
    // compares HIGH DWORDS only -- four 4-byte reads where the whole words were four 8-byte reads and a funnel shift each
    auto sorted_word = [](uint64_t wv) -> uint64_t {
        const uint32_t lo = (uint32_t)wv, hi = (uint32_t)(wv >> 32);
        return ((uint64_t)__builtin_amdgcn_alignbit(hi, lo, 28) << 32) | lo;
    };
    // the rank step's rare case, exact over the whole bin [gs, ge) for the word at position p: its row, and its group if
    // other words share its code
    auto rank_rare = [&](uint32_t key, uint32_t p, uint32_t gs, uint32_t ge, uint32_t &at, uint32_t &grp) __attribute__((always_inline)) {
        if (ge - gs > FS_MAX_GROUP) { s_deep = 1; at = 0xFFFFFFFFu; }
        else {
            uint32_t ls = 0, eq = 0, eqb = 0;
#pragma clang loop unroll(disable)
            for (uint32_t q = gs; q < ge; q++) {
                const uint32_t kq = reinterpret_cast<const uint32_t *>(s_w)[2 * q + 1];
                ls += kq < key; eq += kq == key; eqb += (kq == key) & (q < p);
            }
            at = gs + ls;
            if (eq > 1) { grp = (at << 16) | eq; at += eqb; }
        }
    };
    // ... with the bin's end and the keys at gs + FSS_LOOK .. gs + 2 FSS_LOOK - 1 read together (one wait; k1 = the keys at
    // gs .. gs + FSS_LOOK - 1, which the rank step has in registers): a bin of up to 2 FSS_LOOK words is finished from the
    // eight keys in straight-line code with no bounds -- what lies behind the bin's end is a larger code or a sentinel (a key
    // of all ones could tie with a sentinel: it takes the loop, which stops at the bin's end).  Only a longer bin (6e-8 of
    // the words of i.i.d. data) walks the loop otherwise.
    auto rank_rare2 = [&](uint32_t key, uint32_t p, uint32_t gs, const uint32_t *k1, uint32_t &at, uint32_t &grp) __attribute__((always_inline)) {
        const uint32_t *B = reinterpret_cast<const uint32_t *>(s_w) + 2 * (gs + FSS_LOOK) + 1;
        uint32_t k2[FSS_LOOK];
#pragma unroll
        for (uint32_t t = 0; t < FSS_LOOK; t++) k2[t] = B[2 * t];
        const uint32_t ge = s16[((key >> kshift) & (FS_BINS - 1)) + 1] & FS_START_MASK;
        if ((ge - gs > 2 * FSS_LOOK) | (key == 0xFFFFFFFFu)) rank_rare(key, p, gs, ge, at, grp);
        else {
            uint32_t ls = 0, em = 0;                           // em: bit t = the key at gs + t is mine
#pragma unroll
            for (uint32_t t = 0; t < 2 * FSS_LOOK; t++) {
                const uint32_t kq = t < FSS_LOOK ? k1[t < FSS_LOOK ? t : 0] : k2[t < FSS_LOOK ? 0 : t - FSS_LOOK];
                ls += kq < key ? 1u : 0u;
                em |= kq == key ? 1u << t : 0u;
            }
            const uint32_t eq = __builtin_popcount(em);
            at = gs + ls;
            if (eq > 1) { grp = (at << 16) | eq; at += __builtin_popcount(em & ((1u << (p - gs)) - 1u)); }
        }
    };
    // 3. (every instance) tied groups -> the block's work list.  Entries are reserved with ONE global atomic per workgroup.
    //    (Round 5: the ~1.5 us a workgroup sits out for its return are NOT on the kernel's critical path -- with entries of the
    //    bucket's own and no atomic at all the kernel ran 3.50 against 3.47 ms per GiB, and k_fs_ties, which then has to walk
    //    512 short lists per block, 0.32 against 0.18.)
    auto wl_reserve = [&](uint32_t pos, uint32_t grp) __attribute__((always_inline)) {
        const uint32_t gp = grp >> 16, gs = grp & 0xFFFFu;
        if (pos == gp) reinterpret_cast<uint32_t *>(s_w)[2 * gp + 1] = atomicAdd(&s_wl, gs);   // (the codes are dead)
    };
    auto wl_base = [&]() __attribute__((always_inline)) -> uint32_t {   // 0xFFFFFFFF: nothing to write
        // every tied group's size is in s_wl (wl_reserve) before this barrier, which is also the one between the staged
        // bytes and the row stores: s_wl != 0 is "some thread of the workgroup has an entry to write" (a workgroup-wide OR
        // of the threads' own flags -- a DPP reduce, an LDS exchange and two barriers -- cost 0.3 ms per 2048-block launch)
        __syncthreads();
        const uint32_t tot = s_wl;
        if (tot == 0) return 0xFFFFFFFFu;                      // (uniform)
        if (tid == 0) {
            uint32_t base = atomicAdd(&wl_count[b], tot);
            if (base + tot > wl_cap) { atomicOr(&flag[b], 4u); base = 0xFFFFFFFFu; }   // list full: block flagged
            s_deep = base;
        }
        __syncthreads();
        return s_deep;
    };
    auto wl_entry = [&](uint32_t base, uint64_t wv, uint32_t pos, uint32_t grp) __attribute__((always_inline)) {
        uint4 *WL = wl + (size_t)b * wl_cap;
        const uint32_t gp = grp >> 16, gs = grp & 0xFFFFu, slot0 = base + reinterpret_cast<const uint32_t *>(s_w)[2 * gp + 1];
        WL[slot0 + (pos - gp)] = make_uint4((uint32_t)(wv & FS_LOW_MASK), R0 + gp, slot0, gs);
    };

    // ---- FULL full rounds, FULL + 1 slots, phase-major ----
    auto rounds = [&](auto full_t) __attribute__((always_inline)) -> bool {
        constexpr int FULL = decltype(full_t)::value, NS = FULL + 1;
        static_assert(FULL >= FSS_SPEC && NS <= FSS_ITEMS, "the requested rounds are all full ones");
        uint64_t w[NS];
        w[0] = ~0ull;
        if (v0) w[0] = K[i0];
#pragma unroll
        for (int r = 1; r <= FULL; r++) w[r] = r <= FSS_SPEC ? ws[r <= FSS_SPEC ? r : 0] : K[(r - 1) * FSS_NT + tid];
        if (tid < FSS_SENT) s_w[cc + tid] = ~0ull;             // what the rank step reads past the last bin compares as larger
        __syncthreads();
        if (s_deep) return false;                              // flagged: the block is another sorter's
        // 1. counting sort on the 12 bits below the bucket number (arrival order inside a bin: any order will do)
        uint32_t bin[NS], rk[NS];
#pragma unroll
        for (int r = 0; r < NS; r++) bin[r] = ((uint32_t)(w[r] >> 32) >> hshift) & (FS_BINS - 1);
        rk[0] = 0;
        if (v0) rk[0] = atomicAdd(&s_cp[bin[0] >> 1], 1u << (16 * (bin[0] & 1)));
#pragma unroll
        for (int r = 1; r < NS; r++) rk[r] = atomicAdd(&s_cp[bin[r] >> 1], 1u << (16 * (bin[r] & 1)));
#pragma unroll
        for (int r = 0; r < NS; r++) rk[r] = (rk[r] >> (16 * (bin[r] & 1))) & 0xFFFFu;
        __syncthreads();
        bin_starts();
        __syncthreads();
        {
            // the words that arrived fifth and later in their bin (3e-4 of them) flag it as big: the rank step then needs the
            // bin's start only.  The starts are read masked: a flag may or may not be in yet.
            uint32_t st[NS];
            st[0] = 0;
            if (v0) st[0] = s16[bin[0]];
#pragma unroll
            for (int r = 1; r < NS; r++) st[r] = s16[bin[r]];
            bool late = false;
#pragma unroll
            for (int r = 0; r < NS; r++) late |= rk[r] >= FSS_LOOK;
            if (late) {
#pragma unroll
                for (int r = 0; r < NS; r++)
                    if (rk[r] >= FSS_LOOK) atomicOr(&s_cp[bin[r] >> 1], FS_BIG_BIN << (16 * (bin[r] & 1)));
            }
#pragma unroll
            for (int r = 0; r < NS; r++) rk[r] += st[r] & FS_START_MASK;
            if (v0) s_w[rk[0]] = sorted_word(w[0]);
        }
#pragma unroll
        for (int r = 1; r < NS; r++) s_w[rk[r]] = sorted_word(w[r]);
        __syncthreads();
        // 2. final position = bin start + number of smaller codes in the bin (thread = the words at positions i0 / (r - 1) NT +
        //    tid of the bin-sorted array).  The four words from the bin start are compared in straight-line code with no bounds
        //    at all -- what lies behind the bin's end is a larger code or a sentinel; a bin of more than four (flagged in its
        //    start entry: the bin's end is not read here), or a second word with my code among the four, is the rare case:
        //    detected per wave, redone exactly with a second look at the next four keys (rank_rare2).
        uint32_t pos[NS], grp[NS], gs[NS];                     // grp = group start << 16 | group size (0: not tied)
        bool big[NS];                                          // the bin holds more than FSS_LOOK words
        if (v0) w[0] = s_w[i0];
#pragma unroll
        for (int r = 1; r < NS; r++) w[r] = s_w[(r - 1) * FSS_NT + tid];
        gs[0] = 0;
        if (v0) gs[0] = s16[((uint32_t)(w[0] >> 32) >> kshift) & (FS_BINS - 1)];
#pragma unroll
        for (int r = 1; r < NS; r++) gs[r] = s16[((uint32_t)(w[r] >> 32) >> kshift) & (FS_BINS - 1)];
#pragma unroll
        for (int r = 0; r < NS; r++) { big[r] = gs[r] > FS_START_MASK; gs[r] &= FS_START_MASK; }   // (the bin's end is read in the rare case only)
        uint32_t kq[NS][FSS_LOOK];
        if (v0) {
            const uint32_t *B = reinterpret_cast<const uint32_t *>(s_w) + 2 * gs[0] + 1;
#pragma unroll
            for (uint32_t t = 0; t < FSS_LOOK; t++) kq[0][t] = B[2 * t];
        }
#pragma unroll
        for (int r = 1; r < NS; r++) {
            const uint32_t *B = reinterpret_cast<const uint32_t *>(s_w) + 2 * gs[r] + 1;
#pragma unroll
            for (uint32_t t = 0; t < FSS_LOOK; t++) kq[r][t] = B[2 * t];
        }
        bool rare[NS], rare_any = false;
#pragma unroll
        for (int r = 0; r < NS; r++) {
            const uint32_t key = (uint32_t)(w[r] >> 32);       // inside a bin only the low 32 bits of the code can differ
            uint32_t less = 0, eqt = 0;
#pragma unroll
            for (uint32_t t = 0; t < FSS_LOOK; t++) {
                less += kq[r][t] < key ? 1u : 0u;
                eqt += kq[r][t] == key ? 1u : 0u;
            }
            pos[r] = gs[r] + less; grp[r] = 0;
            rare[r] = (big[r] | (eqt > 1)) & (r > 0 || v0);
            rare_any |= rare[r];
        }
        if (__builtin_amdgcn_ballot_w64(rare_any) != 0) {      // (wave-uniform)
#pragma unroll
            for (int r = 0; r < NS; r++)
                if (rare[r]) rank_rare2((uint32_t)(w[r] >> 32), r ? (r - 1) * FSS_NT + tid : i0, gs[r], kq[r], pos[r], grp[r]);
        }
        if (zb) {
            asm volatile("" ::: "memory");                     // (keeps the search behind the branch: see the header)
#pragma unroll
            for (int r = 0; r < NS; r++)
                if ((r > 0 || v0) && pos[r] != 0xFFFFFFFFu && ((uint32_t)w[r] & 0x0FFFFF00u) == 0 && !grp[r]) d_index[b] = (int)(R0 + pos[r]);
        }
        __syncthreads();                                       // s_cp (bin starts) is dead from here: it takes the BWT bytes
        if (s_deep) { if (tid == 0) atomicOr(&flag[b], 2u); return false; }
        if (v0) s_cb[shift + pos[0]] = (uint8_t)w[0];          // (rows of tied groups are rewritten by k_fs_ties)
#pragma unroll
        for (int r = 1; r < NS; r++) s_cb[shift + pos[r]] = (uint8_t)w[r];
        uint32_t tied = 0;
#pragma unroll
        for (int r = 0; r < NS; r++) tied |= grp[r];
        if (tied) {
#pragma unroll
            for (int r = 0; r < NS; r++)
                if (grp[r]) wl_reserve(pos[r], grp[r]);
        }
        const uint32_t base = wl_base();
        if (base != 0xFFFFFFFFu && tied) {
#pragma unroll
            for (int r = 0; r < NS; r++)
                if (grp[r]) wl_entry(base, w[r], pos[r], grp[r]);
        }
        return true;
    };

    // ---- any fill: eight slots, every one of them guarded ----
    auto guarded = [&]() __attribute__((always_inline)) -> bool {
        uint64_t w[FSS_ITEMS];
#pragma unroll
        for (int r = 0; r < FSS_ITEMS; r++) w[r] = r >= 1 && r <= FSS_SPEC ? ws[r >= 1 && r <= FSS_SPEC ? r : 0] : ~0ull;
        if (v0) w[0] = K[i0];
#pragma unroll
        for (int r = FSS_SPEC + 1; r < FSS_ITEMS; r++)
            if ((uint32_t)r <= full) w[r] = K[(r - 1) * FSS_NT + tid];
        if (tid < FSS_SENT && cc) s_w[cc + tid] = ~0ull;       // what the rank step reads past the last bin compares as larger
        __syncthreads();
        if (s_deep || cc == 0) return false;                   // flagged: the block is another sorter's
        // 1. counting sort
        uint32_t rk[FSS_ITEMS];
#pragma unroll
        for (int r = 0; r < FSS_ITEMS; r++) rk[r] = 0;
        {
            auto count = [&](int r) {
                const uint32_t bin = ((uint32_t)(w[r] >> 32) >> hshift) & (FS_BINS - 1), sh = 16 * (bin & 1);
                rk[r] = (atomicAdd(&s_cp[bin >> 1], 1u << sh) >> sh) & 0xFFFFu;
            };
            if (v0) count(0);
#pragma unroll
            for (int r = 1; r < FSS_ITEMS; r++)
                if ((uint32_t)r <= full) count(r);
        }
        __syncthreads();
        bin_starts();
        __syncthreads();
        {
            auto scatter = [&](int r) {
                const uint32_t bin = ((uint32_t)(w[r] >> 32) >> hshift) & (FS_BINS - 1);
                const uint32_t st = s16[bin];
                if (rk[r] >= FSS_LOOK) atomicOr(&s_cp[bin >> 1], FS_BIG_BIN << (16 * (bin & 1)));   // (see rounds<>)
                s_w[(st & FS_START_MASK) + rk[r]] = sorted_word(w[r]);
            };
            if (v0) scatter(0);
#pragma unroll
            for (int r = 1; r < FSS_ITEMS; r++)
                if ((uint32_t)r <= full) scatter(r);
        }
        __syncthreads();
        // 2. final position, item by item
        uint32_t pos[FSS_ITEMS], grp[FSS_ITEMS];               // grp = group start << 16 | group size (0: not tied)
#pragma unroll
        for (int r = 0; r < FSS_ITEMS; r++) { pos[r] = 0xFFFFFFFFu; grp[r] = 0; }
        {
            auto rank = [&](int r, uint32_t p) {
                const uint64_t wv = s_w[p];
                w[r] = wv;
                const uint32_t key = (uint32_t)(wv >> 32);     // inside a bin only the low 32 bits of the code can differ
                const uint32_t bin = (key >> kshift) & (FS_BINS - 1);
                const uint32_t gf = s16[bin], gs = gf & FS_START_MASK;
                uint32_t less = 0, eqt = 0, kq[FSS_LOOK];
                const uint32_t *B = reinterpret_cast<const uint32_t *>(s_w) + 2 * gs + 1;
#pragma unroll
                for (uint32_t t = 0; t < FSS_LOOK; t++) {
                    kq[t] = B[2 * t];
                    less += kq[t] < key ? 1u : 0u;
                    eqt += kq[t] == key ? 1u : 0u;
                }
                uint32_t at = gs + less;
                const bool rare = (gf > FS_START_MASK) | (eqt > 1);
                if (__builtin_amdgcn_ballot_w64(rare) != 0) {  // (wave-uniform)
                    if (rare) rank_rare2(key, p, gs, kq, at, grp[r]);
                }
                pos[r] = at;
            };
            if (v0) rank(0, i0);
#pragma unroll
            for (int r = 1; r < FSS_ITEMS; r++)
                if ((uint32_t)r <= full) rank(r, (r - 1) * FSS_NT + tid);
            if (zb) {
                asm volatile("" ::: "memory");                 // (keeps the search behind the branch: see the header)
#pragma unroll
                for (int r = 0; r < FSS_ITEMS; r++)
                    if (pos[r] != 0xFFFFFFFFu && ((uint32_t)w[r] & 0x0FFFFF00u) == 0 && !grp[r]) d_index[b] = (int)(R0 + pos[r]);
            }
        }
        __syncthreads();                                       // s_cp (bin starts) is dead from here: it takes the BWT bytes
        if (s_deep) { if (tid == 0) atomicOr(&flag[b], 2u); return false; }
#pragma unroll
        for (int r = 0; r < FSS_ITEMS; r++) {
            if (pos[r] != 0xFFFFFFFFu) s_cb[shift + pos[r]] = (uint8_t)w[r];      // (rows of tied groups are rewritten by k_fs_ties)
            if (grp[r]) wl_reserve(pos[r], grp[r]);
        }
        const uint32_t base = wl_base();
        if (base != 0xFFFFFFFFu) {
#pragma unroll
            for (int r = 0; r < FSS_ITEMS; r++)
                if (grp[r]) wl_entry(base, w[r], pos[r], grp[r]);
        }
        return true;
    };

    // (wave-uniform; neighbouring workgroups of a Zipf block take different instances about half the time)
    const bool go = full == 3 ? rounds(std::integral_constant<int, 3>{}) : full == 4 ? rounds(std::integral_constant<int, 4>{}) : guarded();
    if (!go) return;
    // 4. the rows
    // (Whole dwords in straight-line code, two per thread at most, and the ragged ends by eight lanes: measured, 5.04-5.11 ms
    // per launch against this loop's 4.95-5.02, profiles/sort_entry.md.)
    {
        const uint32_t end = shift + c;                        // staged bytes [shift, end)
        for (uint32_t q = tid; 4 * q < end; q += FSS_NT) {
            const uint32_t v = s_cp[q];
            if (4 * q >= shift && 4 * q + 4 <= end) *reinterpret_cast<uint32_t *>(O - shift + 4 * q) = v;
            else {
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    if (4 * q + k >= shift && 4 * q + k < end) O[4 * q + k - shift] = (uint8_t)(v >> (8 * k));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// groups of equal codes: one thread per member counts the members whose suffix is smaller (text comparison,
// 8 bytes at a time) and writes its row.  Equal codes do not certify equal symbols: the comparison starts at
// the first symbol.
// ---------------------------------------------------------------------------
#ifndef GLC_FST_W
#define GLC_FST_W 4
#endif
constexpr int FST_W = GLC_FST_W;                              // k_fs_ties: members of a run met at a time
__global__ __launch_bounds__(256) void k_fs_ties(const uint8_t *__restrict__ text, size_t stride, uint32_t n,
                                                 const uint4 *__restrict__ wl, uint32_t wl_cap,
                                                 const uint32_t *__restrict__ wl_count, uint32_t *__restrict__ flag,
                                                 uint8_t *__restrict__ bwt_out, size_t bwt_stride,
                                                 int *__restrict__ d_index, uint32_t *__restrict__ sa_out, size_t sa_stride)
{
    uint32_t gx, gy;
    xcd_order(gx, gy);                                         // a block's text in one L2 for the comparisons
    const uint32_t b = gy;
    const uint32_t total = wl_count[b];
    if (total == 0 || total > wl_cap || flag[b]) return;       // (flags of this pass are all set before it starts)
    const uint4 *WL = wl + (size_t)b * wl_cap;
    const uint8_t *T = text + (size_t)b * stride;
    for (uint32_t e = gx * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
        const uint4 me = WL[e];
        const uint32_t gs = me.w, idx = me.x >> 8;
        uint32_t rank = 0;
        bool deep = false;
        // four members at a time: their list entries, then their first 8 text bytes, are loaded together (a member of a
        // run of 100 equal codes would otherwise wait for 200 memory round trips one after the other); only a pair
        // that agrees in those 8 bytes, or sits at the end of the block, takes the byte-exact loop
        const bool fast_me = idx + 12 <= n;
        const uint64_t mine = fast_me ? fs_load_be64(T + idx) : 0ull;
        for (uint32_t f0 = me.z; f0 < me.z + gs && !deep; f0 += FST_W) {
            uint32_t oi[FST_W];
            uint64_t ov[FST_W];
#pragma unroll
            for (int k = 0; k < FST_W; k++) oi[k] = f0 + k < me.z + gs ? WL[f0 + k].x >> 8 : idx;
#pragma unroll
            for (int k = 0; k < FST_W; k++) ov[k] = (oi[k] != idx && fast_me && oi[k] + 12 <= n) ? fs_load_be64(T + oi[k]) : mine;
#pragma unroll
            for (int k = 0; k < FST_W; k++) {
                if (oi[k] == idx) continue;                    // myself, or past the end of the run
                if (fast_me && oi[k] + 12 <= n && ov[k] != mine) rank += ov[k] < mine ? 1u : 0u;
                else rank += fs_suffix_less(T, n, oi[k], idx, &deep) ? 1u : 0u;
            }
        }
        if (deep) { atomicOr(&flag[b], 2u); continue; }
        const uint32_t row = me.y + rank;
        if (bwt_out) bwt_out[(size_t)b * bwt_stride + row] = (uint8_t)me.x;
        if (sa_out) sa_out[(size_t)b * sa_stride + row] = idx;
        if (idx == 0 && d_index) d_index[b] = (int)row;
    }
}

// blocks the fast path gave up on -> live counts for the general sorter
// (`redo` is a per-call copy of the flags for the stages queued speculatively behind the sort: under stage
//  pipelining the next call clears `flag` while they may still be reading)
// nflag[0] = flagged blocks; nflag[3] = ticket of this launch's workgroups: the last one stores the count where the host reads
// it (h_nflag: pinned, device-mapped) -- a copy command behind the pass was one more launch in every call
// nflag[4] = blocks the text-likeness probe did NOT call text-like (constant blocks apart): h_nflag[1].  The host's streak of
// "every block of the call was text-like" (sa_build_begin: small calls skip the bucket sorter's attempt while it lasts) ends
// with the first such block, also in a call that skipped.
__global__ void k_fs_finish(const uint32_t *__restrict__ flag, uint32_t n, uint32_t nblk, uint32_t *__restrict__ lcnt,
                            uint32_t *__restrict__ nflag, uint32_t *__restrict__ redo, uint32_t *__restrict__ keep,
                            uint32_t *__restrict__ list, uint32_t *__restrict__ h_nflag, const uint32_t *__restrict__ dup,
                            uint32_t dup_flag)
{
    __shared__ uint32_t s_last;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nblk) {
        const uint32_t f = (flag[b] && flag[b] != FS_DONE) ? n : 0u;    // (FS_DONE: a constant block, finished by k_fs_tables)
        lcnt[b] = f;
        redo[b] = f;
        keep[b] = f ? 0u : 1u;
        if (f) list[atomicAdd(nflag, 1u)] = b;                 // (any order)
        if (flag[b] != FS_DONE && dup[b] < dup_flag) atomicAdd(nflag + 4, 1u);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&nflag[3], 1u) == gridDim.x - 1 ? 1u : 0u;
    __syncthreads();
    if (s_last && threadIdx.x == 0) {
        __threadfence();
        reinterpret_cast<volatile uint32_t *>(h_nflag)[1] = atomicAdd(nflag + 4, 0u);
        *reinterpret_cast<volatile uint32_t *>(h_nflag) = atomicAdd(nflag, 0u);
        __threadfence_system();
    }
}

// everything the pass accumulates into, cleared by ONE launch (six hipMemsetAsync calls were six dispatches of ~2 us with
// ~8 us between them: 90 us of a 1 MiB call that takes 400)
__global__ __launch_bounds__(256) void k_fs_clear(uint32_t nblk, uint32_t *__restrict__ hist, uint32_t *__restrict__ fill,
                                                  uint32_t *__restrict__ flag, uint32_t flag_value, uint32_t *__restrict__ wlcnt,
                                                  uint32_t *__restrict__ dup, uint32_t *__restrict__ nflag)
{
    const uint32_t nh = nblk * 256u, nf = nblk * FS_MAXNB, total = nh + nf + 3u * nblk + 8u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        if (i < nh) hist[i] = 0;
        else if (i < nh + nf) fill[i - nh] = 0;
        else {
            const uint32_t j = i - nh - nf;
            if (j < nblk) flag[j] = flag_value;
            else if (j < 2 * nblk) wlcnt[j - nblk] = 0;
            else if (j < 3 * nblk) dup[j - 2 * nblk] = 0;
            else nflag[j - 3 * nblk] = 0;                       // [0] flagged blocks, [1] [2] the sample sorter's, [3] k_fs_finish's ticket, [4] blocks the probe did not call text-like
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// k_fs_scan for the sample sorter's pass (bwt_sample.hip): the blocks of `list`
hipError_t fs_scan(hipStream_t st, uint32_t nlisted, const uint32_t *fill, uint32_t *fbase, uint32_t *flag, const uint32_t *list)
{
    hipLaunchKernelGGL(k_fs_scan, dim3(nlisted), dim3(FS_MAXNB), 0, st, fill, fbase, flag, list);
    return hipGetLastError();
}

hipError_t fs_build(const SortCall &c, SaScratch &s)
{
    const hipStream_t st = c.st;
    const uint8_t *const text = c.text;
    const size_t text_stride = c.text_stride, bwt_stride = c.bwt_stride;
    const uint32_t n = c.n, nblk = c.nblk;
    uint8_t *const bwt_out = c.bwt_out;
    int *const d_index = c.d_index;
    uint32_t *const sa_out = c.sa_out(s);
    const uint32_t nbl = fs_bucket_log2(n), nb = 1u << nbl;
    {
        const uint32_t words = nblk * (256u + FS_MAXNB + 3u) + 8u, g = (words + 1023) / 1024;
        // (skip_tier1: every block starts flagged -- no attempt, the sample sorter takes them all)
        hipLaunchKernelGGL(k_fs_clear, dim3(g < 2048 ? g : 2048), dim3(256), 0, st, nblk, s.fs_hist, s.fs_fill, s.fs_flag,
                           s.skip_tier1 ? 1u : 0u, s.fs_wlcnt, s.fs_dup, s.fs_nflag);
    }
    uint32_t *h_nflag = s.h_max_cnt + HW_FLAGGED;              // pinned, device-mapped: written (with HW_NOT_TEXTLIKE behind it) by the kernel that finishes the pass
    const double units = (double)n * nblk;
    // statistics from every 4th 32 KB slice of a block of 512 KiB or more (the pass reads a quarter of the input: 0.27 -> 0.07 ms
    // per GiB)
    const uint32_t nslices = (n + FSH_SLICE - 1) / FSH_SLICE;
    const uint32_t hstep = nslices >= 16 ? 4u : 1u;
    {
        ProfScope ps(s.prof, PROF_FS_HIST, st, units);
        hipLaunchKernelGGL(k_fs_hist, dim3((nslices + hstep - 1) / hstep, nblk), dim3(256), 0, st, text, text_stride, n,
                           s.fs_hist, s.fs_dup, hstep);
    }
    hipLaunchKernelGGL(k_fs_tables, dim3(nblk), dim3(256), 0, st, s.fs_hist, n, s.fs_tab, s.fs_dup, s.fs_flag, text, text_stride,
                       bwt_out, bwt_stride, d_index, sa_out, (size_t)s.nmax, hstep);
    if (s.skip_tier1) {
        // sorter mode 4, or a small call behind a streak of all-text-like calls: no attempt, every block goes to the sample sorter
        hipLaunchKernelGGL(k_fs_finish, dim3((nblk + 255) / 256), dim3(256), 0, st, s.fs_flag, n, nblk, s.fs_lcnt, s.fs_nflag,
                           s.fs_redo[s.parity & 1], s.fs_keep[s.parity & 1], s.ss_list, h_nflag, s.fs_dup, (FS_DUP_FLAG + hstep - 1) / hstep);
        return hipGetLastError();
    }
    // (The 8-byte suffix words of a block make one round trip through memory between k_fs_part2 and k_fs_sort -- 16 of the
    // encoder's 26 bytes of HBM traffic per input byte when a call's words, 8 MiB per block, are far more than the 256 MB
    // Infinity Cache holds.  The whole call is bucketed, then sorted.)
    // tiles of 4096 suffixes, per workgroup: 4 for a few blocks, 1 for one to three (more workgroups for a block on its own).  Round 5, bench.py
    // `value` on one box, 1024-block batches, stage overlap on: 4 / 8 / 12 / 16 / 24 / 32 / 64 tiles -> 93.1 / 95.1 / 94.7 /
    // 95.1 / 95.6 / 93.8 / 87-94 GB/s (16 and 24 fall into two modes from run to run: 94.3-96.5); the kernel itself 3.0 ->
    // 2.9 ms per GiB.  Tiles of 8192 suffixes (1024 threads x 8, 64 KB of LDS, one workgroup per CU: runs of ~128 bytes, half
    // the global atomics) run 2.7 ms -- and give the same `value` as 4 tiles of 4096: a 1024-thread workgroup needs half a CU
    // free AT ONCE, which the MTF and Huffman kernels of the batch before, sharing the chip under stage overlap, rarely leave.
    // Batches of 16 blocks or more: tiles of 8192 suffixes, 1024 threads (runs of ~128 bytes leave for a bucket's slot, half the
    // global atomics), 16 tiles per workgroup.  70 KB of LDS would let two workgroups share a CU, but the registers (76 VGPRs:
    // six waves per SIMD) hold it to ONE.  Squeezed to 64 VGPRs with amdgpu_waves_per_eu(8, 8) (4 spilled) for two per CU, it
    // gave bench.py `value` 105.7-106.5 GB/s against 108.5-109.3 on one box, alternating.  Until the MTF kernel was re-based this
    // shape ran 2.7 ms and gave the same `value` (the stages of the batch before rarely left half a CU free at once); since:
    // alternating on one box, 6 steps: 100.2 / 101.7 / 102.0 GB/s as it was, 102.3 / 102.9 / 103.0 so (8 tiles per workgroup:
    // 102.3 / 102.5 / 102.7); stages back to back 97.8-99.8 -> 101.2-101.7; the kernel 2.91-3.10 -> 2.67-2.73 ms per GiB.
    // (512 threads x 16 suffixes for the same tile: 3.3 ms.)
    {
        ProfScope ps(s.prof, PROF_FS_PART, st, units);
        if (nblk >= 16) {
#ifndef GLC_FSP2_BT
#define GLC_FSP2_BT 8192
#endif
            constexpr int BT = GLC_FSP2_BT, BN = 1024;
            const uint32_t tiles = (n + BT - 1) / BT, per = 16;
            hipLaunchKernelGGL((k_fs_part2<BN, BT / BN, 4>), dim3((tiles + per - 1) / per, nblk), dim3(BN), 0, st, text, text_stride, n, nbl,
                               s.fs_tab, s.keyA, s.fs_kstride, s.fs_fill, s.fs_flag, s.fs_zero, per);
        } else {
            const uint32_t tiles = (n + FSP2_TILE - 1) / FSP2_TILE;
            // (a call of one to three blocks: ONE tile per workgroup -- 256 workgroups for a block on its own: 17.3 -> 12.0 us of
            //  a single cudppCompress call's chain, 0.190 -> 0.182 ms per call)
            const uint32_t per = nblk >= 4 ? FSP2_T : 1u;
            hipLaunchKernelGGL((k_fs_part2<FSP2_NT, FSP2_TILE / FSP2_NT, GLC_FSP2_WAVES>), dim3((tiles + per - 1) / per, nblk), dim3(FSP2_NT), 0, st,
                               text, text_stride, n, nbl, s.fs_tab, s.keyA, s.fs_kstride, s.fs_fill, s.fs_flag, s.fs_zero, per);
        }
    }
    hipLaunchKernelGGL(k_fs_scan, dim3(nblk), dim3(FS_MAXNB), 0, st, s.fs_fill, s.fs_base, s.fs_flag, (const uint32_t *)nullptr);
    {
        ProfScope ps(s.prof, PROF_FS_SORT, st, units);
        if (sa_out || !bwt_out || !d_index)                    // the suffix array itself is asked for: the kernel that writes it
            hipLaunchKernelGGL(k_fs_sort, dim3(nb, nblk), dim3(FSS_NT), 0, st, n, nbl, s.keyA, s.fs_kstride, s.fs_fill, s.fs_base, s.fs_flag,
                               bwt_out, bwt_stride, d_index, sa_out, (size_t)s.nmax, s.fs_wl, s.fs_wl_cap, s.fs_wlcnt);
        else {
            // the kernel finds its bucket and block by shift and mask (xcd_order_pow2): right only for a grid x of exactly
            // 1 << nbl with nbl >= 3.  fs_bucket_log2 gives 4 .. 9 today; a rule that gives less fails here, not in the rows
            if (nbl < 3 || nb != 1u << nbl) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_fs_sort_bwt, dim3(nb, nblk), dim3(FSS_NT), 0, st, nbl, s.keyA, s.fs_kstride, s.fs_fill, s.fs_base, s.fs_flag,
                               bwt_out, bwt_stride, d_index, s.fs_wl, s.fs_wl_cap, s.fs_wlcnt, s.fs_zero);
        }
    }
    hipLaunchKernelGGL(k_fs_ties, dim3(24, nblk), dim3(256), 0, st, text, text_stride, n, s.fs_wl, s.fs_wl_cap, s.fs_wlcnt,
                       s.fs_flag, bwt_out, bwt_stride, d_index, sa_out, (size_t)s.nmax);
    hipLaunchKernelGGL(k_fs_finish, dim3((nblk + 255) / 256), dim3(256), 0, st, s.fs_flag, n, nblk, s.fs_lcnt, s.fs_nflag,
                       s.fs_redo[s.parity & 1], s.fs_keep[s.parity & 1], s.ss_list, h_nflag, s.fs_dup, (FS_DUP_FLAG + hstep - 1) / hstep);
    return hipGetLastError();
}

} // namespace glc
