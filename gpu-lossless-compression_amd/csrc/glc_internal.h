// glc_internal.h -- host-side interfaces between the C-ABI layer (cudpp_api.cpp,
// culzss_api.cpp) and the stage launchers (*.hip).  Plain pointers + sizes.
#pragma once
#include "../../include/cudpp.h"
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <functional>

// Diagnostic switches change what a kernel does (extra stores, cycle stamps, debug counters): a library built with one is an
// experiment, never the product.  They compile only with -DGLC_EXPERIMENT_BUILD, and build.py writes such a library (any
// library built with GLC_CXXFLAGS) to GLC_LIB_OUT only -- libglc_amd.so is always the plain build.
#if (defined(GLC_DEBUG_CAND) || defined(GLC_SS_CLOCKS) || defined(GLC_HB_TIMING)) && !defined(GLC_EXPERIMENT_BUILD)
#error "diagnostic switches need -DGLC_EXPERIMENT_BUILD (and GLC_LIB_OUT: build.py never writes libglc_amd.so from such a build)"
#endif

// in a launcher that returns hipError_t: pass a failed call's error on
#define GLC_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)
// in an entry point that returns CUDPPResult: a failed call's error as the result code
#define CT_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return glc::hip_result(e_); } while (0)

namespace glc {

// what the C ABI answers for a HIP error (cudpp_api.cpp); a failure also clears HIP's sticky last error
CUDPPResult hip_result(hipError_t e);

// ---------------------------------------------------------------------------
// Scratch allocation.  Every device and pinned-host block the library allocates for itself comes from one of the three
// helpers below (tests/test_cpu_alloc_sites.py holds csrc/ to that); buffers the caller owns are never touched.  What a block
// holds when it arrives is whatever the allocator left there, and the library's results must not depend on it: the fill seam
// (glcDebugSetScratchFill, cudpp.h) lets a test choose those contents.  While it is on, each block is filled whole
// with a 32-bit word (tail bytes included) before the helper returns, and the fill has completed by then.  Off -- the
// default -- costs the one branch below.  Process-wide, a debugging aid: not safe against concurrent allocation.
// ---------------------------------------------------------------------------
struct ScratchFill { unsigned on = 0, word = 0; unsigned long long blocks = 0, bytes = 0; };
extern ScratchFill g_scratch_fill;               // cudpp_api.cpp
hipError_t scratch_fill(void *p, size_t bytes, bool pinned, hipStream_t st);   // cudpp_api.cpp
inline hipError_t glc_dev_alloc(void **p, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess && g_scratch_fill.on ? scratch_fill(*p, bytes, false, nullptr) : e;
}
inline hipError_t glc_host_alloc(void **p, size_t bytes)   // pinned host memory (hipHostMallocDefault)
{
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    return e == hipSuccess && g_scratch_fill.on ? scratch_fill(*p, bytes, true, nullptr) : e;
}
inline hipError_t glc_dev_alloc_async(void **p, size_t bytes, hipStream_t st)   // stream-ordered; freed with hipFreeAsync
{
    const hipError_t e = hipMallocAsync(p, bytes, st);
    return e == hipSuccess && g_scratch_fill.on ? scratch_fill(*p, bytes, false, st) : e;
}

constexpr uint32_t MAX_BLOCK_ELEMS = 1u << 20;   // cudppCompress/BWT limit (cudpp-inpar/README.md:96,99)
constexpr uint32_t HUFF_BLOCK      = 4096;       // HUFF_THREADS_PER_BLOCK*HUFF_WORK_PER_THREAD (cudpp_globals.h:60-61)
constexpr uint32_t HUFF_SYMS       = 257;        // HUFF_NUM_CHARS (cudpp_globals.h:62)
constexpr uint32_t HUFF_MAX_WORDS  = 1536;       // HUFF_CODE_BYTES (cudpp_globals.h:66)
constexpr uint32_t MTF_CHUNK       = 4096;       // bytes of BWT output per wave in the MTF kernels
// Histogram of a 4096-symbol sub-block (HuffScratch::sub_hist): no count passes 4096, so a count is a 16-bit half.  Dword j
// holds rank j in its low half and rank j + 128 in its high half (the layout of k_mtf_encode's LDS counters, which leave as
// they stand).  A block's total reaches 2^20: k_huff_build unpacks before it adds.  (GLC_SUBHIST_WIDE: A/B, a dword per count)
#ifdef GLC_SUBHIST_WIDE
constexpr uint32_t SUBHIST_DWORDS  = 256;
#else
constexpr uint32_t SUBHIST_DWORDS  = 128;
#endif
constexpr bool     SUBHIST_PACKED  = SUBHIST_DWORDS == 128;

// fast suffix sorters (bwt_bucket.hip, bwt_sample.hip): buckets of FS_AVG suffixes on average, FS_CAP words of slot each
constexpr uint32_t FS_AVG   = 2048;
constexpr uint32_t FS_CAP   = 4096;             // slot size in the word array
constexpr uint32_t FS_FILLMAX = 4032;            // fullest bucket the in-LDS sort takes (a fuller one flags its block)
constexpr uint32_t FS_MAXNB = 512;               // buckets per block at n = 2^20 (256 buckets of 4096 words: k_fs_sort 1.62 vs 1.3 ms)
constexpr uint32_t FS_MAXNB_LOG2 = 9;
// periodic tier (bwt_periodic.hip): blocks that are one periodic stretch with a period of up to PER_PMAX symbols
constexpr uint32_t PER_PMAX = 4096;
constexpr uint32_t PER_TAKE = 256;                   // blocks of one call the periodic tier takes (its scratch, ~140 KB per slot, is sized by this, not by the plan's rows)
constexpr uint32_t PER_Z    = 2;                     // the explicit zone before the break is PER_Z * L symbols wide (bwt_periodic.hip: why 2)
constexpr uint32_t PER_NU   = (2 * PER_Z + 3) * PER_PMAX + 32;   // bytes of the text of representatives: Z L + 2 p + 1 | separator | Z L + t | padding
// L: the multiple of the period p that covers the longer of the period and the tail t
inline __host__ __device__ uint32_t per_span(uint32_t p, uint32_t t) { const uint32_t m = t > p ? t : p; return p * ((m + p - 1) / p); }
inline __host__ __device__ uint32_t per_text_len(uint32_t p, uint32_t t) { return 2 * PER_Z * per_span(p, t) + 2 * p + 2 + t; }
constexpr uint32_t FS_LCP_CAP = 512;             // suffix comparisons and the sample sorter's rounds give up behind this many symbols
#ifndef GLC_SS_TOL_CAP
#define GLC_SS_TOL_CAP 64                        // (128 until round 6.  With chain groups and the capped direct count the doubling rounds are cheap
#endif                                           //  enough to start earlier: a periodic stretch inside Zipf data 6.4 -> 5.5 ms per 32 blocks, bench.py's
                                                 //  partly_deep batch 9.15 -> 8.93 per 64; 48: 5.3 / 9.0, 32: 5.1 / 9.7, 256: 8.1 / 10.2)
constexpr uint32_t SS_TOL_CAP = GLC_SS_TOL_CAP;  // ... and in the sample sorter's tolerant form STOP behind this many: prefix doubling takes over from there (a multiple of 8)
constexpr uint32_t GRP_SAME = 0x80000000u;        // ... this row continues the group of the row before it (k_grp_flags' result; set up front for the members of a run left at the cap)
constexpr uint32_t SA_CAND = 0x40000000u;         // tolerant form, in the rows of s.sa: this row may share SS_TOL_CAP symbols with the row before it (it was still in a
                                                  // run at that depth, or it is a bucket's first row); every other row was told from its neighbours by fewer
#ifndef GLC_SS_LONG
#define GLC_SS_LONG 256
#endif
constexpr uint32_t SS_LONG = GLC_SS_LONG;        // sample sorter: a run of more positions is cut with pivots (k_ss_long), a shorter one counted out (k_ss_windows)
#ifndef GLC_SSL_SMALL
#define GLC_SSL_SMALL 1024
#endif
constexpr uint32_t SSL_PER_BUCKET = FS_FILLMAX / (SS_LONG + 1), SSL_BIG_PER_BUCKET = FS_FILLMAX / (GLC_SSL_SMALL + 1);   // most bins of > SS_LONG / > 1024 members a bucket of <= 4032 can have
static_assert(SSL_PER_BUCKET < 64, "k_ss_cut lists a bucket's long bins with one wave");

// status bits accumulated on the device (PlanBase::d_status)
constexpr uint32_t ST_BLOCK_OVERFLOW = 1u;       // a 4096-symbol block needs > 1536 words
constexpr uint32_t ST_CAPACITY       = 2u;       // compressed stream would not fit its stride
constexpr uint32_t ST_CORRUPT        = 4u;       // decoder: an offset, length or row index of the stream is out of range

// ---------------------------------------------------------------------------
// live per-kernel profile (glcPlanEnableTiming(plan, 3)): hipEvent pairs recorded on the launch stream around
// the launches of the named kernels; durations are folded in when the plan's streams are idle
// ---------------------------------------------------------------------------
enum ProfSlot { PROF_FS_PART = 0, PROF_FS_SORT, PROF_MTF_ENCODE, PROF_HUFF_PACK, PROF_RS_ONESWEEP8, PROF_FS_HIST,
                PROF_MTF_LISTS, PROF_HUFF_BUILD,
                // decoder (decode.hip)
                PROF_DEC_HUFF, PROF_IMTF_POS, PROF_IMTF_REST, PROF_IBWT_LF, PROF_IBWT_WALK, PROF_IBWT_EMIT,
                // batched order-0 Huffman (hd_batch.hip): the container's HUFF0 codec
                PROF_HDB_HIST, PROF_HDB_TABLE, PROF_HDB_COUNT, PROF_HDB_SCAN, PROF_HDB_PACK, PROF_HDB_SPANS, PROF_HDB_EMIT,
                PROF_NSLOT };
struct KernelProf {
    static constexpr int NPAIR = 4096;
    bool       on = false;
    const char *name[PROF_NSLOT] = {"k_fs_part", "k_fs_sort", "k_mtf_encode", "k_huff_pack", "k_rs_onesweep<8,false>",
                                    "k_fs_hist", "k_mtf_chunk_lists+k_mtf_scan_lists", "k_huff_build",
                                    "k_dec_prepare+k_dec_huff", "k_imtf_pos", "k_imtf_scan+k_imtf_apply",
                                    "k_ibwt_hist+k_rs_scan+k_ibwt_lf", "k_ibwt_walk", "k_ibwt_rank+k_ibwt_emit",
                                    "k_hdb_hist", "k_hdb_table", "k_hdb_enc_count", "k_hdb_enc_scan", "k_hdb_enc_pack",
                                    "k_hdb_span_functions", "k_hdb_emit"};
    double     ms[PROF_NSLOT] = {}, units[PROF_NSLOT] = {};
    long       launches[PROF_NSLOT] = {};
    // event pairs and what they bracket: allocated when profiling is switched on (a plan that never profiles carries
    // none of it)
    hipEvent_t *ev = nullptr;                    // [2 * NPAIR]
    int        *pend_slot = nullptr;             // [NPAIR]
    double     *pend_units = nullptr;            // [NPAIR]
    int        npend = 0;
    long       dropped = 0;                      // launches not bracketed because NPAIR pairs were pending
    long       unread = 0;                       // pairs whose elapsed time could not be read at collect()
    bool enable(bool want)
    {
        if (want && !ev) {
            ev = (hipEvent_t *)calloc(2 * NPAIR, sizeof(hipEvent_t));
            pend_slot = (int *)calloc(NPAIR, sizeof(int));
            pend_units = (double *)calloc(NPAIR, sizeof(double));
            if (!ev || !pend_slot || !pend_units) { on = false; return false; }
        }
        on = want;
        return true;
    }
    int begin(int slot, hipStream_t st)
    {
        if (!on) return -1;
        if (npend >= NPAIR) { dropped++; return -1; }
        const int i = npend;
        for (int k = 0; k < 2; k++)
            if (!ev[2 * i + k] && hipEventCreate(&ev[2 * i + k]) != hipSuccess) return -1;
        pend_slot[i] = slot;
        (void)hipEventRecord(ev[2 * i], st);
        return i;
    }
    void end(int i, double nunits, hipStream_t st)
    {
        if (i < 0) return;
        (void)hipEventRecord(ev[2 * i + 1], st);
        pend_units[i] = nunits;
        npend = i + 1;
    }
    void collect()                               // the caller has synchronised every stream the events were recorded on
    {
        for (int i = 0; i < npend; i++) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]) == hipSuccess) {
                ms[pend_slot[i]] += t; units[pend_slot[i]] += pend_units[i]; launches[pend_slot[i]]++;
            } else unread++;
        }
        npend = 0;
    }
    void reset() { for (int k = 0; k < PROF_NSLOT; k++) { ms[k] = 0; units[k] = 0; launches[k] = 0; } npend = 0; dropped = 0; unread = 0; }
    ~KernelProf()
    {
        if (ev) for (int i = 0; i < 2 * NPAIR; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
        free(ev); free(pend_slot); free(pend_units);
    }
};

// The bracket around the launches of one slot: begins where it is declared, ends where its block does -- braces of their own
// where that must be before the next launch.  KernelProf::begin does not reserve its pair until end: two scopes must never be
// open at once on one profile.  A scope left early (a failed call inside it) still closes its pair.  pr may be null.
struct ProfScope {
    KernelProf *pr; hipStream_t st; double units; int i;
    ProfScope(KernelProf *p, int slot, hipStream_t s, double u) : pr(p), st(s), units(u), i(p ? p->begin(slot, s) : -1) {}
    ~ProfScope() { if (pr) pr->end(i, units, st); }
    ProfScope(const ProfScope &) = delete;
    ProfScope &operator=(const ProfScope &) = delete;
};

// C-ABI helper for the stateless device entry points (CULZSS, CUHD-shaped decoder), which have no plan to hang a profile
// on: a process-wide KernelProf with its own slot names.  out3 = {sum of launch ms, launches, units}; returns 0 past the
// last named slot.  Measurement aid: not thread-safe against concurrent launches.
inline int global_prof_get(KernelProf &pr, int nslot, int index, char *name, size_t name_cap, double *out3)
{
    if (index < 0 || index >= nslot || !out3) return 0;
    if (pr.npend) { (void)hipDeviceSynchronize(); pr.collect(); }
    out3[0] = pr.ms[index]; out3[1] = (double)pr.launches[index]; out3[2] = pr.units[index];
    if (name && name_cap) { size_t i = 0; for (; pr.name[index][i] && i + 1 < name_cap; i++) name[i] = pr.name[index][i]; name[i] = 0; }
    return 1;
}

// ---------------------------------------------------------------------------
// suffix array scratch: everything for `rows` blocks of up to nmax elements
// ---------------------------------------------------------------------------
// SaScratch::d_max_cnt, the general sorter's device counters, and the copy of them a doubling round reads back
enum RoundWord : uint32_t { RD_MAX = 0, RD_SUM,              // most and sum of the blocks' unresolved counts
                            RD_ERROR,                        // a look-back spin hit its bound
                            RD_REFINE_LIVE,                  // live suffixes of the blocks a refinement's tile-local sort could not finish
                            RD_CHAIN_CAND, RD_CHAIN_TAKEN,   // chain groups: candidates / ordered by the rule, every round so far
                            RD_WORDS };
// SaScratch::h_max_cnt, the pinned words: one name per meaning
enum HostWord : uint32_t {
    HW_ROUND = 0,                                // [RD_WORDS] a doubling round's copy of d_max_cnt
    HW_REFINE_LIVE = HW_ROUND + RD_WORDS,        // refine_sort: d_max_cnt[RD_REFINE_LIVE]
    HW_FLAGGED, HW_NOT_TEXTLIKE,                 // blocks the bucket sorter flagged / the probe did not call text-like: written by the pass's
                                                 // last kernel itself (k_fs_finish, through one pointer: the two stay neighbours)
    HW_GIVEN_UP,                                 // fs_nflag[1]: blocks the sample sorter has given up on so far
    HW_LISTED,                                   // fs_nflag[2]: blocks ss_retry_prepare listed or counted (second attempt, tolerant form)
    HW_PER_TAKEN, HW_PER_LONGEST,                // per_count[0 .. 1], one copy: blocks the periodic tier takes, bytes of their longest text of representatives
    HW_PER_DONE,                                 // per_count[2]: blocks the periodic tier finished
    HW_LEFT,                                     // host -> device: the staging word of sa_set_left
    HW_WORDS };
static_assert(HW_WORDS <= 16, "h_max_cnt is 16 words");

// the plan's last sa_build, for the glcPlanLastSort* getters
struct SortStats {
    uint32_t flagged = 0;                        // blocks the bucket sorter gave up on (all of them where it made no attempt)
    uint32_t retried = 0;                        // ... of which the sample sorter took in a second attempt (a bucket past its slot in the first)
    uint32_t general = 0;                        // ... of which the sample sorter gave up on too
    uint32_t periodic = 0;                       // ... of which the periodic tier finished
    uint32_t resumed = 0;                        // ... of which the doubling rounds RESUMED from the sample sorter's tolerant form
    uint32_t chains[2] = {0, 0};                 // chain groups ordered by the rule, candidates refused
    bool     skipped = false;                    // the call skipped the bucket sorter's attempt
};

struct SaScratch {
    uint32_t  nmax = 0, rows = 0, max_tiles = 0, rs_tiles = 0;
    uint64_t *keyA = nullptr, *keyB = nullptr;   // [rows][nmax]
    uint32_t *posA = nullptr, *posB = nullptr;   // [rows][nmax] SA slots of the unresolved list
    uint32_t *isa = nullptr;                     // [rows][nmax] rank+1 of each suffix
    uint32_t *sa = nullptr;                      // [rows][nmax]
    uint32_t *tile_hist = nullptr;               // [rows][rs_tiles][512] look-back granules of the radix passes
    uint32_t *digit_base = nullptr;              // [rows][5][512] exclusive digit offsets, one table per pass
    uint32_t *ghist = nullptr;                   // [rows][5][512] digit totals
    uint32_t  epoch = 255;                       // launch tag of the look-back granules (forces a clear first)
    uint64_t *tile_state = nullptr;              // [rows][max_tiles] look-back granules {flag:2, head:21, unres:21, groups:20}
    uint32_t *ticket = nullptr;                  // [rows] tile tickets of the single-pass rank kernel
    uint32_t *hdA = nullptr, *hdB = nullptr;     // [rows][nmax] SA slot of the group head of each unresolved entry
    uint32_t *cntA = nullptr, *cntB = nullptr;   // [rows] unresolved counts
    uint32_t *rl_flag = nullptr, *rl_cnt = nullptr;   // [rows] tile-local refinement: block needs the global sort / its count
    uint32_t *d_max_cnt = nullptr;               // [RD_WORDS] the general sorter's counters, by RoundWord
    uint32_t *h_max_cnt = nullptr;               // pinned [HW_WORDS]: what the host reads back (sa_read) or stages, by HostWord
    size_t    bytes = 0;
    bool      force_isa = false;                 // tests: skip text refinement, prefix doubling from round 1
    // chain groups of the doubling rounds (bwt_sa.hip k_chain_*): attempted in doubling round r where bit r of chain_rounds is
    // set and at least chain_min suffixes of the call are live (0: never); glcPlanSetChains, defaults from sa_chain_defaults
    long      chain_min = 16384;
    uint32_t  chain_rounds = 0x15;
    // fast path (bwt_bucket.hip, bwt_sample.hip); its words live in keyA/keyB (one allocation, fs_kstride words per block)
    int       sorter = 0;                        // 0 = bucket sorter, then sample sorter, then general sorter for what each flags;
                                                 // 1 = general sorter only; 2 = general sorter, prefix doubling only;
                                                 // 3 = bucket sorter, then general sorter (no sample sorter);
                                                 // 4 = sample sorter first (a caller that knows its data is text-like)
    size_t    fs_kstride = 0;
    uint32_t *fs_hist = nullptr;                 // [rows][256] symbol counts
    uint2    *fs_tab = nullptr;                  // [rows][256] {C, p} scaled to 2^32
    uint32_t *fs_fill = nullptr, *fs_base = nullptr;   // [rows][FS_MAXNB] bucket fill / rank base
    uint32_t *fs_flag = nullptr;                 // [rows] 1 = a bucket overflowed, 2 = deep (equal codes beyond the depth cap)
    uint32_t *fs_lcnt = nullptr;                 // [rows] n for flagged blocks, 0 otherwise
    uint32_t *fs_redo[2] = {nullptr, nullptr};   // [rows] copies of fs_lcnt, one per call parity (read by the speculative Huffman pass)
    uint32_t *fs_keep[2] = {nullptr, nullptr};   // [rows] 1 = the bucket sorter finished the block (the speculative stages' `only` mask)
    uint32_t *fs_dup = nullptr;                  // [rows] repeated 6-grams among the samples k_fs_hist looks at (text-likeness probe)
    uint32_t *fs_zero = nullptr;                 // [rows] bucket that holds the word of suffix 0 (k_fs_part2 -> k_fs_sort_bwt: the BWT index is looked for there only)
    uint32_t *fs_nflag = nullptr;                // 32 bytes, cleared by k_fs_clear: [0] blocks flagged by the bucket sorter; [1] given up on by the sample sorter;
                                                 // [2] listed for its second attempt / the tolerant form; [3] ticket of k_fs_finish's workgroups; [4] blocks the probe
                                                 // did not call text-like; [5 .. 7] unused
    uint4    *fs_wl = nullptr;                   // [rows][fs_wl_cap] runs of equal codes: {index << 8 | bwt, first row, first entry, size}
    uint32_t *fs_wlcnt = nullptr;                // [rows] entries in use
    uint32_t  fs_wl_cap = 0;
    uint32_t *ss_gtile = nullptr;                // [rows][ceil(nmax / 256)] group heads per tile of rows (k_grp_*)
    uint32_t *ss_cnt2 = nullptr;                 // [rows] n for the blocks the resumed doubling works on, else 0
    // periodic tier: blocks every other tier gave up on that turn out to be ONE periodic stretch (allocated on first use)
    bool      periodic = true;                   // glcPlanSetSorter 7 switches it off
    uint4    *per_info = nullptr;                // [rows] {period, first break, exit smaller?, slot}
    uint32_t *per_list = nullptr, *per_ok = nullptr;   // [rows] taken blocks by slot; whose rows were written
    uint32_t *per_count = nullptr;               // 16 bytes: [0] blocks taken, [1] bytes of the longest text of representatives, [2] blocks finished, [3] unused
    uint32_t *per_base = nullptr;                // [min(rows, PER_TAKE)][PER_NU + 1] first row of every representative
    uint8_t  *per_text = nullptr;                // [min(rows, PER_TAKE)][PER_NU] the texts of representatives
    uint32_t  resume_min = 2;                    // fewest blocks given up on for depth that are worth the tolerant pass (0: never; sorter modes 5 / 6).  4 until round 6;
                                                 // with chain groups and the tolerant cap at 64: 2 blocks 2.1-2.6 -> 1.6-2.1 ms per call, 3 blocks 2.4-2.9 -> 1.7-2.2; a lone
                                                 // block 1.8-2.3 against 1.6-2.7 (three kinds of four gain, log lines with runs lose: left as it was)
    // A call makes no bucket-sorter attempt (skip_tier1: every block goes to the sample sorter) under sorter 4
    // ... and, adaptively, for SMALL calls (sa_skips_tier1): the reference's callers hand over one block per call, and a text
    // block's call spent 0.13 of its 0.69 ms on the bucket sorter's fourteen launches that find the block flagged.  After
    // TEXT_STREAK calls in a row in which the probe called every block text-like, a call of up to TEXT_SKIP_MAX blocks goes
    // straight to the sample sorter; the first block the probe does not call text-like (it is evaluated in skipped calls too)
    // ends the streak.  A wrong guess costs time (that one call's blocks take the sample sorter), never correctness.
    uint32_t  textlike_streak = 0;
    // second tier (bwt_sample.hip, string sample sort): the blocks the bucket sorter flagged
    uint32_t *ss_list = nullptr;                 // [3 rows] their block numbers; behind them the ones that get a second attempt; then the ones for the tolerant form
    uint64_t *ss_split = nullptr;                // [rows][FS_MAXNB] first suffix of every bucket as a word [code : 36 | index : 20 | 0 : 8]
    uint32_t *ss_flag = nullptr;                 // [rows] this tier's give-up flags
    uint32_t *ss_l0 = nullptr;                   // [rows][FS_MAXNB] common prefix of a bucket's two splitters
    uint2    *ss_long = nullptr;                 // [rows * FS_MAXNB * (SSL_PER_BUCKET + SSL_BIG_PER_BUCKET)] long bins of the sample sorter's first cut
    unsigned long long *ss_long_count = nullptr; // their number: small ones in the low half, big ones in the high half
    uint16_t *ss_cell = nullptr;                 // [rows][4098] first splitter of every cell of the code space
    hipEvent_t ev_flag = nullptr;                // marks a readback: the bucket sorter's (sa_build_begin / sa_build_finish), then every sa_read of the tiers
    // what the glcPlanLastSort* getters report of the plan's last call: assigned whole by sa_build_begin, the tiers only add to it
    SortStats stats;
    // per-call plumbing between sa_build_begin, sa_build_finish and their caller
    uint32_t  parity = 0;                        // set by the caller before sa_build_begin
    bool      skip_tier1 = false;                // this call makes no bucket-sorter attempt (sa_skips_tier1)
    bool      pending = false;                   // sa_build_begin left the tiers to sa_build_finish
    // The sample sorter's SECOND attempt (a block in a few hundred, whose first samples left a bucket past its slot) is a chain
    // of small launches on one block -- 0.54 of a 256-text-block call's 11.3 ms with the chip idle.  A caller that has stages
    // behind the sort (cudpp_api.cpp: MTF + Huffman) sets stage_partial: sa_build_finish calls it ONCE, with a side stream
    // forked off `st` and the mask of the blocks the first attempt finished, before it queues the second attempt, and joins the
    // side stream before it returns; the caller then runs its stages for the blocks of ss_mask[1] only.
    std::function<hipError_t(hipStream_t, const uint32_t *)> stage_partial;
    bool      partial_used = false;              // set by sa_build_finish when it called stage_partial
    uint32_t *ss_mask[2] = {nullptr, nullptr};   // [rows] 1 = flagged block finished by the sample sorter's first attempt / n = still open then
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    KernelProf *prof = nullptr;                  // owned by the plan
};

// (a streak of EIGHT: a wrong guess -- an i.i.d. block behind the streak -- costs that call 0.33 ms, a right one saves 0.05-0.09;
//  with two, a stream of three text blocks and one other per cycle lost 12 %; with eight a mixed stream rarely gets there and a
//  text stream is there after eight calls)
constexpr uint32_t TEXT_STREAK = 8, TEXT_SKIP_MAX = 4;
inline bool sa_skips_tier1(const SaScratch &s, uint32_t nblk)
{
    return s.sorter == 4 || (s.sorter == 0 && nblk <= TEXT_SKIP_MAX && s.textlike_streak >= TEXT_STREAK);
}
hipError_t sa_scratch_alloc(SaScratch &s, uint32_t nmax, uint32_t rows);
// what a plan starts with: GLC_CHAIN_MIN / GLC_CHAIN_ROUNDS (decimal) where set, else 16384 live suffixes, doubling rounds 0, 2, 4
inline void sa_chain_defaults(long *min_live, uint32_t *round_mask)
{
    const char *m = getenv("GLC_CHAIN_MIN"), *r = getenv("GLC_CHAIN_ROUNDS");
    *min_live = m ? atol(m) : 16384;
    *round_mask = r ? (uint32_t)atol(r) : 0x15u;
}
hipError_t sa_general_reserve(SaScratch &s, bool only_sa);
void       sa_scratch_free(SaScratch &s);

// One call of the suffix sorter: `nblk` blocks of n bytes (block b at text + b * text_stride) on stream st.  With bwt_out
// the BWT bytes (L[i] = SA[i]==0 ? T[n-1] : T[SA[i]-1]) and d_index[b] are produced on the way (bwt_compute_final_kernel,
// compress_kernel.cuh:55-74) -- no separate gather; without it the suffix arrays themselves are the result, in s.sa[b * nmax ..].
struct SortCall {
    hipStream_t st; const uint8_t *text; size_t text_stride; uint32_t n, nblk; uint8_t *bwt_out; size_t bwt_stride; int *d_index;
    uint32_t *sa_out(const SaScratch &s) const { return bwt_out ? nullptr : s.sa; }   // where a tier writes suffix-array rows
};

// One encode call of a COMPRESS plan (cudpp_api.cpp), as the entry points and the container hand it over.  n and nblk are the
// caller's numbers: nothing narrows them before they are checked against the plan.  Strided layout: block b's words at out +
// b * out_stride.  Compact layout (block_off given): at out + block_off[b], back to back from *start on, capacity words in all.
struct ContainerHooks;                                         // container_internal.h
struct CompressCall {
    const uint8_t *in; int *bwt_index; uint32_t *hist, *enc_off; size_t off_stride; uint32_t *size, *out; size_t out_stride;
    size_t n, nblk;
    unsigned long long *block_off = nullptr; const unsigned long long *start = nullptr; size_t capacity = 0;
    ContainerHooks *hooks = nullptr;
    bool compact() const { return block_off != nullptr; }
};
// One decode call, the same way (block_off: the compact layout, nblk + 1 entries: block b's words are comp[block_off[b] ..
// block_off[b + 1]))
struct DecodeCall {
    const int *bwt_index; const uint32_t *hist, *enc_off; size_t off_stride; const uint32_t *comp; size_t comp_stride; uint8_t *out;
    size_t n, nblk;
    const unsigned long long *block_off = nullptr;
};

// Host readbacks: nwords device words to the pinned words from `slot` on, then the host waits -- for ev_flag, recorded behind
// the copy, or (the general sorter's rounds, which also run where no bucket sorter created the event) for the whole stream.
// sa_read_queue and sa_read_wait are its two halves, for the one place that queues work between them.
inline hipError_t sa_read_queue(hipStream_t st, SaScratch &s, HostWord slot, const uint32_t *d_src, uint32_t nwords = 1)
{
    return hipMemcpyAsync(s.h_max_cnt + slot, d_src, 4 * (size_t)nwords, hipMemcpyDeviceToHost, st);
}
inline hipError_t sa_read_wait(hipStream_t st, SaScratch &s, bool whole_stream = false)
{
    if (whole_stream) return hipStreamSynchronize(st);
    GLC_TRY(hipEventRecord(s.ev_flag, st));
    return hipEventSynchronize(s.ev_flag);
}
inline hipError_t sa_read(hipStream_t st, SaScratch &s, const uint32_t *&words, HostWord slot, const uint32_t *d_src, uint32_t nwords = 1,
                          bool whole_stream = false)
{
    words = s.h_max_cnt + slot;
    GLC_TRY(sa_read_queue(st, s, slot, d_src, nwords));
    return sa_read_wait(st, s, whole_stream);
}
// the device's count of blocks still given up on (fs_nflag[1]) := left.  The staging word is the copy's alone: nothing else
// writes it, and every later call of this sits behind a host wait on the same stream.
inline hipError_t sa_set_left(hipStream_t st, SaScratch &s, uint32_t left)
{
    s.h_max_cnt[HW_LEFT] = left;
    return hipMemcpyAsync(s.fs_nflag + 1, s.h_max_cnt + HW_LEFT, 4, hipMemcpyHostToDevice, st);
}

// the tiers in sequence (bwt_tiers.cpp).  Synchronises the stream once per doubling round of the general sorter.
hipError_t sa_build(const SortCall &c, SaScratch &s);
// two-phase form of sa_build (see bwt_tiers.cpp): stages that follow the sort can be queued between the two calls
hipError_t sa_build_begin(const SortCall &c, SaScratch &s);
hipError_t sa_build_finish(const SortCall &c, SaScratch &s, uint32_t *nflagged);

// the general sorter (bwt_sa.hip); cnt0 (optional) = per-block element counts: n for the nsorted blocks to sort, 0 for the others
// resume_depth != 0: s.keyA already holds, for the blocks of cnt0, the words [group : 44 | suffix : 20] of an order that is
// exact for the first resume_depth symbols (grp_keys): no sort from the text, prefix doubling from that depth on
hipError_t sa_build_general(const SortCall &c, SaScratch &s, const uint32_t *cnt0, uint32_t nsorted, uint32_t resume_depth = 0);
// (bwt_sa.hip) the rows of s.sa that the sample sorter's tolerant form left for the ndeep blocks listed for it -> those words
// in s.keyA, s.ss_cnt2[b] = n for the blocks it did not give up on (0 for every other block of the plan); enqueues only
hipError_t grp_keys(const SortCall &c, SaScratch &s, uint32_t ndeep);

// the fast path alone (bwt_bucket.hip): enqueues only; flagged blocks are reported in s.fs_lcnt / s.fs_nflag
hipError_t fs_build(const SortCall &c, SaScratch &s);
uint32_t   fs_bucket_log2(uint32_t n);
// k_fs_scan (bwt_bucket.hip) for the nlisted blocks of `list`: fbase = exclusive scan of a block's bucket fills, a bucket past its slot flags the block
hipError_t fs_scan(hipStream_t st, uint32_t nlisted, const uint32_t *fill, uint32_t *fbase, uint32_t *flag, const uint32_t *list);
// second tier for the nflag blocks listed in s.ss_list (c.nblk is not looked at): enqueues only; blocks it gives up on keep
// n in s.fs_lcnt (the others get 0) and are counted in s.fs_nflag[1]
hipError_t ss_build(const SortCall &c, SaScratch &s, uint32_t nflag, uint32_t attempt = 0);
// blocks of the first attempt whose only trouble was a bucket past its slot -> listed behind ss_list, count in s.fs_nflag[2]
// (count_only: nothing is listed or cleared -- how many there are decides whether the attempt is worth making)
hipError_t ss_retry_prepare(hipStream_t st, uint32_t nflag, SaScratch &s, uint32_t to = 1, bool count_only = false);
// s.ss_mask[0][b] = 1 for the flagged blocks (redo[b] != 0) the first attempt finished (s.fs_lcnt[b] == 0), s.ss_mask[1] = a
// snapshot of s.fs_lcnt: the blocks still open at that moment
hipError_t ss_split_masks(hipStream_t st, uint32_t nblk, SaScratch &s);

// periodic tier (bwt_periodic.hip); enqueue only.  per_detect lists the taken blocks of s.ss_list[0 .. nlisted) whose ss_flag is
// raised (count -> s.per_count[0], the longest text of representatives -> s.per_count[1]); per_text writes their texts of representatives (nu bytes each, stride PER_NU); per_expand
// turns the suffix arrays of those texts (s.sa, rows 0 .. nper) into the blocks' BWT rows and indices, clears ss_flag /
// fs_lcnt of every block it finishes and counts them in s.per_count[2]
hipError_t per_reserve(SaScratch &s);
hipError_t per_detect(const SortCall &c, SaScratch &s, uint32_t nlisted);
// before the sample sorter's first attempt: listed blocks whose beginning is periodic for 3/8 of the block or more get ss_flag = 3
hipError_t per_probe(const SortCall &c, SaScratch &s, uint32_t nlisted);
hipError_t per_text(const SortCall &c, SaScratch &s, uint32_t nper, uint32_t nu);
hipError_t per_expand(const SortCall &c, SaScratch &s, uint32_t nper, uint32_t nu);

// copy SA to the cudppSuffixArray layout (out[0]=n, out[1..n]=SA)
hipError_t sa_export(hipStream_t st, const uint32_t *sa, uint32_t n, uint32_t *out);

// ---------------------------------------------------------------------------
// MTF
// ---------------------------------------------------------------------------
struct MtfScratch {
    KernelProf *prof = nullptr;
    uint32_t nmax = 0, rows = 0, max_chunks = 0;
    uint8_t  *lists = nullptr;       // [rows][max_chunks][256] chunk-local recency lists, then start lists
    uint16_t *lens = nullptr;        // [rows][max_chunks]
    size_t    bytes = 0;
};
hipError_t mtf_scratch_alloc(MtfScratch &s, uint32_t nmax, uint32_t rows);
void       mtf_scratch_free(MtfScratch &s);

// out = MTF(in) per block; if sub_hist != nullptr also writes the histogram of
// each 4096-symbol chunk of the output: sub_hist[b][chunk][SUBHIST_DWORDS].
hipError_t mtf_forward(hipStream_t st, const uint8_t *in, size_t in_stride, uint32_t n, uint32_t nblk,
                       uint8_t *out, size_t out_stride, MtfScratch &s, uint32_t *sub_hist, const uint32_t *only = nullptr,
                       bool skewed = false);
// (`only`, here and in the Huffman stages: if given, blocks whose entry is 0 are skipped -- the second pass over the
//  blocks a later sorter tier rewrote; `skewed`: those blocks are text-like, rank 0 is most of their output -- the encoder's
//  histogram counts it with a ballot per row instead of sixteen adds to one counter)

// ---------------------------------------------------------------------------
// Huffman
// ---------------------------------------------------------------------------
struct HuffScratch {
    KernelProf *prof = nullptr;
    uint32_t nmax = 0, rows = 0, max_sub = 0;
    uint32_t *sub_hist = nullptr;    // [rows][max_sub][SUBHIST_DWORDS]
    uint32_t *codes = nullptr;       // [rows][257]
    uint32_t *lens = nullptr;        // [rows][257]  (one word each for aligned LDS staging)
    size_t    bytes = 0;
};
hipError_t huff_scratch_alloc(HuffScratch &s, uint32_t nmax, uint32_t rows);
void       huff_scratch_free(HuffScratch &s);

// sub-block histograms of caller-supplied symbols (stand-alone Huffman entry point)
hipError_t huff_histogram(hipStream_t st, const uint8_t *sym, size_t stride, uint32_t n, uint32_t nblk, HuffScratch &s);
// tree + codes + offsets (writes d_hist[b][256], d_offsets[b*offset_stride..], d_size[b]).  redo_flag (optional):
// blocks with a non-zero entry are going to be encoded again (speculative pass over blocks the bucket sorter has
// flagged): their status bits are not raised.
hipError_t huff_build(hipStream_t st, uint32_t n, uint32_t nblk, HuffScratch &s, uint32_t *d_hist,
                      uint32_t *d_offsets, size_t offset_stride, uint32_t *d_size,
                      size_t capacity_words, uint32_t *d_status, const uint32_t *redo_flag = nullptr,
                      const uint32_t *only = nullptr);
// pack (reads mtf bytes, writes the stream)
//   d_block_off (compact layout): block b is written at d_compressed + d_block_off[b]; capacity_words bounds the array
hipError_t huff_pack(hipStream_t st, const uint8_t *mtf, size_t mtf_stride, uint32_t n, uint32_t nblk,
                     HuffScratch &s, const uint32_t *d_offsets, size_t offset_stride,
                     uint32_t *d_compressed, size_t comp_stride_words, const uint32_t *only = nullptr,
                     const unsigned long long *d_block_off = nullptr, size_t capacity_words = 0);
// d_off[b] = *d_start (0 if null) + sizes of the blocks before b; d_off[nblk] = the end; past capacity_words -> ST_CAPACITY
hipError_t huff_block_offsets(hipStream_t st, const uint32_t *d_sizes, uint32_t nblk, unsigned long long *d_off,
                              const unsigned long long *d_start, size_t capacity_words, uint32_t *d_status);

hipError_t compact_streams(hipStream_t st, const uint32_t *d_comp, size_t stride, const uint32_t *d_sizes,
                           uint32_t nblk, uint32_t *d_out, unsigned long long *d_off);

hipError_t expand_streams(hipStream_t st, const uint32_t *d_in, const unsigned long long *d_off, uint32_t nblk,
                          uint32_t *d_comp, size_t stride, uint32_t *d_sizes, uint32_t *d_status);

// ---------------------------------------------------------------------------
// batched order-0 Huffman (hd_batch.hip; the public form is glcHdSegments* in include/glc_hd.h): one table per segment,
// thousands of segments per launch.  Segment i is [base + off[i], + min(len[i], max_len)), max_len <= HDB_MAX_LEN, any
// byte alignment; off / len are device arrays.  Everything only enqueues on `st`.  skip (optional): segments whose entry
// is non-zero are left alone.  prof (optional): the live per-kernel profile the launches are bracketed for.
// ---------------------------------------------------------------------------
constexpr uint32_t HDB_MAX_LEN = 1u << 20;
struct HdbSegs { const uint8_t *base; const unsigned long long *off, *len; uint32_t count, max_len; };
// segment i's bytes: base may be null with absolute addresses in off, so the sum is taken on integers
__host__ __device__ inline const uint8_t *hdb_seg(const HdbSegs &g, uint32_t i) { return reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(g.base) + g.off[i]); }
struct HdbOut { uint8_t *base; const unsigned long long *off, *len; uint32_t count, max_len; };   // the decoder's side: written
constexpr size_t HDB_MAX_COUNT = (size_t)1 << 22;            // segments per call: one workgroup of up to 512 lanes each, grid.x * 512 < 2^32
size_t hdb_encode_work_bytes(size_t count);
size_t hdb_decode_work_bytes(size_t count, size_t max_len);          // (without the tables: 4096 bytes of LUT per segment)
// hist[i][256] (u32) = the segment's byte counts (make_hist; else hist is the input and g.base / g.off / g.len are not
// read); from it the table glcHdBuildTable gives -- lens[i][256], codes[i][256], lut[i][2048] (the decode kernels' u16
// form), each optional -- and nunits[i] = ceil(sum hist * lens / 32) + 1, the units of the segment's stream, pad included
hipError_t hdb_tables(hipStream_t st, const HdbSegs &g, bool make_hist, uint32_t *hist, uint8_t *lens, uint16_t *codes,
                      uint16_t *lut, unsigned long long *nunits, const uint32_t *skip, KernelProf *prof);
// segment i's stream, word for word glcHdEncodeHost's, at units_base + unit_off[i]; a segment whose nunits[i] units would
// end past cap_units (counted from units_base), or whose bytes no longer give nunits[i], is not written at all
hipError_t hdb_encode(hipStream_t st, const HdbSegs &g, const uint8_t *lens, const uint16_t *codes,
                      const unsigned long long *nunits, uint32_t *units_base, const unsigned long long *unit_off,
                      unsigned long long cap_units, const uint32_t *skip, void *work, KernelProf *prof);
// g.len[i] symbols of the stream of nunits[i] units at units_base + unit_off[i] to g.base + g.off[i] (g.base may be null with addresses in g.off),
// with the tables in lut.  Reads stay inside the stream's units, writes inside the segment, whatever the units hold.
hipError_t hdb_decode(hipStream_t st, const uint32_t *units_base, const unsigned long long *unit_off,
                      const unsigned long long *nunits, const uint16_t *lut, const HdbOut &g, const uint32_t *skip,
                      void *work, KernelProf *prof);

// ---------------------------------------------------------------------------
// decoder (round-trip parity only; the reference has no GPU decoder)
// ---------------------------------------------------------------------------
struct DecodeScratch {
    KernelProf *prof = nullptr;
    uint32_t nmax = 0, rows = 0, max_tiles = 0, max_split = 0, max_chunks = 0;
    uint8_t  *mtf = nullptr, *bwt = nullptr;     // [rows][nmax]
    uint8_t  *bwt2 = nullptr;                    // second BWT buffer for stage pipelining
    uint8_t  *ilists = nullptr;                  // [rows][max_chunks][256] iMTF chunk permutations / start lists
    uint32_t *lf = nullptr;                      // [rows][nmax+1]  (symbol << 21) | LF(row)
    uint32_t *lut = nullptr;                     // [rows][4096] 12-bit Huffman decode table
    uint32_t *nodes = nullptr;                   // [rows][513]  tree for codes longer than 12 bits
    uint32_t *tile_hist = nullptr;               // [rows][max_tiles][512]
    uint32_t *digit_base = nullptr;              // [rows][512]
    uint32_t *seg = nullptr;                     // [rows][max_seg] len | next << 9
    int      *seg_pos = nullptr;                 // [rows][max_seg] text position of the segment's first symbol
    uint32_t *seg_count = nullptr;               // [rows] segments in use (static splitters + dynamic)
    uint8_t  *slots = nullptr;                   // [rows][max_seg][256] symbols emitted by each segment
    uint32_t  max_seg = 0;
    size_t    bytes = 0;
    int       huff_decoder = 0;                  // glcPlanSetHuffDecoder: 0 by the call's size, 1 k_dec_huff, 2 k_dec_huff_lanes
};
hipError_t tile_hist_scan9(hipStream_t st, uint32_t *tile_hist, uint32_t count, uint32_t *digit_base,
                           uint32_t max_tiles, uint32_t nblk, uint32_t tile_elems);
hipError_t decode_scratch_alloc(DecodeScratch &s, uint32_t nmax, uint32_t rows);
void       decode_scratch_free(DecodeScratch &s);
// stage A: the call's streams -> BWT bytes in `bwt`; stage B: `bwt` -> c.out; decode_blocks: both, through s.bwt
hipError_t decode_stage_a(hipStream_t st, const DecodeCall &c, DecodeScratch &s, uint8_t *bwt, uint32_t *d_status);
hipError_t decode_stage_b(hipStream_t st, const DecodeCall &c, const uint8_t *bwt, DecodeScratch &s, uint32_t *d_status);
hipError_t decode_blocks(hipStream_t st, const DecodeCall &c, DecodeScratch &s, uint32_t *d_status);
// the two halves of stage A on their own (glcHuffmanDecodeBatch, glcMtfInverseBatch): the call's streams -> c.nblk rows of
// symbols at `sym`; nblk rows of MTF bytes at `mtf` -> BWT bytes at `bwt`.  Rows at the strides given.
hipError_t decode_huff_rows(hipStream_t st, const DecodeCall &c, DecodeScratch &s, uint8_t *sym, size_t sym_stride,
                            uint32_t *d_status);
hipError_t decode_imtf_rows(hipStream_t st, uint32_t n, uint32_t nblk, DecodeScratch &s, const uint8_t *mtf, size_t in_stride,
                            uint8_t *bwt, size_t out_stride);
// stage A without its Huffman step, then stage B: c.nblk rows of MTF bytes at `mtf` (stride s.nmax; the container's zero-run
// records are joined into s.mtf) -> c.out.  Of c only bwt_index, out, n and nblk are read.
hipError_t decode_mtf_blocks(hipStream_t st, const DecodeCall &c, const uint8_t *mtf, DecodeScratch &s, uint32_t *d_status);

} // namespace glc
