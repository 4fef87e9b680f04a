// cudpp_api.cpp -- the C ABI of include/cudpp.h: library/plan handles, argument
// validation and the per-call orchestration of the HIP stages.
//
// Mirrors the reference's public layer (cudpp-inpar/src/cudpp/cudpp.cpp:764-919,
// 1000-1034; cudpp_plan.cpp:29-46,81-292,712-799; cudpp_manager.cpp:40-63):
// same entry points, same handle representation (a pointer cast to size_t,
// cudpp_plan.h:51-54), same validation order and result codes.  Differences are
// deliberate and listed in DESIGN.md: plans are reusable (the reference leaks /
// drifts, sa_app.cu:201-202,340-351), nothing is allocated per call
// (compress_app.cu:257,263; sa_app.cu:73-100), HIP failures are returned as
// CUDPP_ERROR_UNKNOWN instead of exit() (cuda_util.h:13-21).
#include "../../include/cudpp.h"
#include "container_internal.h"
#include "glc_internal.h"

#include <new>
#include <stdlib.h>
#include <string.h>

using namespace glc;

// the fill seam of the scratch allocation helpers (glc_internal.h): the word repeated over the whole block, the last 1 to 3
// bytes from the word's low bytes, complete on return (a stream-ordered block is filled on its stream, which is then waited for)
ScratchFill glc::g_scratch_fill;
hipError_t glc::scratch_fill(void *p, size_t bytes, bool pinned, hipStream_t st)
{
    const uint32_t w = g_scratch_fill.word;
    const size_t words = bytes / 4, tail = bytes & 3;
    if (pinned) {
        for (size_t i = 0; i < words; i++) memcpy(static_cast<uint8_t *>(p) + 4 * i, &w, 4);
        memcpy(static_cast<uint8_t *>(p) + 4 * words, &w, tail);
    } else {
        if (words) GLC_TRY(hipMemsetD32Async(static_cast<hipDeviceptr_t>(p), (int)w, words, st));
        if (tail) GLC_TRY(hipMemcpyAsync(static_cast<uint8_t *>(p) + 4 * words, &w, tail, hipMemcpyHostToDevice, st));
        GLC_TRY(hipStreamSynchronize(st));
    }
    g_scratch_fill.blocks++;
    g_scratch_fill.bytes += bytes;
    return hipSuccess;
}

namespace {

struct Manager {
    int device = 0;
};

struct PlanBase {
    CUDPPConfiguration config{};
    uint32_t n = 0, rows = 1;
    hipStream_t stream = nullptr;
    uint32_t *d_status = nullptr;
    uint32_t *h_status = nullptr;
    bool timing = false;
    KernelProf prof;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    float last_ms[4] = {0, 0, 0, 0};

    hipError_t init_common()
    {
        hipError_t e = glc_dev_alloc((void **)&d_status, 4);
        if (e != hipSuccess) return e;
        e = hipMemset(d_status, 0, 4);
        if (e != hipSuccess) return e;
        return glc_host_alloc((void **)&h_status, 4);
    }
    virtual ~PlanBase()
    {
        if (d_status) (void)hipFree(d_status);
        if (h_status) (void)hipHostFree(h_status);
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    }
    // what the entry points ask of a plan whatever its algorithm
    virtual SaScratch *sorter() { return nullptr; }            // the suffix sorter's scratch (MTF plans have none)
    virtual void join_side() {}                                // the plan's stream waits for everything on its side stream (COMPRESS)
    virtual void wire_prof() = 0;                              // point the stage scratches at the plan's live profile
    virtual hipEvent_t side_span_start() { return nullptr; }   // stages on two streams: the event their second span starts at
};

struct SortPlan : PlanBase {                     // CUDPPSaPlan and CUDPPBwtPlan (cudpp_plan.h:289-305, 343-356)
    SaScratch sa;
    ~SortPlan() override { sa_scratch_free(sa); }
    SaScratch *sorter() override { return &sa; }
    void wire_prof() override { sa.prof = &prof; }
};
struct MtfPlan : PlanBase {                      // CUDPPMtfPlan (cudpp_plan.h:358-369)
    MtfScratch mtf;
    ~MtfPlan() override { mtf_scratch_free(mtf); }
    void wire_prof() override { mtf.prof = &prof; }
};

// A double-buffered half changing hands between the calls of one direction: call i works on half i & 1, and may start on
// it once call i - 2 has released it.  (The count runs on when the mode changes; only the releases are forgotten.)
struct HandOver {
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool valid[2] = {false, false};
    uint32_t calls = 0;
    uint32_t next() const { return calls & 1u; }               // the half the next call takes
    uint32_t take() { return calls++ & 1u; }
    void wait_free(uint32_t k, hipStream_t s) const { if (valid[k]) (void)hipStreamWaitEvent(s, ev[k], 0); }
    void release(uint32_t k, hipStream_t s) { (void)hipEventRecord(ev[k], s); valid[k] = true; }
    void reset() { valid[0] = valid[1] = false; }
};

// Device memory a plan keeps for its container path: grown on demand, never shrunk, freed with the plan
struct GrowBuf {
    void *mem = nullptr;
    size_t bytes = 0;
    hipError_t grow(PlanBase &p, size_t want, uint8_t **out)
    {
        if (want > bytes) {
            if (mem) {                                         // (growing: whatever still uses the old one finishes first)
                p.join_side();
                (void)hipStreamSynchronize(p.stream);
                (void)hipFree(mem);
                mem = nullptr; bytes = 0;
            }
            const hipError_t e = glc_dev_alloc(&mem, want);
            if (e != hipSuccess) { mem = nullptr; return e; }
            bytes = want;
        }
        *out = static_cast<uint8_t *>(mem);
        return hipSuccess;
    }
    ~GrowBuf() { if (mem) (void)hipFree(mem); }
};
// ... and the pinned host memory it keeps for the same path (readback words, the host-pointer and file forms' staging)
struct GrowPinned {
    void *mem = nullptr;
    size_t bytes = 0;
    hipError_t grow(PlanBase &p, size_t want, void **out)
    {
        if (want > bytes) {
            if (mem) {                                         // (growing: a copy into or out of the old one finishes first)
                p.join_side();
                (void)hipStreamSynchronize(p.stream);
                (void)hipHostFree(mem);
                mem = nullptr; bytes = 0;
            }
            const hipError_t e = glc_host_alloc(&mem, want);
            if (e != hipSuccess) { mem = nullptr; return e; }
            bytes = want;
        }
        *out = mem;
        return hipSuccess;
    }
    ~GrowPinned() { if (mem) (void)hipHostFree(mem); }
};

struct CompressPlan : PlanBase {                 // CUDPPCompressPlan (cudpp_plan.h:307-341)
    SaScratch sa;
    MtfScratch mtf;
    HuffScratch huff;
    DecodeScratch dec;
    uint8_t *d_bwt = nullptr, *d_mtf = nullptr;  // [rows][n]
    // stage pipelining (glcPlanSetPipelining): the suffix sort of batch i+1 runs on `side` while the
    // MTF + Huffman stages of batch i run on the plan's stream; d_bwt is double-buffered between them
    bool pipelined = false;
    uint8_t *d_bwt2 = nullptr;
    hipStream_t side = nullptr;
    hipEvent_t ev_in = nullptr, ev_sorted[2] = {nullptr, nullptr}, ev_dec_a[2] = {nullptr, nullptr}, ev_s2 = nullptr;
    HandOver enc_half, dec_half;                 // d_bwt / d_bwt2 between compress calls, dec.bwt / dec.bwt2 between decompress calls
    // every event of the side stream: pipeline_init creates them in this order, the destructor destroys them (ev_s2, the
    // last, is the one that is read for a time)
    hipEvent_t *const side_events[10] = {&ev_in, &ev_sorted[0], &ev_sorted[1], &enc_half.ev[0], &enc_half.ev[1],
                                         &ev_dec_a[0], &ev_dec_a[1], &dec_half.ev[0], &dec_half.ev[1], &ev_s2};
    bool side_busy = false;                      // side-stream work issued since the last join
    // container settings (glcPlanSetContainerShuffle / Delta / Codec / Sparse / Runs / Ans) and the filter's frame staging both directions share
    CtSettings ct;
    CtReports ct_reports;                        // what the glcContainerLast* entries report
    GrowBuf ct_stage[2];
    GrowBuf ct_codec[CT_DEV_SLOTS];              // the order-0 container codec's scratch, its sparse and rANS modes' and the runs mode's included: [0] the encoder's, [1] the decoder's; [2] the frame index walk's entries; from [3] on the slots of container_internal.h (CtDevSlot): what a container call used to allocate and free itself -- hipFree waits for the whole device, so a call that frees serialises against every stream of the caller's
    GrowPinned ct_pinned[CT_PIN_SLOTS];          // CtPinSlot: the readback words and the host forms' staging
    SaScratch *sorter() override { return &sa; }
    void wire_prof() override { sa.prof = &prof; mtf.prof = &prof; huff.prof = &prof; dec.prof = &prof; }
    hipEvent_t side_span_start() override { return pipelined ? ev_s2 : nullptr; }
    void join_side() override
    {
        if (!side || !side_busy) return;
        (void)hipEventRecord(ev_in, side);
        (void)hipStreamWaitEvent(stream, ev_in, 0);
        side_busy = false;
    }
    hipError_t pipeline_init()
    {
        if (side) return hipSuccess;
        hipError_t e = glc_dev_alloc((void **)&d_bwt2, (size_t)n * rows);
        if (e == hipSuccess) {
            // lowest priority: the second halves fill the slots the first halves leave free.  Measured on the
            // 4 GiB bench: decode 26.6 (default priority) / 27.3 (lowest) / 25.9 GB/s (highest); encode unchanged.
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            e = hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least);
        }
        for (hipEvent_t *pe : side_events)
            if (e == hipSuccess) e = pe == &ev_s2 ? hipEventCreate(pe) : hipEventCreateWithFlags(pe, hipEventDisableTiming);
        return e;
    }
    ~CompressPlan() override
    {
        if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
        for (hipEvent_t *pe : side_events) if (*pe) (void)hipEventDestroy(*pe);
        sa_scratch_free(sa); mtf_scratch_free(mtf); huff_scratch_free(huff); decode_scratch_free(dec);
        if (d_bwt) (void)hipFree(d_bwt);
        if (d_bwt2) (void)hipFree(d_bwt2);
        if (d_mtf) (void)hipFree(d_mtf);
    }
};

template <class T> T *plan_from(CUDPPHandle h) { return reinterpret_cast<T *>(h); }

CUDPPResult validate_options(const CUDPPConfiguration &c)
{   // cudpp_plan.cpp:29-46
    if ((c.options & CUDPP_OPTION_BACKWARD) && (c.options & CUDPP_OPTION_FORWARD))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if ((c.options & CUDPP_OPTION_EXCLUSIVE) && (c.options & CUDPP_OPTION_INCLUSIVE))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return CUDPP_SUCCESS;
}

struct StageTimer {
    PlanBase *p;
    explicit StageTimer(PlanBase *pl) : p(pl)
    {
        if (p->timing && !p->ev[0])
            for (auto &e : p->ev) (void)hipEventCreate(&e);
    }
    void mark(int i) { if (p->timing) (void)hipEventRecord(p->ev[i], p->stream); }
    void done() { if (p->timing) p->ev_valid = true; }
};

// glcPlanLastTiming's four spans, read from the stage events once the plan's streams are idle.  Stages that ran on two
// streams report their own spans: the second starts at the side stream's event, and the total is the sum of the three.
void read_spans(PlanBase *p)
{
    const hipEvent_t s2 = p->side_span_start();
    (void)hipEventElapsedTime(&p->last_ms[0], p->ev[0], p->ev[1]);
    (void)hipEventElapsedTime(&p->last_ms[1], s2 ? s2 : p->ev[1], p->ev[2]);
    (void)hipEventElapsedTime(&p->last_ms[2], p->ev[2], p->ev[3]);
    if (s2) p->last_ms[3] = p->last_ms[0] + p->last_ms[1] + p->last_ms[2];
    else (void)hipEventElapsedTime(&p->last_ms[3], p->ev[0], p->ev[3]);
}

// Entry check of the plan utilities: the handle and, where the entry has one, its output pointer (a null output is
// reported as an invalid handle, as it always was).  Null: the entry answers CUDPP_ERROR_INVALID_HANDLE.
PlanBase *plan_of(CUDPPHandle planHandle, bool has_out = true)
{
    return planHandle == 0 || planHandle == CUDPP_INVALID_HANDLE || !has_out ? nullptr : plan_from<PlanBase>(planHandle);
}

// Entry check of the batch entries, in the order the codes are documented in: handle, algorithm, datatype (ANY_DATATYPE: the
// entry does not look at it -- glcHuffmanEncodeBatch and the two decompress entries, which take their symbols as bytes
// whatever the plan was made for), then the call's sizes against the plan's.  Null: the entry answers `why`.
enum DatatypeCheck { ANY_DATATYPE, UCHAR_ONLY };
template <class T>
T *batch_plan(CUDPPHandle planHandle, CUDPPAlgorithm algorithm, DatatypeCheck dt, size_t numElements, size_t numBlocks, CUDPPResult &why)
{
    PlanBase *p = plan_of(planHandle);
    why = !p ? CUDPP_ERROR_INVALID_HANDLE
        : p->config.algorithm != algorithm ? CUDPP_ERROR_INVALID_PLAN
        : (dt == UCHAR_ONLY && p->config.datatype != CUDPP_UCHAR) || numElements == 0 || numElements > p->n || numBlocks == 0 ||
          numBlocks > p->rows ? CUDPP_ERROR_ILLEGAL_CONFIGURATION : CUDPP_SUCCESS;
    return why == CUDPP_SUCCESS ? static_cast<T *>(p) : nullptr;
}

// the stats getters and glcPlanSetChains: the utilities' check, then the plan type, then f on the plan's sorter scratch
template <class F> CUDPPResult with_sorter(CUDPPHandle planHandle, bool has_out, F f)
{
    PlanBase *p = plan_of(planHandle, has_out);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    SaScratch *s = p->sorter();
    if (!s) return CUDPP_ERROR_INVALID_PLAN;
    f(*s);
    return CUDPP_SUCCESS;
}

} // namespace

extern "C" {

CUDPPResult cudppCreate(CUDPPHandle *theCudpp)
{
    if (!theCudpp) return CUDPP_ERROR_INVALID_HANDLE;
    Manager *m = new (std::nothrow) Manager();
    if (!m) return CUDPP_ERROR_UNKNOWN;
    if (hipGetDevice(&m->device) != hipSuccess) { delete m; *theCudpp = 0; return CUDPP_ERROR_UNKNOWN; }
    *theCudpp = reinterpret_cast<CUDPPHandle>(m);
    return CUDPP_SUCCESS;
}

CUDPPResult cudppDestroy(CUDPPHandle theCudpp)
{
    if (theCudpp == 0 || theCudpp == CUDPP_INVALID_HANDLE) return CUDPP_ERROR_INVALID_HANDLE;
    delete reinterpret_cast<Manager *>(theCudpp);
    return CUDPP_SUCCESS;
}

CUDPPResult cudppPlan(const CUDPPHandle cudppHandle, CUDPPHandle *planHandle, CUDPPConfiguration config,
                      size_t n, size_t rows, size_t /*rowPitch*/)
{
    if (!planHandle) return CUDPP_ERROR_INVALID_HANDLE;
    *planHandle = CUDPP_INVALID_HANDLE;
    if (cudppHandle == 0 || cudppHandle == CUDPP_INVALID_HANDLE) return CUDPP_ERROR_INVALID_HANDLE;
    CUDPPResult r = validate_options(config);
    if (r != CUDPP_SUCCESS) return r;
    if (rows == 0) rows = 1;
    if (n == 0 || rows > 65535) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;

    PlanBase *plan = nullptr;
    hipError_t e = hipSuccess;
    switch (config.algorithm) {
    case CUDPP_COMPRESS: {
        if (n > MAX_BLOCK_ELEMS) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
        CompressPlan *p = new (std::nothrow) CompressPlan();
        if (!p) return CUDPP_ERROR_UNKNOWN;
        plan = p;
        e = sa_scratch_alloc(p->sa, (uint32_t)n, (uint32_t)rows);
        if (e == hipSuccess) e = mtf_scratch_alloc(p->mtf, (uint32_t)n, (uint32_t)rows);
        if (e == hipSuccess) e = huff_scratch_alloc(p->huff, (uint32_t)n, (uint32_t)rows);
        if (e == hipSuccess) e = glc_dev_alloc((void **)&p->d_bwt, n * rows);
        if (e == hipSuccess) e = glc_dev_alloc((void **)&p->d_mtf, n * rows);
        break;
    }
    case CUDPP_BWT: case CUDPP_SA: {
        if (n > MAX_BLOCK_ELEMS) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
        SortPlan *p = new (std::nothrow) SortPlan();
        if (!p) return CUDPP_ERROR_UNKNOWN;
        plan = p;
        e = sa_scratch_alloc(p->sa, (uint32_t)n, (uint32_t)rows);
        break;
    }
    case CUDPP_MTF: {
        if (n > (1u << 30)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
        MtfPlan *p = new (std::nothrow) MtfPlan();
        if (!p) return CUDPP_ERROR_UNKNOWN;
        plan = p;
        e = mtf_scratch_alloc(p->mtf, (uint32_t)n, (uint32_t)rows);
        break;
    }
    default:
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;   // not on the compression path
    }
    if (e == hipSuccess) e = plan->init_common();
    if (e != hipSuccess) { delete plan; return hip_result(e); }
    plan->config = config;
    plan->n = (uint32_t)n;
    plan->rows = (uint32_t)rows;
    *planHandle = reinterpret_cast<CUDPPHandle>(plan);
    return CUDPP_SUCCESS;
}

CUDPPResult cudppDestroyPlan(CUDPPHandle planHandle)
{
    if (planHandle == CUDPP_INVALID_HANDLE || planHandle == 0) return CUDPP_ERROR_INVALID_HANDLE;
    PlanBase *p = plan_from<PlanBase>(planHandle);
    switch (p->config.algorithm) {
    case CUDPP_COMPRESS: case CUDPP_BWT: case CUDPP_MTF: case CUDPP_SA:
        (void)hipStreamSynchronize(p->stream);
        delete p;
        return CUDPP_SUCCESS;
    default:
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    }
}

// --------------------------------------------------------------------------
// batched entry points
// --------------------------------------------------------------------------
// One body for the two output layouts of a CompressCall.  Strided (c.block_off == nullptr): block b's words at c.out +
// b * c.out_stride, the reference's layout per block.  Compact: block b's words at c.out +
// c.block_off[b], the blocks back to back from *c.start on -- the sizes are known before anything is packed
// (k_huff_build), so the packer writes every block where it ends up and no copy pass follows.  In that mode the packer
// runs once, after the host knows that no block's size can still change (the sorter's tiers are through).
static CUDPPResult compress_batch(CUDPPHandle planHandle, const CompressCall &c)
{
    // c.hooks (the container path, compact layout only): a status word of its own -- a block whose sub-block overflows becomes a raw
    // record there instead of failing the call --, its kernels before the payload offsets and behind the packer, and the
    // packer's block mask
    const ContainerHooks *const hk = c.hooks;
    const bool compact = c.compact();
    CUDPPResult why;
    CompressPlan *p = batch_plan<CompressPlan>(planHandle, CUDPP_COMPRESS, UCHAR_ONLY, c.n, c.nblk, why);
    if (!p) return why;
    const uint32_t n = (uint32_t)c.n, nb = (uint32_t)c.nblk;
    const uint32_t nsub = (n + HUFF_BLOCK - 1) / HUFF_BLOCK;
    if (c.off_stride < nsub) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    hipStream_t st = p->stream;
    StageTimer tm(p);
    hipError_t e = hipSuccess;
    uint32_t *const status = hk ? hk->status : p->d_status;
    uint8_t *bwt = p->d_bwt;
    const uint32_t k = p->enc_half.take();
    hipStream_t s2 = st;                                       // stream of the MTF + Huffman stages
    if (p->pipelined) {
        // The sort stays on the plan's stream (inputs keep their stream order).  MTF + Huffman move to the side
        // stream, where they overlap the sort of the NEXT call; the outputs they write are complete after
        // glcPlanSynchronize / glcCompactStreams / a device synchronize (include/cudpp.h).
        e = p->pipeline_init();
        if (e != hipSuccess) return hip_result(e);
        bwt = k ? p->d_bwt2 : p->d_bwt;
        p->enc_half.wait_free(k, st);                          // this BWT half is free again
        s2 = p->side;
    }
    // The stages after the sort are queued BEFORE the host waits for the sorter's one readback (how many blocks the
    // bucket sorter handed to the general sorter): the GPU has MTF + Huffman to do while the host wakes up and queues
    // the next call.  In the rare batch with flagged blocks they run again on the corrected BWT.
    tm.mark(0);
    p->sa.parity = k;
    const SortCall sort{st, c.in, n, n, nb, bwt, p->n, c.bwt_index};
    e = sa_build_begin(sort, p->sa);
    tm.mark(1);
    // MTF + Huffman of the blocks of `only` (all if null) on `stream`, behind whatever error `err` already holds
    auto run_stages = [&](hipStream_t stream, hipError_t err, const uint32_t *redo_flag, const uint32_t *only, bool skewed) {
        if (err == hipSuccess) err = mtf_forward(stream, bwt, p->n, n, nb, p->d_mtf, p->n, p->mtf, p->huff.sub_hist, only, skewed);
        if (p->timing) (void)hipEventRecord(p->ev[2], stream);
        // (compact layout: a block has no slot of its own to overflow -- the array's capacity is checked with the offsets)
        if (err == hipSuccess) err = huff_build(stream, n, nb, p->huff, c.hist, c.enc_off, c.off_stride, c.size,
                                                compact ? (size_t)(HUFF_MAX_WORDS + 1) * nsub : c.out_stride, status,
                                                redo_flag, only);
        if (err == hipSuccess && !compact) err = huff_pack(stream, p->d_mtf, p->n, n, nb, p->huff, c.enc_off, c.off_stride,
                                                           c.out, c.out_stride, only);
        return err;
    };
    auto after_sort = [&](const uint32_t *redo_flag, const uint32_t *only, bool skewed) {
        if (p->pipelined) {
            (void)hipEventRecord(p->ev_sorted[k], st);
            (void)hipStreamWaitEvent(s2, p->ev_sorted[k], 0);
            if (p->timing) (void)hipEventRecord(p->ev_s2, s2);
        }
        e = run_stages(s2, e, redo_flag, only, skewed);
        if (p->timing) (void)hipEventRecord(p->ev[3], s2);
    };
    // Blocks the bucket sorter has given up on (flagged up front as text-like, or after its attempt) are skipped by this
    // speculative pass (`only` = the sorter's keep mask of this call) and encoded below, once their sort is final.
    const bool tiers = p->sa.sorter == 0 || p->sa.sorter == 3 || p->sa.sorter == 4;
    const bool speculate = !tiers || !sa_skips_tier1(p->sa, nb);   // (no attempt of the bucket sorter: nothing to speculate on)
    if (speculate) after_sort(nullptr, tiers ? p->sa.fs_keep[k] : nullptr, false);
    uint32_t nflag = 0;
    // (not in the pipelined mode, whose stages have a stream of their own already, nor under the stage timer, whose events sit on
    //  the plan's stream: the blocks the sample sorter's first attempt finished get their MTF + Huffman beside its second attempt)
    if (speculate && tiers && !p->pipelined && !p->timing)
        p->sa.stage_partial = [&](hipStream_t aux, const uint32_t *only) { return run_stages(aux, hipSuccess, nullptr, only, true); };
    if (e == hipSuccess) e = sa_build_finish(sort, p->sa, &nflag);
    p->sa.stage_partial = nullptr;                             // (it refers to this call's arguments)
    if (e == hipSuccess && (nflag || !speculate)) {
        // sa_build_finish has queued the other sorters for the flagged blocks on st; this pass is ordered after the
        // last of them (ev_sorted) and touches only those blocks -- those still open after the sample sorter's first attempt if
        // the others' stages have been queued beside its second one
        tm.mark(1);                                            // the sort stage ends here: the other tiers' time is the sort's
        after_sort(nullptr, p->sa.partial_used ? p->sa.ss_mask[1] : (speculate && tiers ? p->sa.fs_redo[k] : nullptr), true);   // (the blocks of the other tiers: text-like)
    }
    if (e == hipSuccess && compact) {
        if (hk && hk->before_offsets) e = hk->before_offsets(s2);
        if (e == hipSuccess) e = huff_block_offsets(s2, c.size, nb, c.block_off, c.start, c.capacity, status);
        if (e == hipSuccess) e = huff_pack(s2, p->d_mtf, p->n, n, nb, p->huff, c.enc_off, c.off_stride, c.out, 0,
                                           hk ? hk->pack_only : nullptr, c.block_off, c.capacity);
        if (e == hipSuccess && hk && hk->after_pack) e = hk->after_pack(s2);
        if (p->timing) (void)hipEventRecord(p->ev[3], s2);
    }
    tm.done();
    if (p->pipelined) { p->enc_half.release(k, s2); p->side_busy = true; }
    return hip_result(e);
}

CUDPPResult glcCompressBatch(CUDPPHandle planHandle, const unsigned char *d_uncompressed, int *d_bwtIndex,
                             unsigned int *d_hist, unsigned int *d_encodeOffset, size_t offsetStride,
                             unsigned int *d_compressedSize, unsigned int *d_compressed,
                             size_t compressedStrideWords, size_t numElements, size_t numBlocks)
{
    return compress_batch(planHandle, CompressCall{d_uncompressed, d_bwtIndex, d_hist, d_encodeOffset, offsetStride, d_compressedSize,
                                                   d_compressed, compressedStrideWords, numElements, numBlocks});
}

CUDPPResult glcCompressBatchCompact(CUDPPHandle planHandle, const unsigned char *d_uncompressed, int *d_bwtIndex,
                                    unsigned int *d_hist, unsigned int *d_encodeOffset, size_t offsetStride,
                                    unsigned int *d_compressedSize, unsigned int *d_compact, size_t capacityWords,
                                    unsigned long long *d_blockOffsets, const unsigned long long *d_startOffset,
                                    size_t numElements, size_t numBlocks)
{
    if (!d_blockOffsets || !d_compact) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return compress_batch(planHandle, CompressCall{d_uncompressed, d_bwtIndex, d_hist, d_encodeOffset, offsetStride, d_compressedSize,
                                                   d_compact, 0, numElements, numBlocks, d_blockOffsets, d_startOffset, capacityWords});
}

// the Huffman half of cudppCompress on its own (histogram, tree + codes, bit packer, offsets: rows a5-a8)
CUDPPResult glcHuffmanEncodeBatch(CUDPPHandle planHandle, const unsigned char *d_symbols, unsigned int *d_hist,
                                  unsigned int *d_encodeOffset, size_t offsetStride, unsigned int *d_compressedSize,
                                  unsigned int *d_compressed, size_t compressedStrideWords, size_t numElements,
                                  size_t numBlocks)
{
    CUDPPResult why;
    CompressPlan *p = batch_plan<CompressPlan>(planHandle, CUDPP_COMPRESS, ANY_DATATYPE, numElements, numBlocks, why);
    if (!p) return why;
    const uint32_t n = (uint32_t)numElements, nb = (uint32_t)numBlocks;
    if (offsetStride < (n + HUFF_BLOCK - 1) / HUFF_BLOCK) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    p->join_side();
    hipStream_t st = p->stream;
    hipError_t e = huff_histogram(st, d_symbols, n, n, nb, p->huff);
    if (e == hipSuccess) e = huff_build(st, n, nb, p->huff, d_hist, d_encodeOffset, offsetStride, d_compressedSize,
                                        compressedStrideWords, p->d_status);
    if (e == hipSuccess) e = huff_pack(st, d_symbols, n, n, nb, p->huff, d_encodeOffset, offsetStride, d_compressed,
                                       compressedStrideWords);
    return hip_result(e);
}

CUDPPResult glcPlanSetPipelining(CUDPPHandle planHandle, int on)
{
    PlanBase *base = plan_of(planHandle);
    if (!base) return CUDPP_ERROR_INVALID_HANDLE;
    if (base->config.algorithm != CUDPP_COMPRESS) return CUDPP_ERROR_INVALID_PLAN;
    CompressPlan *p = static_cast<CompressPlan *>(base);
    p->join_side();
    if (p->side) (void)hipStreamSynchronize(p->side);
    (void)hipStreamSynchronize(p->stream);
    p->pipelined = on != 0;
    p->enc_half.reset();
    p->dec_half.reset();
    return CUDPP_SUCCESS;
}

CUDPPResult glcBwtBatch(CUDPPHandle planHandle, const unsigned char *d_in, unsigned char *d_out, int *d_index,
                        size_t numElements, size_t numBlocks)
{
    CUDPPResult why;
    SortPlan *p = batch_plan<SortPlan>(planHandle, CUDPP_BWT, UCHAR_ONLY, numElements, numBlocks, why);
    if (!p) return why;
    const uint32_t n = (uint32_t)numElements, nb = (uint32_t)numBlocks;
    return hip_result(sa_build(SortCall{p->stream, d_in, n, n, nb, d_out, n, d_index}, p->sa));
}

CUDPPResult glcMtfBatch(CUDPPHandle planHandle, const unsigned char *d_in, unsigned char *d_out,
                        size_t numElements, size_t numBlocks)
{
    CUDPPResult why;
    MtfPlan *p = batch_plan<MtfPlan>(planHandle, CUDPP_MTF, UCHAR_ONLY, numElements, numBlocks, why);
    if (!p) return why;
    const uint32_t n = (uint32_t)numElements, nb = (uint32_t)numBlocks;
    return hip_result(mtf_forward(p->stream, d_in, n, n, nb, d_out, n, p->mtf, nullptr));
}

// the entry check of the decoder's entries, and the decoder's scratch on first use
static CompressPlan *decode_plan(CUDPPHandle planHandle, size_t numElements, size_t numBlocks, CUDPPResult &why)
{
    CompressPlan *p = batch_plan<CompressPlan>(planHandle, CUDPP_COMPRESS, ANY_DATATYPE, numElements, numBlocks, why);
    if (p && !p->dec.lf) {
        why = hip_result(decode_scratch_alloc(p->dec, p->n, p->rows));
        if (why != CUDPP_SUCCESS) return nullptr;
    }
    return p;
}

static CUDPPResult decompress_batch(CUDPPHandle planHandle, const DecodeCall &c)
{
    CUDPPResult why;
    CompressPlan *p = decode_plan(planHandle, c.n, c.nblk, why);
    if (!p) return why;
    if (!p->pipelined) return hip_result(decode_blocks(p->stream, c, p->dec, p->d_status));
    // pipelined: Huffman + inverse MTF on the plan's stream (inputs keep their stream order), the inverse
    // BWT -- a memory-latency-bound walk -- on the side stream, where it overlaps stage A of the next call.
    // d_out is complete after glcPlanSynchronize / a device synchronize.
    hipError_t e = p->pipeline_init();
    if (e != hipSuccess) return hip_result(e);
    hipStream_t st = p->stream;
    const uint32_t k = p->dec_half.take();
    uint8_t *bwt = k ? p->dec.bwt2 : p->dec.bwt;
    p->dec_half.wait_free(k, st);
    e = decode_stage_a(st, c, p->dec, bwt, p->d_status);
    (void)hipEventRecord(p->ev_dec_a[k], st);
    (void)hipStreamWaitEvent(p->side, p->ev_dec_a[k], 0);
    if (e == hipSuccess) e = decode_stage_b(p->side, c, bwt, p->dec, p->d_status);
    p->dec_half.release(k, p->side);
    p->side_busy = true;
    return hip_result(e);
}

CUDPPResult glcDecompressBatch(CUDPPHandle planHandle, const int *d_bwtIndex, const unsigned int *d_hist,
                               const unsigned int *d_encodeOffset, size_t offsetStride,
                               const unsigned int *d_compressed, size_t compressedStrideWords,
                               unsigned char *d_out, size_t numElements, size_t numBlocks)
{
    return decompress_batch(planHandle, DecodeCall{d_bwtIndex, d_hist, d_encodeOffset, offsetStride, d_compressed,
                                                   compressedStrideWords, d_out, numElements, numBlocks});
}

CUDPPResult glcDecompressBatchCompact(CUDPPHandle planHandle, const int *d_bwtIndex, const unsigned int *d_hist,
                                      const unsigned int *d_encodeOffset, size_t offsetStride,
                                      const unsigned int *d_compact, size_t compactWords,
                                      const unsigned long long *d_blockOffsets, unsigned char *d_out,
                                      size_t numElements, size_t numBlocks)
{
    if (!d_blockOffsets) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return decompress_batch(planHandle, DecodeCall{d_bwtIndex, d_hist, d_encodeOffset, offsetStride, d_compact, compactWords, d_out,
                                                   numElements, numBlocks, d_blockOffsets});
}

// the decoder stage by stage (tests, A/B timing): the Huffman step alone, the inverse of glcHuffmanEncodeBatch ...
CUDPPResult glcHuffmanDecodeBatch(CUDPPHandle planHandle, const unsigned int *d_hist, const unsigned int *d_encodeOffset,
                                  size_t offsetStride, const unsigned int *d_compressed, size_t compressedStrideWords,
                                  unsigned char *d_symbols, size_t numElements, size_t numBlocks)
{
    CUDPPResult why;
    CompressPlan *p = decode_plan(planHandle, numElements, numBlocks, why);
    if (!p) return why;
    p->join_side();
    return hip_result(decode_huff_rows(p->stream, DecodeCall{nullptr, d_hist, d_encodeOffset, offsetStride, d_compressed,
                                                              compressedStrideWords, nullptr, numElements, numBlocks},
                                       p->dec, d_symbols, numElements, p->d_status));
}

// ... and the inverse MTF alone, the inverse of glcMtfBatch
CUDPPResult glcMtfInverseBatch(CUDPPHandle planHandle, const unsigned char *d_mtf, unsigned char *d_out, size_t numElements,
                               size_t numBlocks)
{
    CUDPPResult why;
    CompressPlan *p = decode_plan(planHandle, numElements, numBlocks, why);
    if (!p) return why;
    p->join_side();
    return hip_result(decode_imtf_rows(p->stream, (uint32_t)numElements, (uint32_t)numBlocks, p->dec, d_mtf, numElements, d_out,
                                       numElements));
}

// which Huffman decode kernel the plan's decoder uses: 0 by the call's size, 1 k_dec_huff, 2 k_dec_huff_lanes
CUDPPResult glcPlanSetHuffDecoder(CUDPPHandle planHandle, int mode)
{
    PlanBase *base = plan_of(planHandle);
    if (!base) return CUDPP_ERROR_INVALID_HANDLE;
    if (base->config.algorithm != CUDPP_COMPRESS) return CUDPP_ERROR_INVALID_PLAN;
    if (mode < 0 || mode > 2) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    static_cast<CompressPlan *>(base)->dec.huff_decoder = mode;
    return CUDPP_SUCCESS;
}

// --------------------------------------------------------------------------
// the reference's single-block entry points
// --------------------------------------------------------------------------
CUDPPResult cudppCompress(CUDPPHandle planHandle, unsigned char *d_uncompressed, int *d_bwtIndex,
                          unsigned int * /*d_histSize: ignored, as compress_app.cu:507-526*/,
                          unsigned int *d_hist, unsigned int *d_encodeOffset, unsigned int *d_compressedSize,
                          unsigned int *d_compressed, size_t numElements)
{
    if (planHandle == 0) return CUDPP_ERROR_INVALID_HANDLE;
    const size_t nsub = (numElements + HUFF_BLOCK - 1) / HUFF_BLOCK;
    return glcCompressBatch(planHandle, d_uncompressed, d_bwtIndex, d_hist, d_encodeOffset, nsub ? nsub : 1,
                            d_compressedSize, d_compressed, (size_t)(HUFF_MAX_WORDS + 1) * (nsub ? nsub : 1),
                            numElements, 1);
}

CUDPPResult cudppBurrowsWheelerTransform(CUDPPHandle planHandle, unsigned char *d_in, unsigned char *d_out,
                                         int *d_index, size_t numElements)
{
    if (planHandle == 0) return CUDPP_ERROR_INVALID_HANDLE;
    return glcBwtBatch(planHandle, d_in, d_out, d_index, numElements, 1);
}

CUDPPResult cudppMoveToFrontTransform(CUDPPHandle planHandle, unsigned char *d_in, unsigned char *d_out,
                                      size_t numElements)
{
    if (planHandle == 0) return CUDPP_ERROR_INVALID_HANDLE;
    return glcMtfBatch(planHandle, d_in, d_out, numElements, 1);
}

CUDPPResult cudppSuffixArray(CUDPPHandle planHandle, unsigned char *d_str, unsigned int *d_keys_sa,
                             size_t numElements)
{
    CUDPPResult why;
    SortPlan *p = batch_plan<SortPlan>(planHandle, CUDPP_SA, UCHAR_ONLY, numElements, 1, why);   // (one block: a plan has a row at least)
    if (!p) return why;
    const uint32_t n = (uint32_t)numElements;
    hipError_t e = sa_build(SortCall{p->stream, d_str, n, n, 1, nullptr, 0, nullptr}, p->sa);
    if (e == hipSuccess) e = sa_export(p->stream, p->sa.sa, n, d_keys_sa);
    return hip_result(e);
}

// --------------------------------------------------------------------------
// plan utilities
// --------------------------------------------------------------------------
CUDPPResult glcPlanSetStream(CUDPPHandle planHandle, void *hipStream)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    p->stream = reinterpret_cast<hipStream_t>(hipStream);
    return CUDPP_SUCCESS;
}

__global__ void k_status_fetch(uint32_t *__restrict__ d_status, uint32_t *__restrict__ h_status)
{
    *reinterpret_cast<volatile uint32_t *>(h_status) = *d_status;
    *d_status = 0;
}

CUDPPResult glcPlanSynchronize(CUDPPHandle planHandle)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    p->join_side();
    // status word: fetched into pinned memory and cleared by ONE small kernel (a copy command + a fill command were two more
    // ~5 us links in the chain a cudppCompress caller waits for)
    hipLaunchKernelGGL(k_status_fetch, dim3(1), dim3(1), 0, p->stream, p->d_status, p->h_status);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) return CUDPP_ERROR_UNKNOWN;
    if (p->timing && p->ev_valid) read_spans(p);
    return *p->h_status ? CUDPP_ERROR_UNKNOWN : CUDPP_SUCCESS;
}

CUDPPResult glcPlanEnableTiming(CUDPPHandle planHandle, int enable)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    p->timing = enable != 0;
    p->ev_valid = false;
    if (!p->prof.enable((enable & 2) != 0)) return CUDPP_ERROR_INSUFFICIENT_RESOURCES;
    p->prof.reset();
    p->wire_prof();
    return CUDPP_SUCCESS;
}

CUDPPResult glcPlanSetSorter(CUDPPHandle planHandle, int mode)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    SaScratch *s = p->sorter();
    if (!s) return CUDPP_ERROR_INVALID_PLAN;
    if (mode < 0 || mode > 7) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    s->sorter = mode >= 5 ? 0 : mode;
    s->resume_min = mode == 5 ? 0u : (mode == 6 ? 1u : 2u);
    s->periodic = mode != 7 && mode != 5;                      // (5: "from scratch" for everything the sample sorter gives up on)
    return CUDPP_SUCCESS;
}

CUDPPResult glcPlanLastSortStats(CUDPPHandle planHandle, unsigned int *flaggedBlocks)
{
    return with_sorter(planHandle, flaggedBlocks, [&](SaScratch &s) { *flaggedBlocks = s.stats.flagged; });
}

CUDPPResult glcPlanLastSortStatsEx(CUDPPHandle planHandle, unsigned int *out2)
{
    return with_sorter(planHandle, out2, [&](SaScratch &s) { out2[0] = s.stats.flagged; out2[1] = s.stats.general; });
}

// out[0] = blocks of the plan's last call that the sample sorter took in a second attempt (other samples)
CUDPPResult glcPlanLastSortRetries(CUDPPHandle planHandle, unsigned int *out)
{
    return with_sorter(planHandle, out, [&](SaScratch &s) { out[0] = s.stats.retried; });
}

// out[0] = 1 if the plan's last call skipped the bucket sorter's attempt (sorter mode 4, or a small call behind a streak of calls
// whose every block the text-likeness probe flagged), out[1] = the streak
CUDPPResult glcPlanLastSortSkipped(CUDPPHandle planHandle, unsigned int *out2)
{
    return with_sorter(planHandle, out2, [&](SaScratch &s) { out2[0] = s.stats.skipped ? 1u : 0u; out2[1] = s.textlike_streak; });
}

// out[0] = blocks of the plan's last call that the periodic tier finished
CUDPPResult glcPlanLastSortPeriodic(CUDPPHandle planHandle, unsigned int *out)
{
    return with_sorter(planHandle, out, [&](SaScratch &s) { out[0] = s.stats.periodic; });
}

// out[0] = blocks of the plan's last call whose doubling rounds resumed from the sample sorter's tolerant form
CUDPPResult glcPlanLastSortResumed(CUDPPHandle planHandle, unsigned int *out)
{
    return with_sorter(planHandle, out, [&](SaScratch &s) { out[0] = s.stats.resumed; });
}

// out2[0] = chain groups the plan's last call ordered by the rule, out2[1] = candidates the verification or the direction refused
CUDPPResult glcPlanLastSortChains(CUDPPHandle planHandle, unsigned int *out2)
{
    return with_sorter(planHandle, out2, [&](SaScratch &s) { out2[0] = s.stats.chains[0]; out2[1] = s.stats.chains[1]; });
}

// chain groups of the doubling rounds: the plan's attempt schedule (minLive < 0 / roundMask == ~0u restore the defaults)
CUDPPResult glcPlanSetChains(CUDPPHandle planHandle, long minLive, unsigned int roundMask)
{
    return with_sorter(planHandle, true, [&](SaScratch &s) {
        long dmin;
        uint32_t dmask;
        sa_chain_defaults(&dmin, &dmask);
        s.chain_min = minLive < 0 ? dmin : minLive;
        s.chain_rounds = roundMask == ~0u ? dmask : roundMask;
    });
}

// diagnostic: the give-up flags of the plan's last sort, per block (waits for the plan's stream).  out_fs[b]: bucket sorter
// (1 = a bucket overflowed / flagged up front as text-like, 2 = equal codes deeper than the cap, 4 = work list full);
// out_ss[b]: sample sorter (1 = a bucket overflowed, 2 = deeper than its cap / a run no window holds)
CUDPPResult glcPlanDebugSortFlags(CUDPPHandle planHandle, unsigned int *out_fs, unsigned int *out_ss, size_t numBlocks)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    SaScratch *s = p->sorter();
    if (!s || numBlocks > s->rows) return CUDPP_ERROR_INVALID_PLAN;
    if (hipStreamSynchronize(p->stream) != hipSuccess) return CUDPP_ERROR_UNKNOWN;
    if (out_fs && hipMemcpy(out_fs, s->fs_flag, numBlocks * 4, hipMemcpyDeviceToHost) != hipSuccess) return CUDPP_ERROR_UNKNOWN;
    if (out_ss && hipMemcpy(out_ss, s->ss_flag, numBlocks * 4, hipMemcpyDeviceToHost) != hipSuccess) return CUDPP_ERROR_UNKNOWN;
    return CUDPP_SUCCESS;
}

// diagnostic: bucket fills of block `block` as the last bucketing pass left them (FS_MAXNB = 512 entries)
CUDPPResult glcPlanDebugBucketFill(CUDPPHandle planHandle, size_t block, unsigned int *out512)
{
    PlanBase *p = plan_of(planHandle, out512);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    SaScratch *s = p->sorter();
    if (!s || block >= s->rows) return CUDPP_ERROR_INVALID_PLAN;
    if (hipStreamSynchronize(p->stream) != hipSuccess) return CUDPP_ERROR_UNKNOWN;
    return hipMemcpy(out512, s->fs_fill + block * FS_MAXNB, FS_MAXNB * 4, hipMemcpyDeviceToHost) == hipSuccess ? CUDPP_SUCCESS : CUDPP_ERROR_UNKNOWN;
}

// diagnostic, process-wide: the fill seam of the scratch allocation helpers (glc_internal.h)
void glcDebugSetScratchFill(unsigned int on, unsigned int word)
{
    g_scratch_fill = ScratchFill{on ? 1u : 0u, word, 0, 0};
}

void glcDebugScratchFillStats(unsigned long long out2[2])
{
    if (!out2) return;
    out2[0] = g_scratch_fill.blocks;
    out2[1] = g_scratch_fill.bytes;
}

// the event pairs are read when the plan's streams are idle: both getters wait for them first
static void prof_collect(PlanBase *p)
{
    if (p->prof.npend == 0) return;
    p->join_side();
    (void)hipStreamSynchronize(p->stream);
    p->prof.collect();
}

CUDPPResult glcPlanKernelProfileEx(CUDPPHandle planHandle, int index, char *name, size_t nameCap, double *out3)
{
    PlanBase *p = plan_of(planHandle, out3);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    if (index < 0 || index >= PROF_NSLOT) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    prof_collect(p);
    out3[0] = p->prof.ms[index]; out3[1] = (double)p->prof.launches[index]; out3[2] = p->prof.units[index];
    if (name && nameCap) { strncpy(name, p->prof.name[index], nameCap - 1); name[nameCap - 1] = 0; }
    return CUDPP_SUCCESS;
}

// the kernel with the largest accumulated launch time: {ms, launches, input bytes processed}; resets the profile
CUDPPResult glcPlanKernelProfile(CUDPPHandle planHandle, double *out3)
{
    PlanBase *p = plan_of(planHandle, out3);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    prof_collect(p);
    int best = 0;
    for (int k = 1; k < PROF_NSLOT; k++) if (p->prof.ms[k] > p->prof.ms[best]) best = k;
    out3[0] = p->prof.ms[best]; out3[1] = (double)p->prof.launches[best]; out3[2] = p->prof.units[best];
    p->prof.reset();
    return CUDPP_SUCCESS;
}

// launches the live profile could not account for: out2[0] = not bracketed (more than 4096 launches pending between two
// reads), out2[1] = bracketed but unreadable
CUDPPResult glcPlanKernelProfileLost(CUDPPHandle planHandle, unsigned long long *out2)
{
    PlanBase *p = plan_of(planHandle, out2);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    out2[0] = (unsigned long long)p->prof.dropped; out2[1] = (unsigned long long)p->prof.unread;
    return CUDPP_SUCCESS;
}

CUDPPResult glcCompactStreams(CUDPPHandle planHandle, const unsigned int *d_compressed,
                              size_t compressedStrideWords, const unsigned int *d_compressedSize,
                              size_t numBlocks, unsigned int *d_out, unsigned long long *d_outOffsets)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    if (!d_compressed || !d_compressedSize || !d_out || !d_outOffsets || numBlocks == 0)
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    p->join_side();
    return hip_result(compact_streams(p->stream, d_compressed, compressedStrideWords, d_compressedSize,
                                      (uint32_t)numBlocks, d_out, d_outOffsets));
}

CUDPPResult glcExpandStreams(CUDPPHandle planHandle, const unsigned int *d_in, const unsigned long long *d_inOffsets,
                             size_t numBlocks, unsigned int *d_compressed, size_t compressedStrideWords,
                             unsigned int *d_compressedSize)
{
    PlanBase *p = plan_of(planHandle);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    if (!d_in || !d_inOffsets || !d_compressed || numBlocks == 0 || compressedStrideWords == 0)
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    p->join_side();
    return hip_result(expand_streams(p->stream, d_in, d_inOffsets, (uint32_t)numBlocks, d_compressed,
                                     compressedStrideWords, d_compressedSize, p->d_status));
}

CUDPPResult glcPlanLastTiming(CUDPPHandle planHandle, float *ms4)
{
    PlanBase *p = plan_of(planHandle, ms4);
    if (!p) return CUDPP_ERROR_INVALID_HANDLE;
    for (int i = 0; i < 4; i++) ms4[i] = p->last_ms[i];
    return CUDPP_SUCCESS;
}

} // extern "C"

namespace glc {
// the one place a HIP error becomes a result code (glc_internal.h); the error is not left sticky for the caller's next HIP call
CUDPPResult hip_result(hipError_t e)
{
    if (e == hipSuccess) return CUDPP_SUCCESS;
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? CUDPP_ERROR_INSUFFICIENT_RESOURCES : CUDPP_ERROR_UNKNOWN;
}

// internal: the container path (container_api.cpp) drives a plan through these
CUDPPResult plan_compress_hooked(CUDPPHandle planHandle, CompressCall c, ContainerHooks &hk)
{
    c.hooks = &hk;
    return compress_batch(planHandle, c);
}

bool plan_info(CUDPPHandle planHandle, uint32_t *n, uint32_t *rows, hipStream_t *st, uint32_t *next_parity)
{
    PlanBase *p = plan_of(planHandle);
    if (!p || p->config.algorithm != CUDPP_COMPRESS || p->config.datatype != CUDPP_UCHAR) return false;
    if (n) *n = p->n;
    if (rows) *rows = p->rows;
    if (st) *st = p->stream;
    if (next_parity) *next_parity = static_cast<CompressPlan *>(p)->enc_half.next();
    return true;
}

void plan_join(CUDPPHandle planHandle) { plan_from<CompressPlan>(planHandle)->join_side(); }

bool plan_pipelined(CUDPPHandle planHandle) { return plan_from<CompressPlan>(planHandle)->pipelined; }
CtSettings &plan_container_settings(CUDPPHandle planHandle) { return plan_from<CompressPlan>(planHandle)->ct; }
CtReports &plan_container_reports(CUDPPHandle planHandle) { return plan_from<CompressPlan>(planHandle)->ct_reports; }

hipError_t plan_stage(CUDPPHandle planHandle, uint32_t which, size_t bytes, uint8_t **out)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    return p->ct_stage[which].grow(*p, bytes, out);
}

hipError_t plan_codec_scratch(CUDPPHandle planHandle, uint32_t which, size_t bytes, uint8_t **out)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    return p->ct_codec[which].grow(*p, bytes, out);
}

hipError_t plan_pinned_scratch(CUDPPHandle planHandle, uint32_t which, size_t bytes, void **out)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    return p->ct_pinned[which].grow(*p, bytes, out);
}

KernelProf *plan_prof(CUDPPHandle planHandle) { return &plan_from<CompressPlan>(planHandle)->prof; }

void plan_stage_mark(CUDPPHandle planHandle, int i)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    if (!p->timing) return;
    StageTimer tm(p);
    tm.mark(i);
    if (i == 1 && p->pipelined && p->ev_s2) (void)hipEventRecord(p->ev_s2, p->stream);   // (glcPlanSynchronize reads the second span from it)
    if (i == 3) tm.done();
}

hipError_t plan_bwt_mtf(CUDPPHandle planHandle, const uint8_t *in, uint32_t n, uint32_t nb, int *bwt_index, const uint8_t **mtf, size_t *stride)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    p->join_side();                                            // (an earlier pipelined call may still read d_bwt / d_mtf there)
    p->sa.parity = p->enc_half.next();
    hipError_t e = sa_build(SortCall{p->stream, in, n, n, nb, p->d_bwt, p->n, bwt_index}, p->sa);
    if (e == hipSuccess) e = mtf_forward(p->stream, p->d_bwt, p->n, n, nb, p->d_mtf, p->n, p->mtf, nullptr);
    *mtf = p->d_mtf; *stride = p->n;
    return e;
}

hipError_t plan_decode_rows(CUDPPHandle planHandle, uint8_t **mtf, size_t *stride)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    if (!p->dec.lf) {
        const hipError_t e = decode_scratch_alloc(p->dec, p->n, p->rows);
        if (e != hipSuccess) return e;
    }
    *mtf = p->dec.mtf; *stride = p->dec.nmax;
    return hipSuccess;
}

hipError_t plan_decode_from_mtf(CUDPPHandle planHandle, uint32_t first_row, const int *bwt_index, uint8_t *out, uint32_t n, uint32_t nblk)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    if (!p->dec.lf || first_row + nblk > p->dec.rows) return hipErrorInvalidValue;
    p->join_side();                                            // (stage B of an earlier pipelined call uses the same scratch)
    return decode_mtf_blocks(p->stream, DecodeCall{bwt_index, nullptr, nullptr, 0, nullptr, 0, out, n, nblk},
                             p->dec.mtf + (size_t)first_row * p->dec.nmax, p->dec, p->d_status);
}

void plan_wait_released(CUDPPHandle planHandle)
{
    CompressPlan *p = plan_from<CompressPlan>(planHandle);
    if (p->pipelined) p->enc_half.wait_free(p->enc_half.next(), p->stream);
}
} // namespace glc
