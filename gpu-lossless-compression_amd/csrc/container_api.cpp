// container_api.cpp -- the C ABI of include/glc_container.h that works on a COMPRESS plan: the BWT container,
// its frame index and range reads, what the plan reports of its last calls, and the plan's container settings.  (The plan-less
// segment calls of that header -- CRC, filters, sparse, dedup, zero-run, rANS, the probes -- are segments_api.cpp.)
//
// Format.  A stream is a header, frames and a trailer.  Its header's triple (version, flags, elem) is a CtFormat, and a format says
// two things: the FILTER every frame's bytes go through as one segment before the frame's blocks are cut (none, the byte-plane
// shuffle of shuffle.hip, the fused delta + shuffle of delta.hip, under version 11 that delta with the flags' lag and fold, lag.hip,
// under version 12 the 2-D predictor of grid.hip with the row width of the header's word 3, or under version 15 the byte predictor
// of byte_delta.hip with the flags' lag and word 3's row stride, or under version 17 the 3-D predictor of vol.hip with word 3's row
// width and the plane stride of the header's word 7),
// and which record KINDS a frame may hold (0 BWT + Huffman and
// 1 raw always; 2 order-0 Huffman, 3 its sparse form (sparse.hip), 4 the BWT codec's zero-run form (zrun.hip), 5 the order-0
// codec's rANS form (ans.hip) and 6 its dedup form (dedup.hip) where kind2_legal() .. kind6_legal() say so).  ct_legal() is the
// one table of legal triples: format_of() picks the writer's from the plan's settings (the lowest version whose kinds hold every
// kind they may write), parse_format() accepts a reader's.  Under format version 10 (filter-auto) the filter is each FRAME's: the
// stream's triple is (10, 0, 0), word 3 of a frame header names the frame's filter, and ct_frame_format() gives the format a frame
// went through -- the writer picks it per frame from the filter probe (filter_probe.hip, filter_rule.h; one host read of seven
// costs per frame), the readers take it from the frame.  Format version 13 (filter-lag) is version 10 whose frame word may also
// carry version 11's lag and fold: the writer enqueues the lag probe behind the filter probe (lag_probe.hip, lag_rule.h) and
// reads ten costs and three lags with the same one wait; its triple (13, 0, 0) is parse_stream_format()'s.  Format version 14
// (filter-grid) is version 13 whose frame word may also name the 2-D predictor of version 12: the grid probe (grid_probe.hip,
// grid_rule.h) is enqueued behind the lag probe, and the one wait brings thirteen costs, three lags and three widths.  With
// glcPlanSetContainerFilterByte the stream is version 16: a frame word may also name the byte predictor at a lag and a row stride,
// the byte probe (byte_probe.hip, byte_rule.h) is enqueued behind the grid probe, and the one wait brings fifteen costs, three
// lags, three widths and the byte lag and stride.
//
// Encode (Encoder).  A filtered frame is staged through filter_device() into staging kept with the plan and encoded from there;
// crc_all is taken over the original bytes.  With the BWT codec one hooked glcCompressBatchCompact per frame writes the Huffman
// records straight into the container; with its runs mode on (frame_runs, kind 4) the plan's sorter and MTF stage feed the
// zero-run split and the batched order-0 encoder.  With the order-0 codec (hd_batch.hip) frame_order0 is the one path: a mode hands
// it its parts -- what gives every block's record size, the kinds kernel where the mode has its own, and what writes the records
// behind the payload offsets.  frame_plain: batched histograms and tables, kind 2.  frame_sparse: kinds 2 and 3.  frame_ans: kind
// 5, the histograms alone and the kernels of ans.hip.  frame_auto: the probe of auto.hip and a kind per block out of 2, 3 and 5.
// frame_dedup (kind 6, format version 9): the map of the frame's 512-byte chunks runs first, the chunks that repeat an earlier
// chunk of the frame are elided, and the sparse mode's compaction and the batched encoder work on what is kept.  Either way the
// kernels of container.hip decide the record kinds before the payload offsets are scanned, copy the raw records, CRC everything
// and write the frame's tables behind the packer.  Frames chain on the device (a cursor word): no host read inside or between
// frames, one at the end.  With the CHOOSE codec (super_frame) the bigram probe of choose.hip runs over what is one frame
// otherwise, its stats rows are read back (the one host read per such group), the rule of choose_rule.h picks the BWT or the
// order-0 codec per block, and every maximal run of blocks of one choice becomes one frame by that codec's path above: format
// version 3, kinds 0, 1 and 2, no reader change.  With glcPlanSetContainerChooseFilters (class_rule.h) the order-0 frames take the
// auto mode and the filter-auto ladder up to the level's step: from level 2 on the filter probe (at level 5 the byte probe's lag
// sums and rows as well) runs over the same blocks as segments, the same one read brings their costs, a frame is cut wherever a
// block's class -- BWT, or order-0 with the element size its costs pick -- changes, and an order-0 frame's filter is pick_filter's
// over the whole frame; the stream is version 8, 10, 13, 14 or 16, whose readers take kind-0 runs already.
//
// Decode (Decoder).  decode_walk() runs ct_walk() (container_internal.h), the one loop over a stream's headers, fed either from
// the caller's device buffers or from a Source through staging; the frame index (glcContainerIndex*) is the same walk without the
// decoding, and a range read (glcContainerReadRange*) decodes a subset of the blocks of the frames its range overlaps.  Per frame
// the host range-checks the 32-byte frame header, the device checks the tables and records (one verdict read back), then raw
// records are copied out and for_runs() hands every maximal run of blocks of one kind to that kind's decoder: kind 0 to
// glcDecompressBatchCompact reading the tables in place, kind 2 to the batched order-0 decoder, kind 3 to it as well (the kept
// bytes into scratch, then expanded under the record's mask), kind 4 to it too (A and B into scratch, joined into the BWT
// decoder's MTF rows, then its inverse MTF and inverse BWT), kind 5 to the rANS decoder (tables from the verified histograms, then
// one pass), kind 6 to the order-0 decoder and the sparse join (the kept chunks put back; one fill pass then copies the elided
// ones from their sources).  The decoded bytes are checked against the blocks' CRCs; a filtered frame is decoded into staging,
// checked there and inverted into the output by filter_device().
//
// Reports and settings.  What glcContainerLastError, LastRangeStats, LastChoice and LastFilters answer is one CtReports kept in the
// plan: it starts with the plan and goes with it, and two plans share nothing.  The glcPlanSet/GetContainer* entries are ct_set()
// and ct_get() over the plan's CtSettings, whose set_*() are the whole rule.
#include "../../include/glc_container.h"
#include "container_internal.h"
#include "dedup_rule.h"
#include "byte_rule.h"
#include "filter_rule.h"
#include "grid_rule.h"
#include "lag_rule.h"

#include <fcntl.h>
#include <memory>
#include <new>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

using namespace glc;

// the frame index of one container (glcContainerIndex*): what the walk over its headers found, kept on the host
struct GlcContainerIndex {
    uint32_t hdr[8] = {}, trailer[4] = {};                    // copies of the stream header and of the trailer
    unsigned long long len = 0, total = 0;                    // container bytes; input bytes
    uint32_t block_len = 0;
    CtFormat fmt;
    std::vector<CtFrameRef> frames;
};

namespace glc {
static const CrcTables h_crc = crc_make_tables();
uint32_t crc32_host(const void *data, size_t len, uint32_t crc)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    uint32_t r = ~crc;
    for (size_t i = 0; i < len; i++) r = h_crc.t[0][(r ^ p[i]) & 255] ^ (r >> 8);
    return ~r;
}
} // namespace glc

namespace {

// what glcContainerLastError reports: kept with the plan (CtReports), like everything a plan's calls leave behind
void set_error(CUDPPHandle plan, unsigned long long what, unsigned long long frame = ~0ull, unsigned long long block = ~0ull)
{
    unsigned long long *e = plan_container_reports(plan).error;
    e[0] = what; e[1] = frame; e[2] = block;
}

CUDPPResult fail(CUDPPHandle plan, unsigned long long what, unsigned long long frame = ~0ull, unsigned long long block = ~0ull)
{
    set_error(plan, what, frame, block);
    return what == CT_CAPACITY ? CUDPP_ERROR_ILLEGAL_CONFIGURATION : CUDPP_ERROR_UNKNOWN;
}

#define CT_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

struct Plan {
    CUDPPHandle h = 0;
    uint32_t n = 0, rows = 0, parity = 0;
    hipStream_t st = nullptr;
    bool ok(CUDPPHandle plan) { h = plan; return plan != 0 && plan != CUDPP_INVALID_HANDLE && plan_info(plan, &n, &rows, &st, &parity); }
    // what the entry points that tell a bad handle from a plan of another kind return
    CUDPPResult check(CUDPPHandle plan)
    {
        if (ok(plan)) return CUDPP_SUCCESS;
        return plan == 0 || plan == CUDPP_INVALID_HANDLE ? CUDPP_ERROR_INVALID_HANDLE : CUDPP_ERROR_INVALID_PLAN;
    }
};

// worst case of one frame of nb blocks of blk_len (raw records)
unsigned long long frame_bound(uint32_t nb, uint32_t blk_len)
{
    return frame_bytes(nb, blk_len, (unsigned long long)nb * ct_raw_words(blk_len) + nb);
}

// -------------------------------------------------------------------------------------------------------------------------
// the format rule (ct_legal() and format_of() of container_internal.h: the table the device's walk reads as well)
// -------------------------------------------------------------------------------------------------------------------------
void make_header(uint32_t h[8], const CtFormat &f, uint32_t block_len, unsigned long long total)
{
    h[0] = CT_MAGIC_STREAM; h[1] = f.version | (f.flags << 16);
    h[2] = block_len; h[3] = f.word3();
    h[4] = (uint32_t)total; h[5] = (uint32_t)(total >> 32);
    h[7] = f.plane;                                            // (0 but under version 17, whose CRC covers it)
    h[6] = ct_header_crc(h, [](const uint32_t *w, size_t n) { return crc32_host(w, n); });
}

// measure with a null Carver, allocate (alloc(bytes, &base) -> hipError_t), carve again on the allocation
template <class Alloc, class Carve>
hipError_t carve_on(Alloc alloc, Carve carve)
{
    Carver measure;
    carve(measure);
    void *base = nullptr;
    CT_HIP(alloc(measure.bytes(), &base));
    Carver place(base);
    carve(place);
    return hipSuccess;
}
// alloc for carve_on: the plan's codec scratch `which` (plan_codec_scratch)
auto codec_scratch(CUDPPHandle plan, uint32_t which)
{
    return [=](size_t bytes, void **base) { return plan_codec_scratch(plan, which, bytes, reinterpret_cast<uint8_t **>(base)); };
}

// -------------------------------------------------------------------------------------------------------------------------
// encoder: device scratch for two frames (the plan's call parity) of up to `rows` blocks, and the running state
// -------------------------------------------------------------------------------------------------------------------------
struct Encoder {
    Plan P;
    void *mem = nullptr;
    CtEncState *state = nullptr;
    uint32_t *status = nullptr;
    unsigned long long *d_len = nullptr;
    CtEncFrame fr[2] = {};
    CtFormat fmt;                                             // what the plan's settings write
    uint32_t codec = CT_CODEC_BWT;                            // the plan's container codec
    CtMode mode = CT_MODE_PLAIN;                              // and its mode (one that fits the codec: CtSettings keeps that)
    CtEncHuff0 h0 = {};                                       // the order-0 codec's scratch, kept with the plan
    CtEncSparse sp = {};                                      // the sparse mode's, behind h0's; a plan that never has it on has none
    CtEncRuns zr = {};                                        // the runs mode's, kept with the plan; a plan that never has it on has none
    CtEncAns an = {};                                         // the rANS mode's, behind h0's; a plan that never has it on has none
    CtEncAuto au = {};                                        // the auto mode's: both scratches above and its own
    CtEncDedup dd = {};                                       // the dedup mode's: the sparse mode's scratch (masks, compaction space) and its own
    uint8_t *stage[2] = {nullptr, nullptr};                   // the plan's frame staging, by call parity when pipelined
    unsigned long long *ch_stats = nullptr, *h_stats = nullptr;   // the CHOOSE codec's probe rows [rows][4]: device, pinned
    // choose-filters (class_rule.h): the level; from level 2 on the filter probe's rows and seven costs of every block of a
    // super-frame, at level 5 the byte probe's lag sums, {lag, 0} words, rows and two costs of every block as well.  The cost rows
    // lie behind ch_stats ([rows][4], [rows][7], [rows][2]), so that one copy brings all of a super-frame's statistics
    uint32_t level = 0;
    uint32_t *cf_planes = nullptr, *cb_words = nullptr, *cb_planes = nullptr;
    unsigned long long *cf_costs = nullptr, *cb_costs = nullptr, *cb_lag_sums = nullptr;
    static constexpr size_t CLASS_HOST_WORDS = CHOOSE_STATS + FILTER_CANDS + BYTE_ROWS;       // 64-bit words a block, device and pinned
    CtReports rep;                                            // this call's choice and filters, committed when it succeeds
    // filter-auto (format version 10): the filter probe's rows and costs of one frame, the frame as its one segment {offset, length},
    // the costs on the host (pinned); rep.filters counts the frames each candidate got (the plan's own filter's candidate with the
    // setting off)
    bool filter_auto = false;
    uint32_t own_pick = 0;                                    // the candidate every frame counts for with the setting off
    uint32_t *fp_planes = nullptr;
    // filter-lag (format version 13): the lag probe's sums, winners and rows of the same frame; its three costs lie behind the filter
    // probe's seven and its winners behind those, so that one copy brings all thirteen words to the host
    bool filter_lag = false;
    unsigned long long *lp_sums = nullptr;
    uint32_t *lp_lags = nullptr, *lp_planes = nullptr;
    // filter-grid (format version 14): the grid probe's sums, winners and rows of the same frame; its three costs lie behind the lag
    // probe's, the lags behind those and the widths behind the lags: one copy brings all of it
    bool filter_grid = false;
    uint32_t *gw_sums = nullptr, *gw_widths = nullptr, *gw_planes = nullptr;
    // filter-byte (format version 16): the byte probe's sums, winners and rows of the same frame; its two costs lie behind the grid
    // probe's, and its lag and stride words behind the widths: one copy brings all of it
    bool filter_byte = false;
    unsigned long long *bp_lag_sums = nullptr;
    uint32_t *bp_sums = nullptr, *bp_words = nullptr, *bp_planes = nullptr;
    unsigned long long *fp_costs = nullptr, *fp_seg = nullptr, *h_costs = nullptr;

    // everything of a runs frame is on the plan's stream in order, so one set serves pipelined calls as well
    void carve_runs(Carver &c)
    {
        const size_t R = P.rows;
        zr.x_off = c.take<unsigned long long>(R);
        zr.x_len = c.take<unsigned long long>(R);
        zr.seg_off = c.take<unsigned long long>(2 * R);
        zr.seg_len = c.take<unsigned long long>(2 * R);
        zr.nun = c.take<unsigned long long>(2 * R);
        zr.unit_off = c.take<unsigned long long>(2 * R);
        zr.skip_enc = c.take<uint32_t>(2 * R);
        zr.skip_b = c.take<uint32_t>(R);
        zr.nz = c.take<uint32_t>(R);
        zr.hist_b = c.take<uint32_t>(256 * R);
        zr.codes = c.take<uint16_t>(256 * 2 * R);
        zr.lens = c.take<uint8_t>(256 * 2 * R);
        c.align(256);
        zr.work = c.take<uint8_t>(hdb_encode_work_bytes(2 * R));
        c.align(256);
        zr.stride = (P.n + 15u) & ~15u;
        zr.a = c.take<uint8_t>(R * zr.stride);
        zr.b = c.take<uint8_t>(R * zr.stride);
    }
    void carve_huff0(Carver &c)
    {
        const size_t R = P.rows;
        const bool sparse = mode == CT_MODE_SPARSE || mode == CT_MODE_AUTO || mode == CT_MODE_DEDUP, ans = mode == CT_MODE_ANS || mode == CT_MODE_AUTO;
        h0.nun = c.take<unsigned long long>(R);
        h0.blk_off = c.take<unsigned long long>(R);
        h0.blk_len = c.take<unsigned long long>(R);
        h0.codes = c.take<uint16_t>(256 * R);
        h0.lens = c.take<uint8_t>(256 * R);
        c.align(256);
        h0.work = c.take<uint8_t>(hdb_encode_work_bytes(R));
        if (ans) {
            // everything of a frame runs on the plan's stream in order, so one set of chunk slots serves pipelined calls as well
            const size_t slots = R * ans_chunks(P.n);
            an.sc.nch_max = ans_chunks(P.n);
            an.sc.states = c.take<uint32_t>(slots * ANS_LANES);
            an.sc.counts = c.take<uint32_t>(slots);
            an.skip_ans = c.take<uint32_t>(R);
            c.align(256);
            an.tab = c.take<uint8_t>(R * ANS_TAB_BYTES);
            an.sc.units = c.take<uint16_t>(slots * ANS_CHUNK);
        }
        if (mode == CT_MODE_AUTO) {
            au.uniform = c.take<uint32_t>(256 * R);
            au.hist_s = c.take<uint32_t>(256 * R);
            au.wa = c.take<uint32_t>(R);
            au.pick5 = c.take<uint32_t>(R);
        }
        if (!sparse) return;
        // everything of a frame runs on the plan's stream in order, so one compaction space serves pipelined calls as well
        sp.mask_stride = sp_mask_words(P.n);
        sp.kept_stride = (P.n + 15u) & ~15u;
        sp.klen = c.take<unsigned long long>(R);
        sp.kept_off = c.take<unsigned long long>(R);
        sp.unit_off = c.take<unsigned long long>(R);
        h0.in_off = c.take<unsigned long long>(R);
        h0.in_len = c.take<unsigned long long>(R);
        sp.mask = c.take<uint32_t>(R * sp.mask_stride);
        sp.fill = c.take<uint32_t>(R);
        sp.is3 = c.take<uint32_t>(R);
        sp.skip_move = c.take<uint32_t>(R);
        sp.skip_table = c.take<uint32_t>(R);
        c.align(256);
        sp.kept = c.take<uint8_t>(R * sp.kept_stride);
        if (mode != CT_MODE_DEDUP) return;
        // the map's table and hashes, the map itself and what the records take from it: ONE set whether pipelining is on or off,
        // like the compaction space -- everything of a dedup frame runs on the plan's stream in order, so a second set would never
        // be in use.  It grows with the plan's codec scratch, whose growth joins the side stream first (GrowBuf).
        dd.nch = (P.n + DD_CHUNK - 1) / DD_CHUNK;
        dd.mask_stride = (dd.nch + 31) / 32;
        dd.slots = (uint32_t)dedup_slots(R * dd.nch);
        dd.src = c.take<uint32_t>(R * dd.nch);
        dd.refs = c.take<uint32_t>(R * dd.nch);
        dd.mask = c.take<uint32_t>(R * dd.mask_stride);
        dd.E = c.take<uint32_t>(R);
        dd.lo = c.take<uint32_t>(R);
        c.align(16);
        dd.table = c.take<DdSlot>((size_t)dd.slots + 1);
        dd.hash = c.take<uint64_t>(R * dd.nch);
    }
    void carve(Carver &c)
    {
        const size_t R = P.rows, nsub = (P.n + HUFF_BLOCK - 1) / HUFF_BLOCK;
        state = c.take<CtEncState>(1); c.round(64);
        status = c.take<uint32_t>(1); c.round(64);
        d_len = c.take<unsigned long long>(1); c.round(256);
        for (auto &f : fr) {
            f.boff = c.take<unsigned long long>(R + 1);
            f.seg_off = c.take<unsigned long long>(2 * R + 2);
            f.seg_len = c.take<unsigned long long>(2 * R + 2);
            f.start = c.take<unsigned long long>(1);
            f.kind = c.take<uint32_t>(R);
            f.size = c.take<uint32_t>(R);
            f.only = c.take<uint32_t>(R);
            f.hist = c.take<uint32_t>(256 * R);
            f.enc_off = c.take<uint32_t>(R * nsub);
            f.crc = c.take<uint32_t>(2 * R + 2);
            f.bwt = c.take<int>(R);
            f.tcrc = c.take<uint32_t>(2);
            c.round(256);
        }
        if (codec == CT_CODEC_CHOOSE) ch_stats = c.take<unsigned long long>(CHOOSE_STATS * R);
        if (level >= 2) {
            cf_costs = c.take<unsigned long long>(FILTER_CANDS * R);
            cb_costs = c.take<unsigned long long>(BYTE_ROWS * R);
            c.align(16);
            cf_planes = c.take<uint32_t>(FILTER_ROWS * 256 * R);
        }
        if (level >= 5) {
            cb_planes = c.take<uint32_t>(BYTE_ROWS * 256 * R);
            cb_lag_sums = c.take<unsigned long long>(BYTE_LAGS * R);
            cb_words = c.take<uint32_t>(2 * R);
        }
        if (filter_auto) {
            fp_planes = c.take<uint32_t>(FILTER_ROWS * 256);
            fp_costs = c.take<unsigned long long>(FP_HOST_WORDS);
            lp_lags = reinterpret_cast<uint32_t *>(fp_costs + ncosts());
            gw_widths = lp_lags + 4;
            bp_words = lp_lags + 8;
            fp_seg = c.take<unsigned long long>(2);
            if (filter_lag) {
                lp_sums = c.take<unsigned long long>(LAG_SUMS);
                c.align(16);
                lp_planes = c.take<uint32_t>(LAG_ROWS * 256);
            }
            if (filter_grid) {
                c.align(16);
                gw_planes = c.take<uint32_t>(LAG_ROWS * 256);
                gw_sums = c.take<uint32_t>(GRID_SUMS);
            }
            if (filter_byte) {
                c.align(16);
                bp_planes = c.take<uint32_t>(BYTE_ROWS * 256);
                bp_lag_sums = c.take<unsigned long long>(BYTE_LAGS);
                bp_sums = c.take<uint32_t>(BYTE_SUM_ROW);
            }
        }
    }

    hipError_t init()
    {
        const CtSettings &s = plan_container_settings(P.h);
        fmt = format_of(s);
        codec = s.codec;
        mode = s.mode;
        filter_auto = s.filter_auto;
        filter_lag = s.filter_lag;
        filter_grid = s.filter_grid;
        filter_byte = s.filter_byte;
        level = s.choose_filters;
        if (level) {                                          // the order-0 frames' settings: the level's, as an order-0 plan has them
            mode = CT_MODE_AUTO;
            filter_auto = level >= 2; filter_lag = level >= 3; filter_grid = level >= 4; filter_byte = level >= 5;
        }
        for (uint32_t i = 0; i < FILTER_CANDS; i++) {             // the candidate that is the plan's own filter
            const FilterCand c = filter_cand(i);
            if (c.elem == (fmt.elem ? fmt.elem : 1u) && (c.delta != 0) == fmt.delta()) own_pick = i;
        }
        if (mode == CT_MODE_RUNS) CT_HIP(carve_on(codec_scratch(P.h, 0), [&](Carver &c) { carve_runs(c); }));
        if (codec != CT_CODEC_BWT) CT_HIP(carve_on(codec_scratch(P.h, 0), [&](Carver &c) { carve_huff0(c); }));
        if (codec == CT_CODEC_CHOOSE) CT_HIP(plan_pinned_scratch(P.h, CT_PIN_STATS, 8 * (level >= 2 ? CLASS_HOST_WORDS : CHOOSE_STATS) * (size_t)P.rows, (void **)&h_stats));
        if (filter_auto) CT_HIP(plan_pinned_scratch(P.h, CT_PIN_COSTS, 8 * FP_HOST_WORDS, (void **)&h_costs));
        if (fmt.filtered() || filter_auto) {
            const int nstage = plan_pipelined(P.h) ? 2 : 1;
            for (int i = 0; i < nstage; i++) CT_HIP(plan_stage(P.h, i, (size_t)P.rows * P.n, &stage[i]));
            if (nstage == 1) stage[1] = stage[0];
        }
        CT_HIP(carve_on(codec_scratch(P.h, CT_DEV_ENC_TABLES), [&](Carver &c) { carve(c); }));   // (the plan's: nothing is freed here)
        return filter_auto ? hipMemsetAsync(fp_seg, 0, 8, P.st) : hipSuccess;
    }

    // filter-auto: the probe of the frame where it lies, its seven costs read back with one wait (as the CHOOSE codec reads its
    // stats), and the rule on the host.  A frame beyond the probe's 2^31 bytes is judged by its first 2^31.  With filter-lag the
    // lag probe's sums, winners, rows and costs are enqueued behind it -- the winners never leave the device between them -- and
    // the same wait brings ten costs and three lags; the walk is lag_rule.h's.  With filter-grid the grid probe follows in the same
    // way, and the walk is grid_rule.h's over thirteen costs; with filter-byte the byte probe follows, and the walk is byte_rule.h's
    // over fifteen.  *pick: the candidate (below BYTE_CANDS), *lag: its lag, *width: its row width, for a byte candidate its row
    // stride (0 but for a grid candidate and the strided byte candidate).
    static constexpr size_t FP_HOST_WORDS = BYTE_CANDS + 5;   // up to fifteen costs, then the three lags and the three widths in two 64-bit words each, the byte lag and stride in one
    size_t ncosts() const { return filter_byte ? BYTE_CANDS : filter_grid ? GRID_CANDS : LAG_CANDS; }
    CUDPPResult pick_filter(const uint8_t *d_in, unsigned long long frame_len, uint32_t *pick, uint32_t *lag, uint32_t *width)
    {
        const uint32_t max_len = (uint32_t)std::min<unsigned long long>(frame_len, GLC_FILTER_PROBE_MAX_LEN);
        CT_TRY(ct_put_u64(P.st, fp_seg + 1, frame_len));     // (fp_seg[0], the segment's offset, is 0 from init() on)
        CT_TRY(filter_probe_segments(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, fp_planes, fp_costs));
        *lag = 1;
        *width = 0;
        if (!filter_lag) {
            CT_TRY(hipMemcpyAsync(h_costs, fp_costs, 8 * FILTER_CANDS, hipMemcpyDeviceToHost, P.st));
            CT_TRY(hipStreamSynchronize(P.st));
            *pick = filter_pick(h_costs);
            return CUDPP_SUCCESS;
        }
        CT_TRY(lag_probe_sums(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, lp_sums, lp_lags));
        CT_TRY(lag_probe_planes(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, lp_lags, lp_planes, fp_costs + FILTER_CANDS));
        if (filter_grid) {
            CT_TRY(grid_probe_sums(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, gw_sums, gw_widths));
            CT_TRY(grid_probe_planes(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, gw_widths, gw_planes, fp_costs + LAG_CANDS));
        }
        if (filter_byte) {
            CT_TRY(byte_probe_sums(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, bp_lag_sums, bp_sums, bp_words));
            CT_TRY(byte_probe_planes(P.st, d_in, fp_seg, fp_seg + 1, 1, max_len, bp_words, bp_planes, fp_costs + GRID_CANDS));
        }
        CT_TRY(hipMemcpyAsync(h_costs, fp_costs, 8 * (ncosts() + 5), hipMemcpyDeviceToHost, P.st));
        CT_TRY(hipStreamSynchronize(P.st));
        const uint32_t *words = reinterpret_cast<const uint32_t *>(h_costs + ncosts());      // three lags, a pad, three widths, a pad, the byte lag and stride
        *pick = filter_byte ? byte_pick(h_costs) : filter_grid ? grid_pick(h_costs) : lag_pick(h_costs);
        if (*pick >= GRID_CANDS) {                            // (a strided candidate without a stride costs GRID_NO_COST: never picked)
            *lag = lag_clamp(words[8]);
            *width = *pick == GRID_CANDS ? 0u : byte_stride_word(words[9]);
        } else if (*pick >= LAG_CANDS) *width = grid_width_word(words[4 + *pick - LAG_CANDS]);      // (never 0: such a candidate costs GRID_NO_COST)
        else if (*pick >= FILTER_CANDS) *lag = lag_clamp(words[*pick - FILTER_CANDS]);
        return CUDPP_SUCCESS;
    }

    // one frame of nb blocks of blk_len from d_in, written at the device cursor into out (cap bytes).  With a filter the frame
    // goes through it as one segment into staging and its blocks are cut from there; the input's own bytes still make crc_all.
    // `by`: the codec that writes this frame (the plan's, or what the CHOOSE codec picked for its blocks).
    CUDPPResult frame(const uint8_t *d_in, uint32_t nb, uint32_t blk_len, uint8_t *out, unsigned long long cap, uint32_t by)
    {
        rep.choice[by == CT_CODEC_BWT ? 0 : 1] += nb;
        rep.choice[2]++;
        (void)plan_info(P.h, nullptr, nullptr, nullptr, &P.parity);
        const CtEncFrame &f = fr[P.parity];
        const uint8_t *orig = nullptr;
        CtFormat ff = fmt;                                    // the format whose filter this frame goes through
        uint32_t pick = own_pick;
        if (filter_auto && by == CT_CODEC_HUFF0) {             // (a BWT frame of the CHOOSE codec takes no filter: word 0)
            uint32_t lag = 1, width = 0;
            const CUDPPResult r = pick_filter(d_in, (unsigned long long)nb * blk_len, &pick, &lag, &width);
            if (r != CUDPP_SUCCESS) return r;
            const uint32_t lags[LAG_ELEMS] = {lag, lag, lag}, widths[LAG_ELEMS] = {width, width, width};
            const GridCand c = byte_cand(pick, lags, widths, lag, width);     // (below FILTER_CANDS: filter_rule.h's candidate, lag 1 and no fold)
            ff.elem = c.elem > 1 || pick >= GRID_CANDS ? c.elem : 0;      // (a byte candidate's frame has elem 1: version 15's format)
            ff.flags = c.delta ? CT_FLAG_DELTA | (c.fold ? CT_FLAG_FOLD : 0u) | (c.lag - 1u) << CT_LAG_SHIFT | (c.width ? CT_FLAG_GRID : 0u) : 0;
            ff.width = c.width;                               // (the frame's format: ct_frame_format()'s of the word written below)
        }
        if (pick < FILTER_CANDS) rep.filters[pick]++;         // (a frame that took a lag or grid candidate counts among all frames only)
        else if (pick < LAG_CANDS) { rep.lag_filters[pick - FILTER_CANDS]++; rep.lag_filters[LAG_ELEMS]++; }
        else if (pick < GRID_CANDS) { rep.grid_filters[pick - LAG_CANDS]++; rep.grid_filters[LAG_ELEMS]++; }
        else { rep.byte_filters[pick - GRID_CANDS]++; rep.byte_filters[BYTE_ROWS]++; }
        rep.filters[FILTER_CANDS]++;
        if (ff.filtered()) {
            plan_wait_released(P.h);                          // (the frame that staged here two calls ago is through)
            CT_TRY(filter_device(P.st, ff, d_in, stage[P.parity], (unsigned long long)nb * blk_len, false));
            orig = d_in;
            d_in = stage[P.parity];
        }
        if (mode == CT_MODE_RUNS) return frame_runs(f, d_in, orig, nb, blk_len, out, cap);
        if (by == CT_CODEC_HUFF0) {
            const Frame0 F{f, d_in, orig, nb, blk_len, out, cap, filter_auto ? ct_frame_word(ff) : 0u};
            return mode == CT_MODE_SPARSE ? frame_sparse(F) : mode == CT_MODE_ANS ? frame_ans(F) : mode == CT_MODE_AUTO ? frame_auto(F) :
                   mode == CT_MODE_DEDUP ? frame_dedup(F) : frame_plain(F);
        }
        const uint32_t nsub = (blk_len + HUFF_BLOCK - 1) / HUFF_BLOCK;
        ContainerHooks hk;
        hk.status = status;
        hk.pack_only = f.only;
        hk.before_offsets = [&](hipStream_t s2) { return ct_enc_kind(s2, f, nb, blk_len, state); };
        hk.after_pack = [&](hipStream_t s2) { return ct_enc_after_pack(s2, f, d_in, orig, nb, blk_len, out, cap, state); };
        return plan_compress_hooked(P.h, CompressCall{d_in, f.bwt, f.hist, f.enc_off, nsub, f.size, reinterpret_cast<uint32_t *>(out), 0,
                                                      blk_len, nb, f.boff, f.start, (size_t)(cap / 4)}, hk);
    }

    // The order-0 codec's frame in every mode, wholly on the plan's stream: the blocks as segments of the frame -> sizes(), the
    // mode's passes up to everything the kinds need -> kinds() (ct_enc_kind0 unless the mode brings its own) -> payload offsets ->
    // place(out as words, its capacity in words), the mode's records written behind the offsets -> the same stage behind the packer
    // as ever.  The five functions below are the modes: each says its parts and what they share.
    struct Frame0 {
        const CtEncFrame &f; const uint8_t *d_in, *orig; uint32_t nb, blk_len; uint8_t *out; unsigned long long cap;
        uint32_t word;                                        // the frame header's word 3: the frame's filter under version 10, else 0
    };
    template <class Sizes, class Kinds, class Place>
    CUDPPResult frame_order0(const Frame0 &F, Sizes sizes, Kinds kinds, Place place)
    {
        uint32_t *out_words = reinterpret_cast<uint32_t *>(F.out);
        const unsigned long long cap_words = F.cap / 4;
        plan_stage_mark(P.h, 0);
        CT_TRY(ct_block_offsets(P.st, h0.blk_off, h0.blk_len, F.nb, F.blk_len));
        CT_TRY(sizes());
        plan_stage_mark(P.h, 1);
        CT_TRY(kinds());
        CT_TRY(huff_block_offsets(P.st, F.f.size, F.nb, F.f.boff, F.f.start, (size_t)cap_words, status));
        CT_TRY(place(out_words, cap_words));
        plan_stage_mark(P.h, 2);
        CT_TRY(ct_enc_after_pack(P.st, F.f, F.d_in, F.orig, F.nb, F.blk_len, F.out, F.cap, state, F.word));
        plan_stage_mark(P.h, 3);
        return CUDPP_SUCCESS;
    }
    template <class Sizes, class Place>
    CUDPPResult frame_order0(const Frame0 &F, Sizes sizes, Place place)
    {
        return frame_order0(F, sizes, [&] { return ct_enc_kind0(P.st, mode, F.f, h0, sp, an, au, F.nb, F.blk_len, state); }, place);
    }

    // tables (and with them every record's size) -> kinds -> the batched encoder
    CUDPPResult frame_plain(const Frame0 &F)
    {
        KernelProf *prof = plan_prof(P.h);
        const CtEncFrame &f = F.f;
        const HdbSegs g{F.d_in, h0.blk_off, h0.blk_len, F.nb, F.blk_len};
        return frame_order0(
            F, [&] { return hdb_tables(P.st, g, true, f.hist, h0.lens, h0.codes, nullptr, h0.nun, nullptr, prof); },
            [&](uint32_t *out, unsigned long long cap) { return hdb_encode(P.st, g, h0.lens, h0.codes, h0.nun, out, f.boff, cap, f.only, h0.work, prof); });
    }

    // the sparse mode: tables of the whole blocks -> fill bytes -> masks -> kind 3 or 2 (histograms corrected) -> compaction of
    // the kind-3 blocks -> their tables, of K -> record sizes and the record rule -> payload offsets -> masks into the records
    // and every stream encoded behind its mask (kind 2 from the frame, kind 3 from the compaction space)
    CUDPPResult frame_sparse(const Frame0 &F)
    {
        KernelProf *prof = plan_prof(P.h);
        const CtEncFrame &f = F.f;
        const uint32_t nb = F.nb, blk_len = F.blk_len;
        const HdbSegs g2{nullptr, h0.in_off, h0.in_len, nb, blk_len};                      // (absolute addresses: frame blocks and K's)
        return frame_order0(
            F,
            [&]() -> hipError_t {
                const HdbSegs g{F.d_in, h0.blk_off, h0.blk_len, nb, blk_len};
                CT_HIP(hdb_tables(P.st, g, true, f.hist, h0.lens, h0.codes, nullptr, h0.nun, nullptr, prof));
                CT_HIP(ct_enc_sparse_fill(P.st, f.hist, nb, sp.fill));
                CT_HIP(ct_block_offsets(P.st, sp.kept_off, sp.klen, nb, sp.kept_stride));    // (klen itself comes two steps on)
                SpSegs s{const_cast<uint8_t *>(F.d_in), h0.blk_off, h0.blk_len, sp.kept, sp.kept_off, sp.fill, sp.mask, nullptr,
                         sp.mask_stride, nullptr, nb, blk_len};
                CT_HIP(sparse_mask(P.st, s));
                CT_HIP(ct_enc_sparse_decide(P.st, s, sp, f.hist, h0.in_off, h0.in_len));
                s.skip = sp.skip_move;
                CT_HIP(sparse_compact(P.st, s));
                return hdb_tables(P.st, g2, false, f.hist, h0.lens, h0.codes, nullptr, h0.nun, sp.skip_table, prof);
            },
            [&](uint32_t *out, unsigned long long cap) -> hipError_t {
                CT_HIP(ct_enc_sparse_place(P.st, f, sp, nb, blk_len, out, cap));
                return hdb_encode(P.st, g2, h0.lens, h0.codes, h0.nun, out, sp.unit_off, cap, f.only, h0.work, prof);
            });
    }

    // the rANS mode: histograms (the Huffman tables that come with them are not used) -> the blocks' rANS tables -> every chunk
    // coded into its scratch slot -> record sizes and the record rule -> payload offsets -> counts, states and units into the
    // records
    CUDPPResult frame_ans(const Frame0 &F)
    {
        KernelProf *prof = plan_prof(P.h);
        const CtEncFrame &f = F.f;
        AnsSegs a{const_cast<uint8_t *>(F.d_in), h0.blk_off, h0.blk_len, f.hist, an.tab, nullptr, F.nb, F.blk_len};
        return frame_order0(
            F,
            [&]() -> hipError_t {
                const HdbSegs g{F.d_in, h0.blk_off, h0.blk_len, F.nb, F.blk_len};
                CT_HIP(hdb_tables(P.st, g, true, f.hist, h0.lens, h0.codes, nullptr, h0.nun, nullptr, prof));
                CT_HIP(ans_tables(P.st, a));
                return ans_encode(P.st, a, an.sc);
            },
            [&](uint32_t *out, unsigned long long cap) {
                a.skip = an.skip_ans;
                return ans_place(P.st, a, an.sc, out, f.boff, cap);
            });
    }

    // the auto mode: one probe of the blocks (counts and uniform chunks) -> fill bytes and the blocks' rANS tables (their q) ->
    // candidate S of every block and the estimate wA, from the statistics alone -> the Huffman tables of candidate S's counts,
    // and with them wS -> the choice per block -> masks and compaction of the blocks that stay kind 3, the rANS coder on the
    // blocks chosen as kind 5 -> actual sizes and the record rule -> payload offsets -> masks and rANS records placed, kind 2 and
    // K encoded behind them
    CUDPPResult frame_auto(const Frame0 &F)
    {
        KernelProf *prof = plan_prof(P.h);
        const CtEncFrame &f = F.f;
        const uint32_t nb = F.nb, blk_len = F.blk_len;
        const HdbSegs g2{nullptr, h0.in_off, h0.in_len, nb, blk_len};                      // (absolute addresses: frame blocks and K's)
        AnsSegs a{const_cast<uint8_t *>(F.d_in), h0.blk_off, h0.blk_len, f.hist, an.tab, nullptr, nb, blk_len};
        return frame_order0(
            F,
            [&]() -> hipError_t {
                CT_HIP(ct_block_offsets(P.st, sp.kept_off, sp.klen, nb, sp.kept_stride));    // (klen itself comes two steps on)
                CT_HIP(probe_segments(P.st, F.d_in, h0.blk_off, h0.blk_len, nb, blk_len, f.hist, au.uniform));
                CT_HIP(ct_enc_sparse_fill(P.st, f.hist, nb, sp.fill));
                CT_HIP(ans_tables(P.st, a));
                SpSegs s{const_cast<uint8_t *>(F.d_in), h0.blk_off, h0.blk_len, sp.kept, sp.kept_off, sp.fill, sp.mask, nullptr,
                         sp.mask_stride, nullptr, nb, blk_len};
                CT_HIP(ct_enc_auto_candidates(P.st, s, sp, au, f.hist, an.tab, h0.in_off, h0.in_len));
                CT_HIP(hdb_tables(P.st, g2, false, au.hist_s, h0.lens, h0.codes, nullptr, h0.nun, sp.skip_table, prof));
                CT_HIP(ct_enc_auto_choose(P.st, f, h0, sp, an, au, nb, blk_len));
                s.skip = sp.skip_move;
                CT_HIP(sparse_mask(P.st, s));
                CT_HIP(sparse_compact(P.st, s));
                a.skip = an.skip_ans;                         // (1 = not rANS-coded; behind the kinds: no kind-5 record to place)
                return ans_encode(P.st, a, an.sc);
            },
            [&](uint32_t *out, unsigned long long cap) -> hipError_t {
                CT_HIP(ct_enc_sparse_place(P.st, f, sp, nb, blk_len, out, cap));
                CT_HIP(ans_place(P.st, a, an.sc, out, f.boff, cap));
                return hdb_encode(P.st, g2, h0.lens, h0.codes, h0.nun, out, sp.unit_off, cap, f.only, h0.work, prof);
            });
    }

    // the dedup mode, wholly on the plan's stream: the map of the frame's chunks (hash, insert, verify) -> per block the mask, the
    // refs, the lowest source block and kind 6 or 2 -> compaction of the kind-6 blocks (the sparse mode's mover under the mask
    // widened to 64-byte chunks) -> counts and tables, of K or of the whole block -> record sizes and the record rule -> payload
    // offsets -> masks and refs into the records and every stream encoded behind them.  Its kinds kernel is its own: the one
    // mode that hands frame_order0 that part as well.
    CUDPPResult frame_dedup(const Frame0 &F)
    {
        KernelProf *prof = plan_prof(P.h);
        const CtEncFrame &f = F.f;
        const uint32_t nb = F.nb, blk_len = F.blk_len;
        const HdbSegs g2{nullptr, h0.in_off, h0.in_len, nb, blk_len};                      // (absolute addresses: frame blocks and K's)
        DdSegs m{const_cast<uint8_t *>(F.d_in), h0.blk_off, h0.blk_len, dd.hash, dd.table, dd.slots, dd.src, nb, blk_len, dd.nch};
        m.nch = (blk_len + DD_CHUNK - 1) / DD_CHUNK;                                       // (the frame's: the tail frame's blocks are shorter)
        m.slots = (uint32_t)dedup_slots((size_t)nb * m.nch);
        CtEncDedup d = dd;
        d.nch = m.nch;
        return frame_order0(
            F,
            [&]() -> hipError_t {
                CT_HIP(ct_block_offsets(P.st, sp.kept_off, sp.klen, nb, sp.kept_stride));    // (klen itself comes two steps on)
                CT_HIP(dedup_map(P.st, m));
                CT_HIP(ct_enc_dedup_decide(P.st, d, sp, h0.blk_off, F.d_in, nb, blk_len, f.hist, h0.in_off, h0.in_len));
                const SpSegs s{const_cast<uint8_t *>(F.d_in), h0.blk_off, h0.blk_len, sp.kept, sp.kept_off, sp.fill, sp.mask, nullptr,
                               sp.mask_stride, sp.skip_move, nb, blk_len};
                CT_HIP(sparse_compact(P.st, s));
                return hdb_tables(P.st, g2, true, f.hist, h0.lens, h0.codes, nullptr, h0.nun, sp.skip_table, prof);
            },
            [&] { return ct_enc_dedup_kind(P.st, f, h0, sp, d, nb, blk_len, state); },
            [&](uint32_t *out, unsigned long long cap) -> hipError_t {
                CT_HIP(ct_enc_dedup_place(P.st, f, sp, d, nb, blk_len, out, cap));
                return hdb_encode(P.st, g2, h0.lens, h0.codes, h0.nun, out, sp.unit_off, cap, f.only, h0.work, prof);
            });
    }

    // the BWT codec's frame with the runs mode on, wholly on the plan's stream: BWT and MTF of the blocks by the plan's sorter
    // and MTF stage -> the split into A and B -> tables of the A's (their counts are the record's hist) and of the B's -> nz,
    // record sizes and the record rule -> payload offsets -> nz and the pairs into the records -> every stream encoded at its
    // place, A's and B's in one launch -> the same stage behind the packer as ever
    CUDPPResult frame_runs(const CtEncFrame &f, const uint8_t *d_in, const uint8_t *orig, uint32_t nb, uint32_t blk_len,
                           uint8_t *out, unsigned long long cap)
    {
        KernelProf *prof = plan_prof(P.h);
        plan_stage_mark(P.h, 0);
        const uint8_t *mtf = nullptr;
        size_t mtf_stride = 0;
        CT_TRY(plan_bwt_mtf(P.h, d_in, blk_len, nb, f.bwt, &mtf, &mtf_stride));
        plan_stage_mark(P.h, 1);
        CT_TRY(ct_enc_runs_segs(P.st, zr, mtf, mtf_stride, nb, blk_len));
        const ZrSegs z{nullptr, zr.x_off, zr.x_len, nullptr, zr.seg_off, zr.seg_len, nullptr, zr.seg_off + nb, zr.seg_len + nb, nullptr,
                       nb, blk_len};
        CT_TRY(zrun_split(P.st, z));
        CT_TRY(ct_enc_runs_empty(P.st, zr, nb));
        const HdbSegs ga{nullptr, zr.seg_off, zr.seg_len, nb, blk_len}, gb{nullptr, zr.seg_off + nb, zr.seg_len + nb, nb, blk_len};
        CT_TRY(hdb_tables(P.st, ga, true, f.hist, zr.lens, zr.codes, nullptr, zr.nun, nullptr, prof));
        CT_TRY(hdb_tables(P.st, gb, true, zr.hist_b, zr.lens + 256ull * nb, zr.codes + 256ull * nb, nullptr, zr.nun + nb, zr.skip_b, prof));
        CT_TRY(ct_enc_runs_kind(P.st, f, zr, nb, blk_len, state));
        CT_TRY(huff_block_offsets(P.st, f.size, nb, f.boff, f.start, (size_t)(cap / 4), status));
        CT_TRY(ct_enc_runs_place(P.st, f, zr, nb, reinterpret_cast<uint32_t *>(out), cap / 4));
        const HdbSegs gab{nullptr, zr.seg_off, zr.seg_len, 2 * nb, blk_len};
        CT_TRY(hdb_encode(P.st, gab, zr.lens, zr.codes, zr.nun, reinterpret_cast<uint32_t *>(out), zr.unit_off, cap / 4, zr.skip_enc, zr.work, prof));
        plan_stage_mark(P.h, 2);
        CT_TRY(ct_enc_after_pack(P.st, f, d_in, orig, nb, blk_len, out, cap, state));
        plan_stage_mark(P.h, 3);
        return CUDPP_SUCCESS;
    }

    // The CHOOSE codec's super-frame (what is one frame with the other codecs): the bigram probe of its blocks, their stats rows
    // read back in one copy and one wait, the rule on the host (choose_rule.h), and one frame per maximal run of blocks of one
    // choice, each by that codec's own path at the device cursor.  An order-0 frame is wholly on the plan's stream, so it waits
    // for what a pipelined BWT frame in front of it still has on the side stream (the cursor and the running CRC chain there).
    CUDPPResult super_frame(const uint8_t *d_in, uint32_t nb, uint32_t blk_len, uint8_t *out, unsigned long long cap)
    {
        CT_TRY(ct_block_offsets(P.st, h0.blk_off, h0.blk_len, nb, blk_len));
        CT_TRY(bigram_probe_segments(P.st, d_in, h0.blk_off, h0.blk_len, nb, blk_len, ch_stats));
        // choose-filters from level 2 on: the filter probe with the blocks as its segments, at level 5 the byte probe's lag sums and
        // its rows at {best lag, stride 0} -- no stride, lag or width search per block: those are the frame's
        const size_t R = P.rows;
        if (level >= 2 && blk_len >= CHOOSE_MIN_LEN) {
            CT_TRY(filter_probe_segments(P.st, d_in, h0.blk_off, h0.blk_len, nb, blk_len, cf_planes, cf_costs));
            if (level >= 5) {
                CT_TRY(byte_probe_lags(P.st, d_in, h0.blk_off, h0.blk_len, nb, blk_len, cb_lag_sums, cb_words));
                CT_TRY(byte_probe_planes(P.st, d_in, h0.blk_off, h0.blk_len, nb, blk_len, cb_words, cb_planes, cb_costs));
            }
            CT_TRY(hipMemcpyAsync(h_stats, ch_stats, 8 * CLASS_HOST_WORDS * R, hipMemcpyDeviceToHost, P.st));
        } else
            CT_TRY(hipMemcpyAsync(h_stats, ch_stats, 8 * CHOOSE_STATS * (size_t)nb, hipMemcpyDeviceToHost, P.st));
        CT_TRY(hipStreamSynchronize(P.st));
        // the key of a block (class_rule.h): CLASS_BWT, or the order-0 codec with the block's element size
        auto by = [&](uint32_t b) {
            unsigned long long cost[CLASS_COSTS] = {};
            const bool probed = level >= 2 && blk_len >= CHOOSE_MIN_LEN;
            if (probed) {
                memcpy(cost, h_stats + CHOOSE_STATS * R + FILTER_CANDS * (size_t)b, 8 * FILTER_CANDS);
                cost[FILTER_CANDS] = level >= 5 ? h_stats[(CHOOSE_STATS + FILTER_CANDS) * R + BYTE_ROWS * (size_t)b] : GRID_NO_COST;
            }
            return class_key(probed ? level : 0u, blk_len, cost, h_stats + CHOOSE_STATS * (size_t)b);
        };
        for (uint32_t a = 0; a < nb;) {
            const uint32_t key = by(a), c = key == CLASS_BWT ? CT_CODEC_BWT : CT_CODEC_HUFF0;
            uint32_t b = a + 1;
            while (b < nb && by(b) == key) b++;
            if (c == CT_CODEC_HUFF0) plan_join(P.h);
            const CUDPPResult r = frame(d_in + (size_t)a * blk_len, b - a, blk_len, out, cap, c);
            if (r != CUDPP_SUCCESS) return r;
            a = b;
        }
        return CUDPP_SUCCESS;
    }

    // the call is through: what glcContainerLastChoice and glcContainerLastFilters report is this call's from here on
    CUDPPResult succeeded()
    {
        CtReports &r = plan_container_reports(P.h);
        memcpy(r.choice, rep.choice, sizeof r.choice);
        memcpy(r.filters, rep.filters, sizeof r.filters);
        memcpy(r.lag_filters, rep.lag_filters, sizeof r.lag_filters);
        memcpy(r.grid_filters, rep.grid_filters, sizeof r.grid_filters);
        memcpy(r.byte_filters, rep.byte_filters, sizeof r.byte_filters);
        set_error(P.h, CT_OK);
        return CUDPP_SUCCESS;
    }

    // every frame of [d_in, + len) with the plan's n and rows
    CUDPPResult frames(const uint8_t *d_in, unsigned long long len, uint8_t *out, unsigned long long cap)
    {
        unsigned long long pos = 0;
        while (pos < len) {
            const unsigned long long left = len - pos;
            const uint32_t nb = left >= P.n ? (uint32_t)std::min<unsigned long long>(P.rows, left / P.n) : 1u;
            const uint32_t bl = left >= P.n ? P.n : (uint32_t)left;
            const CUDPPResult r = codec == CT_CODEC_CHOOSE ? super_frame(d_in + pos, nb, bl, out, cap) : frame(d_in + pos, nb, bl, out, cap, codec);
            if (r != CUDPP_SUCCESS) return r;
            pos += (unsigned long long)nb * bl;
        }
        return CUDPP_SUCCESS;
    }
};

// -------------------------------------------------------------------------------------------------------------------------
// decoder
// -------------------------------------------------------------------------------------------------------------------------
// body(a, count) -> CUDPPResult over the maximal runs [a, a + count) of the blocks 0 .. nb: in(a, a) = a run may start at block a,
// in(a, b) = block b may join the run that starts at a.  Stops at the first body that fails.
template <class In, class Body>
CUDPPResult for_runs(uint32_t nb, In in, Body body)
{
    for (uint32_t a = 0; a < nb;) {
        if (!in(a, a)) { a++; continue; }
        uint32_t b = a + 1;
        while (b < nb && in(a, b)) b++;
        const CUDPPResult r = body(a, b - a);
        if (r != CUDPP_SUCCESS) return r;
        a = b;
    }
    return CUDPP_SUCCESS;
}

struct Decoder {
    Plan P;
    void *mem = nullptr;
    size_t cap_nb = 0;
    CtDecFrame f = {};
    CtDecState *state = nullptr;
    unsigned long long *h_verdict = nullptr;                  // pinned
    CtFormat fmt;                                             // the stream header's
    CtDecHuff0 h0 = {};
    CtDecDedup dd = {};                                       // a version-9 frame's map and widened masks, behind h0's

    // the scratch of a frame that may hold kind 2, kept with the plan: tables for nb blocks, span-function prefixes for `chunk`
    // of them at a time (at most the plan's rows, and at most 256 MiB of prefixes)
    void carve_huff0(Carver &c, uint32_t nb, uint32_t blk_len)
    {
        const size_t n4 = ((size_t)nb + 63) & ~(size_t)63;
        h0.nun = c.take<unsigned long long>(n4);
        h0.skip = c.take<uint32_t>(n4);
        h0.lut = c.take<uint16_t>(2048 * (size_t)nb);
        c.align(256);
        h0.work = c.take<uint8_t>(hdb_decode_work_bytes(h0.chunk, blk_len));
        h0.kinds = fmt.kinds();
        if (fmt.kind5_legal()) {
            c.align(256);
            h0.ans_tab = c.take<uint8_t>((size_t)h0.chunk * ANS_TAB_BYTES);
        }
        if (!fmt.kind3_legal() && !fmt.kind4_legal() && !fmt.kind6_legal()) return;
        h0.k_off = c.take<unsigned long long>(n4);
        h0.k_len = c.take<unsigned long long>(n4);
        h0.u_off = c.take<unsigned long long>(n4);
        h0.skip3 = c.take<uint32_t>(n4);
        c.align(256);
        h0.kept_stride = (blk_len + 15u) & ~15u;
        h0.kept = c.take<uint8_t>((size_t)h0.chunk * h0.kept_stride);
        if (fmt.kind6_legal()) {
            dd.chunk = h0.chunk;
            dd.stride64 = sp_mask_words(blk_len);
            dd.src = c.take<uint32_t>((size_t)nb * ((blk_len + DD_CHUNK - 1) / DD_CHUNK));
            dd.mask64 = c.take<uint32_t>((size_t)h0.chunk * dd.stride64);
        }
        if (!fmt.kind4_legal()) return;
        h0.kept_b = c.take<uint8_t>((size_t)h0.chunk * h0.kept_stride);
        h0.b_off = c.take<unsigned long long>(n4);
        h0.b_len = c.take<unsigned long long>(n4);
        h0.ub_off = c.take<unsigned long long>(n4);
        h0.nun_b = c.take<unsigned long long>(n4);
        h0.m_off = c.take<unsigned long long>(n4);
        h0.m_len = c.take<unsigned long long>(n4);
        h0.skip_b = c.take<uint32_t>(n4);
        h0.skip_tb = c.take<uint32_t>(n4);
        h0.hist_b = c.take<uint32_t>(256 * (size_t)nb);
        h0.lut_b = c.take<uint16_t>(2048 * (size_t)nb);
    }
    hipError_t reserve_huff0(uint32_t nb, uint32_t blk_len)
    {
        const size_t per = hdb_decode_work_bytes(1, blk_len) + 512;
        h0.chunk = (uint32_t)std::min<size_t>(std::min<size_t>(P.rows, nb), std::max<size_t>(1, ((size_t)256 << 20) / per));
        if (fmt.kind4_legal()) CT_HIP(plan_decode_rows(P.h, &h0.mtf, &h0.mtf_stride));   // (where the join leaves the MTF bytes)
        return carve_on(codec_scratch(P.h, 1), [&](Carver &c) { carve_huff0(c, nb, blk_len); });
    }

    static size_t verdict_words(uint32_t nb) { return 2 + ((size_t)nb + 1) / 2; }
    void carve(Carver &c, uint32_t nb)
    {
        const size_t n2 = (size_t)nb + 2;
        f.seg_off = c.take<unsigned long long>(n2);
        f.seg_len = c.take<unsigned long long>(n2);
        f.verdict = c.take<unsigned long long>(verdict_words(nb));
        f.crc = c.take<uint32_t>(n2);
    }
    hipError_t reserve(uint32_t nb)
    {
        if (nb <= cap_nb && mem) return hipSuccess;
        // the plan's tables and pinned words (a larger frame in the same call: the plan waits for its stream before it lets the
        // old ones go)
        CT_HIP(carve_on(
            [&](size_t bytes, void **base) {
                hipError_t e = plan_codec_scratch(P.h, CT_DEV_DEC_TABLES, bytes, reinterpret_cast<uint8_t **>(&mem));
                if (e != hipSuccess) { mem = nullptr; return e; }
                e = plan_pinned_scratch(P.h, CT_PIN_VERDICT, 8 * verdict_words(nb), (void **)&h_verdict);
                if (e != hipSuccess) h_verdict = nullptr;
                *base = mem;
                return e;
            },
            [&](Carver &c) { carve(c, nb); }));
        cap_nb = nb;
        return hipSuccess;
    }
    hipError_t begin()
    {
        hipError_t e = plan_codec_scratch(P.h, CT_DEV_DEC_STATE, sizeof(CtDecState), reinterpret_cast<uint8_t **>(&state));
        if (e != hipSuccess) { state = nullptr; return e; }
        e = hipMemsetAsync(state, 0, sizeof(CtDecState), P.st);
        if (e == hipSuccess) e = hipMemsetAsync(&state->err, 0xFF, 8, P.st);
        return e;
    }

    // a frame in device memory whose header (nb, blk_len, payload words) the host has range-checked; decoded to out.  A
    // filtered frame is decoded into the plan's staging, checked block by block there and inverted into out in one launch.
    // With a subset (a range read: need[b] != 0 = block b is wanted) the frame gets every check of its tables and records as
    // ever, but only the wanted blocks are decoded, into the plan's staging at their own places whatever the format, and
    // checked there; *staged is the staging and final_out is not touched (the inverse filter of a range is the caller's).
    // In a version-9 frame a wanted kind-6 block b needs the blocks [bwt_index[b], b) as sources (dedup_rule.h): they are decoded
    // and joined as well, but neither filled nor compared with their crc_raw; *decoded counts them with the wanted ones.
    // word: the frame header's word 3, which under version 10 names the frame's filter (ct_frame_format)
    CUDPPResult frame(const uint8_t *fr, uint32_t nb, uint32_t blk_len, unsigned long long pw, uint32_t word, uint8_t *final_out, uint32_t fi,
                      const uint8_t *need = nullptr, uint8_t **staged = nullptr, unsigned long long *decoded = nullptr)
    {
        CT_TRY(reserve(nb));
        const CtFormat ff = ct_frame_format(fmt, word);
        uint8_t *out = final_out;
        if (ff.filtered() || need) CT_TRY(plan_stage(P.h, 0, (size_t)nb * blk_len, &out));
        if (staged) *staged = out;
        std::vector<uint8_t> need9;                               // version 9: need[] with the source-only blocks marked 2
        auto want = [&](uint32_t b) { return !need || need[b] != 0; };
        auto checked = [&](uint32_t b) { return !need || need[b] == DEDUP_NEEDED; };
        // what for_runs() walks: the runs of wanted blocks (all of them: one run), and of the blocks that are checked
        auto wanted = [&](uint32_t, uint32_t b) { return want(b); };
        auto to_check = [&](uint32_t, uint32_t b) { return checked(b); };
        const bool k2 = fmt.kind2_legal();
        KernelProf *prof = plan_prof(P.h);
        if (k2) CT_TRY(reserve_huff0(nb, blk_len));
        CT_TRY(ct_dec_verify(P.st, f, fr, nb, blk_len, pw, k2 ? &h0 : nullptr, prof));
        CT_TRY(hipMemcpyAsync(h_verdict, f.verdict, 8 * verdict_words(nb), hipMemcpyDeviceToHost, P.st));
        CT_TRY(hipStreamSynchronize(P.st));
        if (h_verdict[0]) return fail(P.h, CT_FRAME_TABLE, fi);
        if (h_verdict[1] != ~0ull) return fail(P.h, h_verdict[1] >> 32, fi, h_verdict[1] & 0xFFFFFFFFu);
        const uint32_t *kind = reinterpret_cast<const uint32_t *>(h_verdict + 2);
        if (need && fmt.kind6_legal()) {
            const CtTables T9 = ct_tables(nb, blk_len);
            std::vector<uint32_t> idx(nb);
            CT_TRY(hipMemcpyAsync(idx.data(), fr + CT_FRAME_HDR + 4 * T9.bwt, 4ull * nb, hipMemcpyDeviceToHost, P.st));
            CT_TRY(hipStreamSynchronize(P.st));
            need9.assign(need, need + nb);
            (void)dedup_mark_sources(kind, idx.data(), nb, need9.data());   // (every run of needed blocks asks for its sources)
            need = need9.data();
        }
        if (decoded) for (uint32_t b = 0; b < nb; b++) *decoded += want(b) ? 1 : 0;
        CUDPPResult r = for_runs(nb, wanted, [&](uint32_t a, uint32_t cnt) { return hip_result(ct_dec_raw(P.st, f, fr, nb, blk_len, out, a, cnt)); });
        if (r != CUDPP_SUCCESS) return r;
        const CtTables T = ct_tables(nb, blk_len);
        const uint32_t *W = reinterpret_cast<const uint32_t *>(fr + CT_FRAME_HDR);
        const unsigned int *pay = reinterpret_cast<const unsigned int *>(fr + CT_FRAME_HDR + 4 * T.words);
        // the maximal runs [a, b) of wanted blocks of kind K: more(a, b) = block b may still join the run that starts at a
        auto of_kind = [&](uint32_t K, auto more) {
            return [&want, kind, K, more](uint32_t a, uint32_t b) { return kind[b] == K && want(b) && more(a, b); };
        };
        auto in_rows = [&](uint32_t a, uint32_t b) { return b - a < P.rows; };
        auto in_chunk = [&](uint32_t a, uint32_t b) { return b - a < h0.chunk; };        // a chunk of the plan's rows at a time
        auto same_chunk = [&](uint32_t a, uint32_t b) { return b / h0.chunk == a / h0.chunk; };
        const unsigned long long *pay_off = reinterpret_cast<const unsigned long long *>(W + T.pay_off);
        r = for_runs(nb, of_kind(CT_KIND_HUFF, in_rows), [&](uint32_t a, uint32_t cnt) {
            return glcDecompressBatchCompact(P.h, reinterpret_cast<const int *>(W + T.bwt) + a, W + T.hist + 256ull * a,
                                             W + T.enc_off + (size_t)T.nsub * a, T.nsub, pay, pw, pay_off + a, out + (size_t)a * blk_len,
                                             blk_len, cnt);
        });
        if (r != CUDPP_SUCCESS) return r;
        if (k2) r = for_runs(nb, of_kind(CT_KIND_HUFF0, in_chunk), [&](uint32_t a, uint32_t cnt) -> CUDPPResult {
            // (k_cd_raw has put every block's output range into f.seg_*: absolute addresses, so the base is null)
            const HdbOut g{nullptr, f.seg_off + a, f.seg_len + a, cnt, blk_len};
            CT_TRY(hdb_decode(P.st, pay, pay_off + a, h0.nun + a, h0.lut + 2048ull * a, g, nullptr, h0.work, prof));
            return CUDPP_SUCCESS;
        });
        if (r != CUDPP_SUCCESS) return r;
        // sparse blocks: K decoded into scratch, then expanded
        if (fmt.kind3_legal()) r = for_runs(nb, of_kind(CT_KIND_SPARSE, in_chunk), [&](uint32_t a, uint32_t cnt) -> CUDPPResult {
            const HdbOut g{nullptr, h0.k_off + a, h0.k_len + a, cnt, blk_len};
            CT_TRY(hdb_decode(P.st, pay, h0.u_off + a, h0.nun + a, h0.lut + 2048ull * a, g, h0.skip3 + a, h0.work, prof));
            const SpSegs s{nullptr, f.seg_off + a, f.seg_len + a, nullptr, h0.k_off + a, W + T.bwt + a, const_cast<uint32_t *>(pay),
                           pay_off + a, 0, nullptr, cnt, blk_len};
            CT_TRY(sparse_join(P.st, s));
            return CUDPP_SUCCESS;
        });
        if (r != CUDPP_SUCCESS) return r;
        // rANS blocks: their tables from the histograms, then one pass
        if (fmt.kind5_legal()) r = for_runs(nb, of_kind(CT_KIND_ANS, in_chunk), [&](uint32_t a, uint32_t cnt) -> CUDPPResult {
            const AnsSegs g{nullptr, f.seg_off + a, f.seg_len + a, W + T.hist + 256ull * a, h0.ans_tab, nullptr, cnt, blk_len};
            CT_TRY(ans_tables(P.st, g));
            CT_TRY(ans_decode(P.st, g, pay, pay_off + a, nullptr));
            return CUDPP_SUCCESS;
        });
        if (r != CUDPP_SUCCESS) return r;
        // zero-run blocks inside one chunk of the decoder: A and B decoded into scratch, joined into the rows b % chunk of the
        // decoder's MTF bytes, and from there the BWT codec's own inverse MTF and inverse BWT
        if (fmt.kind4_legal()) r = for_runs(nb, of_kind(CT_KIND_RUNS, same_chunk), [&](uint32_t a, uint32_t cnt) -> CUDPPResult {
            const HdbOut ga{nullptr, h0.k_off + a, h0.k_len + a, cnt, blk_len}, gb{nullptr, h0.b_off + a, h0.b_len + a, cnt, blk_len};
            CT_TRY(hdb_decode(P.st, pay, h0.u_off + a, h0.nun + a, h0.lut + 2048ull * a, ga, h0.skip3 + a, h0.work, prof));
            CT_TRY(hdb_decode(P.st, pay, h0.ub_off + a, h0.nun_b + a, h0.lut_b + 2048ull * a, gb, h0.skip_b + a, h0.work, prof));
            const ZrSegs z{nullptr, h0.m_off + a, h0.m_len + a, nullptr, h0.k_off + a, h0.k_len + a, nullptr, h0.b_off + a, h0.b_len + a,
                           nullptr, cnt, blk_len};
            CT_TRY(zrun_join(P.st, z));
            CT_TRY(plan_decode_from_mtf(P.h, a % h0.chunk, reinterpret_cast<const int *>(W + T.bwt) + a, out + (size_t)a * blk_len, blk_len, cnt));
            return CUDPP_SUCCESS;
        });
        if (r != CUDPP_SUCCESS) return r;
        // dedup blocks inside one chunk of the decoder: K decoded into scratch and put back under the mask (widened to 64-byte
        // chunks for the sparse mode's join, which leaves its fill byte in the elided chunks until the fill pass)
        if (fmt.kind6_legal()) {
            r = for_runs(nb, wanted, [&](uint32_t a, uint32_t cnt) { return hip_result(ct_dec_dedup_expand(P.st, fr, nb, blk_len, a, cnt, dd, false)); });
            if (r != CUDPP_SUCCESS) return r;
            r = for_runs(nb, of_kind(CT_KIND_DEDUP, same_chunk), [&](uint32_t a, uint32_t cnt) -> CUDPPResult {
                const HdbOut g{nullptr, h0.k_off + a, h0.k_len + a, cnt, blk_len};
                CT_TRY(hdb_decode(P.st, pay, h0.u_off + a, h0.nun + a, h0.lut + 2048ull * a, g, h0.skip3 + a, h0.work, prof));
                CT_TRY(ct_dec_dedup_expand(P.st, fr, nb, blk_len, a, cnt, dd, true));
                const SpSegs s{nullptr, f.seg_off + a, f.seg_len + a, nullptr, h0.k_off + a, W + T.bwt + a,
                               dd.mask64 + (size_t)(a % dd.chunk) * dd.stride64, nullptr, dd.stride64, nullptr, cnt, blk_len};
                CT_TRY(sparse_join(P.st, s));
                return CUDPP_SUCCESS;
            });
            if (r != CUDPP_SUCCESS) return r;
        }
        plan_join(P.h);
        // the fill: behind every join of the frame, in front of the decoded-CRC pass; sources are kept chunks, so one pass completes
        // the frame.  Only the blocks that are checked are filled.
        if (fmt.kind6_legal()) {
            const DdSegs g{nullptr, f.seg_off, f.seg_len, nullptr, nullptr, 0, dd.src, nb, blk_len, (blk_len + DD_CHUNK - 1) / DD_CHUNK};
            r = for_runs(nb, to_check, [&](uint32_t a, uint32_t cnt) { return hip_result(dedup_fill(P.st, g, a, cnt)); });
            if (r != CUDPP_SUCCESS) return r;
        }
        if (need)
            return for_runs(nb, to_check, [&](uint32_t a, uint32_t cnt) {
                return hip_result(ct_dec_check(P.st, f, fr, nb, blk_len, out, fi, state, false, a, cnt));
            });
        CT_TRY(ct_dec_check(P.st, f, fr, nb, blk_len, out, fi, state, !ff.filtered()));
        if (ff.filtered()) {
            CT_TRY(filter_device(P.st, ff, out, final_out, (unsigned long long)nb * blk_len, true));
            CT_TRY(ct_dec_fold(P.st, f, final_out, nb, blk_len, state));
        }
        return CUDPP_SUCCESS;
    }

    // after the last frame: the decoded-bytes verdict and the whole output's CRC against the trailer's (a range read has no
    // whole output: it stops at the blocks' verdict)
    CUDPPResult end(uint32_t trailer_crc, bool whole = true)
    {
        CtDecState s;
        CT_TRY(hipMemcpyAsync(&s, state, sizeof(s), hipMemcpyDeviceToHost, P.st));
        CT_TRY(hipStreamSynchronize(P.st));
        if (s.err != ~0ull) return fail(P.h, CT_DECODED_CRC, (s.err - 1) >> 32, (s.err - 1) & 0xFFFFFFFFu);
        if (whole && s.crc_all != trailer_crc) return fail(P.h, CT_DECODED_CRC);
        return CUDPP_SUCCESS;
    }
};

// -------------------------------------------------------------------------------------------------------------------------
// streamed forms: a source of input bytes and a sink of output bytes (host buffers or files), one frame at a time
// -------------------------------------------------------------------------------------------------------------------------
struct Source {
    virtual ~Source() {}
    virtual bool read(void *dst, size_t n) = 0;                  // exactly n bytes or false
};
struct Sink {
    virtual ~Sink() {}
    virtual bool write(const void *src, size_t n) = 0;           // false: no room (capacity) or an I/O error
};
struct MemSource : Source {
    const uint8_t *p; unsigned long long left;
    MemSource(const void *q, unsigned long long n) : p(static_cast<const uint8_t *>(q)), left(n) {}
    bool read(void *dst, size_t n) override { if (n > left) return false; memcpy(dst, p, n); p += n; left -= n; return true; }
};
struct MemSink : Sink {
    uint8_t *p; unsigned long long cap, used = 0;
    MemSink(void *q, unsigned long long c) : p(static_cast<uint8_t *>(q)), cap(c) {}
    bool write(const void *src, size_t n) override { if (n > cap - used) return false; memcpy(p + used, src, n); used += n; return true; }
};
struct FileSource : Source {
    FILE *f;
    explicit FileSource(FILE *g) : f(g) {}
    bool read(void *dst, size_t n) override { return fread(dst, 1, n, f) == n; }
};
struct FileSink : Sink {
    FILE *f;
    explicit FileSink(FILE *g) : f(g) {}
    bool write(const void *src, size_t n) override { return fwrite(src, 1, n, f) == n; }
};

// staging of the host-pointer and file forms: views of the plan's grow-only slots (nothing is freed by a call)
struct Pinned {
    CUDPPHandle plan; uint32_t slot;
    void *p = nullptr; size_t n = 0;
    Pinned(CUDPPHandle h, uint32_t s) : plan(h), slot(s) {}
    hipError_t reserve(size_t m)
    {
        if (m <= n) return hipSuccess;
        const hipError_t e = plan_pinned_scratch(plan, slot, m, &p);
        if (e == hipSuccess) n = m; else { p = nullptr; n = 0; }
        return e;
    }
};
struct DevBuf {
    CUDPPHandle plan; uint32_t slot;
    void *p = nullptr; size_t n = 0;
    DevBuf(CUDPPHandle h, uint32_t s) : plan(h), slot(s) {}
    hipError_t reserve(size_t m)
    {
        if (m <= n) return hipSuccess;
        const hipError_t e = plan_codec_scratch(plan, slot, m, reinterpret_cast<uint8_t **>(&p));
        if (e == hipSuccess) n = m; else { p = nullptr; n = 0; }
        return e;
    }
};

// Input staging is double-buffered: the copy of frame i + 1 into pinned memory and onto the device runs while frame i encodes;
// a frame's container bytes come back through pinned memory once the device cursor says how many there are.
CUDPPResult compress_stream(CUDPPHandle plan, Source &src, unsigned long long len, Sink &out, unsigned long long *outLen)
{
    Encoder E;
    if (!E.P.ok(plan)) return CUDPP_ERROR_INVALID_PLAN;
    CT_TRY(E.init());
    const unsigned long long fmax = (unsigned long long)E.P.n * E.P.rows;
    Pinned hin[2] = {{plan, CT_PIN_IN0}, {plan, CT_PIN_IN1}}, hout{plan, CT_PIN_OUT};
    DevBuf din[2] = {{plan, CT_DEV_IN0}, {plan, CT_DEV_IN1}}, dout{plan, CT_DEV_OUT};
    const size_t inb = (size_t)std::min(fmax, std::max(len, 1ull));
    for (int i = 0; i < 2; i++) { CT_TRY(hin[i].reserve(inb)); CT_TRY(din[i].reserve(inb)); }
    // (a last chunk: blocks + tail; with the CHOOSE codec a chunk may come out as one frame per block)
    const unsigned long long ocap = (E.codec == CT_CODEC_CHOOSE ? E.P.rows * frame_bound(1, E.P.n) : frame_bound(E.P.rows, E.P.n) + frame_bound(1, E.P.n)) + CT_TRAILER;
    CT_TRY(dout.reserve(ocap));
    CT_TRY(hout.reserve(ocap));
    uint32_t hdr[8];
    make_header(hdr, E.fmt, E.P.n, len);
    if (!out.write(hdr, CT_HDR)) return fail(plan, CT_CAPACITY);
    unsigned long long total = CT_HDR;
    hipStream_t cs = nullptr;
    CT_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{cs};
    hipEvent_t copied[2] = {nullptr, nullptr}, used[2] = {nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; int n; ~EvGuard() { for (int i = 0; i < n; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } eg1{copied, 2}, eg2{used, 2};
    for (int i = 0; i < 2; i++) {
        CT_TRY(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
        CT_TRY(hipEventCreateWithFlags(&used[i], hipEventDisableTiming));
    }
    // chunk i: input bytes [i * fmax, ...) -- a frame of `rows` blocks, or the last blocks and the tail
    const unsigned long long nchunk = (len + fmax - 1) / fmax;
    auto stage = [&](unsigned long long i) -> CUDPPResult {
        const int k = (int)(i & 1);
        const size_t m = (size_t)std::min(fmax, len - i * fmax);
        CT_TRY(hipEventSynchronize(used[k]));                 // (an unrecorded event is complete)
        if (!src.read(hin[k].p, m)) return fail(plan, CT_TRUNCATED);
        CT_TRY(hipMemcpyAsync(din[k].p, hin[k].p, m, hipMemcpyHostToDevice, cs));
        CT_TRY(hipEventRecord(copied[k], cs));
        return CUDPP_SUCCESS;
    };
    CT_TRY(ct_enc_header(E.P.st, static_cast<uint8_t *>(dout.p), 0, hdr, E.state));   // (cap 0: state only)
    if (nchunk) { CUDPPResult r = stage(0); if (r != CUDPP_SUCCESS) return r; }
    for (unsigned long long i = 0; i < nchunk; i++) {
        const int k = (int)(i & 1);
        const unsigned long long m = std::min(fmax, len - i * fmax);
        CT_TRY(hipStreamWaitEvent(E.P.st, copied[k], 0));
        CT_TRY(hipMemsetAsync(&E.state->cursor, 0, 8, E.P.st));
        CUDPPResult r = E.frames(static_cast<const uint8_t *>(din[k].p), m, static_cast<uint8_t *>(dout.p), ocap);
        if (r != CUDPP_SUCCESS) return r;
        plan_join(plan);
        CT_TRY(hipEventRecord(used[k], E.P.st));
        if (i + 1 < nchunk) { r = stage(i + 1); if (r != CUDPP_SUCCESS) return r; }
        unsigned long long fb = 0;
        CT_TRY(hipMemcpyAsync(&fb, &E.state->cursor, 8, hipMemcpyDeviceToHost, E.P.st));
        CT_TRY(hipStreamSynchronize(E.P.st));
        if (fb > ocap) return fail(plan, CT_CAPACITY);
        CT_TRY(hipMemcpyAsync(hout.p, dout.p, fb, hipMemcpyDeviceToHost, E.P.st));   // (on the plan's stream: hipMemcpy goes through stream 0)
        CT_TRY(hipStreamSynchronize(E.P.st));
        if (!out.write(hout.p, fb)) return fail(plan, CT_CAPACITY);
        total += fb;
    }
    CT_TRY(hipMemsetAsync(&E.state->cursor, 0, 8, E.P.st));
    CT_TRY(ct_enc_trailer(E.P.st, static_cast<uint8_t *>(dout.p), ocap, E.state, E.d_len));
    CT_TRY(hipMemcpyAsync(hout.p, dout.p, CT_TRAILER, hipMemcpyDeviceToHost, E.P.st));
    CT_TRY(hipStreamSynchronize(E.P.st));
    if (!out.write(hout.p, CT_TRAILER)) return fail(plan, CT_CAPACITY);
    total += CT_TRAILER;
    if (outLen) *outLen = total;
    return E.succeeded();
}

// -------------------------------------------------------------------------------------------------------------------------
// decode: one walk over a stream's frames, fed from device memory or from a Source
// -------------------------------------------------------------------------------------------------------------------------
struct Feed {
    virtual ~Feed() {}
    // n = 32 or 16 header bytes at stream position pos, into host memory (frame: the index a failure names, ~0 = none)
    virtual CUDPPResult header(void *dst, unsigned long long pos, size_t n, unsigned long long frame) = 0;
    // the device pointers of the fb-byte frame at pos, whose header fh has been fetched, and of its ob output bytes, which
    // follow `done` decoded ones
    virtual CUDPPResult frame(const uint32_t fh[8], unsigned long long pos, unsigned long long fb, unsigned long long done, size_t ob,
                              uint32_t fi, const uint8_t **fr, uint8_t **out) = 0;
    virtual CUDPPResult taken(size_t ob) = 0;                    // the frame's output is complete on the plan's stream
};

// stream header -> frames -> trailer -> the decoded bytes' verdict over ct_walk(), the walk the frame index makes as well;
// cap: the room for output.  Returns the stream's total.
CUDPPResult walk_result(CUDPPHandle plan, const CtWalkEnd &end, CUDPPResult stopped)
{
    if (end.what == CT_WALK_STOPPED) return stopped;
    if (end.what == CT_WALK_CONFIG) { set_error(plan, CT_OK); return CUDPP_ERROR_ILLEGAL_CONFIGURATION; }
    if (end.what != CT_OK) return fail(plan, end.what, end.frame);
    set_error(plan, CT_OK);
    return CUDPP_SUCCESS;
}

CUDPPResult decode_walk(Decoder &D, Feed &feed, unsigned long long len, unsigned long long cap, unsigned long long *total)
{
    const CUDPPHandle plan = D.P.h;
    CUDPPResult r = CUDPP_SUCCESS;                              // why a callback stopped the walk
    const CtWalkEnd end = ct_walk(
        h_crc, len, D.P.n, plan_container_settings(plan).reader(),   // a plan with the sparse and runs modes off is a version-4 reader
        [&](uint32_t *dst, unsigned long long pos, uint32_t bytes, unsigned long long frame) {
            return (r = feed.header(dst, pos, bytes, frame)) == CUDPP_SUCCESS;
        },
        [&](const uint32_t *, const CtFormat &fmt, uint32_t, unsigned long long tot) {
            D.fmt = fmt;
            *total = tot;
            if (tot > cap) r = fail(plan, CT_CAPACITY);
            else r = hip_result(D.begin());
            return r == CUDPP_SUCCESS;
        },
        [&](uint32_t fi, const uint32_t *fh, const CtFrameRef &F) {
            const size_t ob = (size_t)F.nb * F.bl;
            const uint8_t *fr = nullptr;
            uint8_t *out = nullptr;
            if ((r = feed.frame(fh, F.pos, frame_bytes(F.nb, F.bl, F.pw), F.out_off, ob, fi, &fr, &out)) != CUDPP_SUCCESS) return false;
            if ((r = D.frame(fr, F.nb, F.bl, F.pw, F.filter, out, fi)) != CUDPP_SUCCESS) return false;
            return (r = feed.taken(ob)) == CUDPP_SUCCESS;
        },
        [&](const uint32_t *tr, uint32_t) { return (r = D.end(tr[2])) == CUDPP_SUCCESS; });
    return walk_result(plan, end, r);
}

// the caller's device buffers: headers come by a device-to-host copy, frames are decoded where they lie
struct DeviceFeed : Feed {
    hipStream_t st;
    const uint8_t *in;
    uint8_t *out;
    DeviceFeed(hipStream_t s, const void *i, void *o) : st(s), in(static_cast<const uint8_t *>(i)), out(static_cast<uint8_t *>(o)) {}
    CUDPPResult header(void *dst, unsigned long long pos, size_t n, unsigned long long) override
    {
        CT_TRY(hipMemcpyAsync(dst, in + pos, n, hipMemcpyDeviceToHost, st));
        CT_TRY(hipStreamSynchronize(st));
        return CUDPP_SUCCESS;
    }
    CUDPPResult frame(const uint32_t *, unsigned long long pos, unsigned long long, unsigned long long done, size_t, uint32_t,
                      const uint8_t **fr, uint8_t **o) override
    {
        *fr = in + pos; *o = out + done;
        return CUDPP_SUCCESS;
    }
    CUDPPResult taken(size_t) override { return CUDPP_SUCCESS; }
};

// a Source read in order and a Sink: a frame goes through pinned memory onto the device, its output back the same way
struct StreamFeed : Feed {
    CUDPPHandle plan;
    hipStream_t st;
    Source &src;
    Sink &sink;
    Pinned hf, ho;
    DevBuf df, dob;
    StreamFeed(CUDPPHandle p, hipStream_t s, Source &i, Sink &o)
        : plan(p), st(s), src(i), sink(o), hf(p, CT_PIN_IN0), ho(p, CT_PIN_OUT), df(p, CT_DEV_IN0), dob(p, CT_DEV_OUT) {}
    CUDPPResult header(void *dst, unsigned long long, size_t n, unsigned long long frame) override
    {
        return src.read(dst, n) ? CUDPP_SUCCESS : fail(plan, CT_TRUNCATED, frame);
    }
    CUDPPResult frame(const uint32_t fh[8], unsigned long long, unsigned long long fb, unsigned long long, size_t ob, uint32_t fi,
                      const uint8_t **fr, uint8_t **o) override
    {
        // room for the worst frame of this one's shape (fh[1] blocks of fh[2] bytes, all stored raw), not for its own bytes alone:
        // the next stream of the same shape, however it compresses, then finds the staging large enough and nothing is freed
        const size_t room = (size_t)std::max(fb, frame_bound(fh[1], fh[2]));
        CT_TRY(hf.reserve(room)); CT_TRY(df.reserve(room));
        CT_TRY(ho.reserve(ob)); CT_TRY(dob.reserve(ob));
        memcpy(hf.p, fh, CT_FRAME_HDR);
        if (!src.read(static_cast<uint8_t *>(hf.p) + CT_FRAME_HDR, fb - CT_FRAME_HDR)) return fail(plan, CT_TRUNCATED, fi);
        CT_TRY(hipMemcpyAsync(df.p, hf.p, fb, hipMemcpyHostToDevice, st));
        *fr = static_cast<const uint8_t *>(df.p); *o = static_cast<uint8_t *>(dob.p);
        return CUDPP_SUCCESS;
    }
    CUDPPResult taken(size_t ob) override
    {
        CT_TRY(hipMemcpyAsync(ho.p, dob.p, ob, hipMemcpyDeviceToHost, st));
        CT_TRY(hipStreamSynchronize(st));
        return sink.write(ho.p, ob) ? CUDPP_SUCCESS : fail(plan, CT_CAPACITY);
    }
};

CUDPPResult decompress_stream(CUDPPHandle plan, Source &src, unsigned long long len, Sink &out, unsigned long long cap,
                              unsigned long long *outLen)
{
    Decoder D;
    if (!D.P.ok(plan)) return CUDPP_ERROR_INVALID_PLAN;
    StreamFeed feed(plan, D.P.st, src, out);
    unsigned long long total = 0;
    const CUDPPResult r = decode_walk(D, feed, len, cap, &total);
    if (r == CUDPP_SUCCESS && outLen) *outLen = total;
    return r;
}

// the two file entry points: stat and open, the streamed call, close; a failing close of the output fails a call that had not
template <class Call>
CUDPPResult with_files(const char *inPath, const char *outPath, Call call)
{
    if (!inPath || !outPath) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    struct stat sb;
    if (stat(inPath, &sb) != 0) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    FILE *fi = fopen(inPath, "rb");
    if (!fi) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    FILE *fo = fopen(outPath, "wb");
    if (!fo) { fclose(fi); return CUDPP_ERROR_ILLEGAL_CONFIGURATION; }
    FileSource s(fi);
    FileSink k(fo);
    CUDPPResult r = call(s, (unsigned long long)sb.st_size, k);
    fclose(fi);
    if (fclose(fo) != 0 && r == CUDPP_SUCCESS) r = CUDPP_ERROR_UNKNOWN;
    return r;
}

// -------------------------------------------------------------------------------------------------------------------------
// the frame index and range reads.  An index is ct_walk() over a container's headers and nothing else: 32 bytes per frame
// from a host buffer or a file, one launch of k_ct_index and one readback for device memory.  A range read takes the frames
// the range overlaps from the index, fetches each of them whole, gives it the checks of the full decode (Decoder::frame with
// a block subset), decodes the blocks the range needs into the plan's staging and delivers the range's bytes from there.
// -------------------------------------------------------------------------------------------------------------------------
struct RandomSource {                                            // container bytes by position: a host buffer or a file
    virtual ~RandomSource() {}
    virtual bool at(void *dst, unsigned long long pos, size_t n) = 0;            // exactly n bytes or false
};
struct MemRandom : RandomSource {
    const uint8_t *p; unsigned long long len;
    MemRandom(const void *q, unsigned long long n) : p(static_cast<const uint8_t *>(q)), len(n) {}
    bool at(void *dst, unsigned long long pos, size_t n) override
    {
        if (pos > len || n > len - pos) return false;
        memcpy(dst, p + pos, n);
        return true;
    }
};
struct FileRandom : RandomSource {
    int fd = -1;
    unsigned long long len = 0;
    explicit FileRandom(const char *path)
    {
        struct stat sb;
        if (path && (fd = open(path, O_RDONLY)) >= 0) {
            if (fstat(fd, &sb) == 0) len = (unsigned long long)sb.st_size;
            else { close(fd); fd = -1; }
        }
    }
    ~FileRandom() { if (fd >= 0) close(fd); }
    bool at(void *dst, unsigned long long pos, size_t n) override
    {
        uint8_t *d = static_cast<uint8_t *>(dst);
        while (n) {
            const ssize_t k = pread(fd, d, n, (off_t)pos);
            if (k <= 0) return false;
            d += k; pos += (unsigned long long)k; n -= (size_t)k;
        }
        return true;
    }
};

CUDPPResult index_result(CUDPPHandle plan, std::unique_ptr<GlcContainerIndex> &ix, const CtWalkEnd &end, CUDPPResult stopped,
                         GlcContainerIndex **index)
{
    const CUDPPResult r = walk_result(plan, end, stopped);
    if (r != CUDPP_SUCCESS) return r;
    ix->fmt = CtFormat();
    (void)parse_volume_format(ix->hdr, &ix->fmt);
    ix->block_len = ix->hdr[2];
    ix->total = (unsigned long long)ix->hdr[4] | ((unsigned long long)ix->hdr[5] << 32);
    *index = ix.release();
    return CUDPP_SUCCESS;
}

CUDPPResult index_host(CUDPPHandle plan, RandomSource &src, unsigned long long len, GlcContainerIndex **index)
{
    Plan P;
    if (const CUDPPResult bad = P.check(plan)) return bad;
    if (!index) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    std::unique_ptr<GlcContainerIndex> ix(new (std::nothrow) GlcContainerIndex);
    if (!ix) return CUDPP_ERROR_INSUFFICIENT_RESOURCES;
    ix->len = len;
    CUDPPResult r = CUDPP_SUCCESS;
    const CtWalkEnd end = ct_walk(
        h_crc, len, P.n, plan_container_settings(plan).reader(),
        [&](uint32_t *dst, unsigned long long pos, uint32_t bytes, unsigned long long frame) {
            if (src.at(dst, pos, bytes)) return true;
            r = fail(plan, CT_TRUNCATED, frame);
            return false;
        },
        [&](const uint32_t *h, const CtFormat &, uint32_t, unsigned long long) { memcpy(ix->hdr, h, CT_HDR); return true; },
        [&](uint32_t, const uint32_t *, const CtFrameRef &ref) {
            try { ix->frames.push_back(ref); } catch (const std::bad_alloc &) { r = CUDPP_ERROR_INSUFFICIENT_RESOURCES; return false; }
            return true;
        },
        [&](const uint32_t *tr, uint32_t) { memcpy(ix->trailer, tr, CT_TRAILER); return true; });
    return index_result(plan, ix, end, r, index);
}

// where a range read's container bytes come from and where its output goes
struct RangeIO {
    virtual ~RangeIO() {}
    virtual CUDPPResult small(void *dst, unsigned long long pos, size_t n) = 0;           // a few bytes into host memory
    // the fb-byte frame at pos in device memory, ordered on the plan's stream, and its 32-byte header in host memory
    virtual CUDPPResult frame(unsigned long long pos, unsigned long long fb, const uint8_t **fr, uint32_t fh[8]) = 0;
    // n decoded bytes in device memory (ready on the plan's stream) are bytes [out_pos, + n) of the range
    virtual CUDPPResult deliver(const uint8_t *d_src, size_t n, unsigned long long out_pos) = 0;
};
struct DeviceRangeIO : RangeIO {
    hipStream_t st;
    const uint8_t *in;
    uint8_t *out;
    DeviceRangeIO(hipStream_t s, const void *i, void *o) : st(s), in(static_cast<const uint8_t *>(i)), out(static_cast<uint8_t *>(o)) {}
    CUDPPResult small(void *dst, unsigned long long pos, size_t n) override
    {
        CT_TRY(hipMemcpyAsync(dst, in + pos, n, hipMemcpyDeviceToHost, st));
        CT_TRY(hipStreamSynchronize(st));
        return CUDPP_SUCCESS;
    }
    CUDPPResult frame(unsigned long long pos, unsigned long long, const uint8_t **fr, uint32_t fh[8]) override
    {
        *fr = in + pos;
        return small(fh, pos, CT_FRAME_HDR);
    }
    CUDPPResult deliver(const uint8_t *d_src, size_t n, unsigned long long out_pos) override
    {
        CT_TRY(hipMemcpyAsync(out + out_pos, d_src, n, hipMemcpyDeviceToDevice, st));
        return CUDPP_SUCCESS;
    }
};
// a host buffer or a file, one frame at a time through pinned memory; the output goes back the same way
struct HostRangeIO : RangeIO {
    hipStream_t st;
    RandomSource &src;
    uint8_t *out;
    Pinned hf, ho;
    DevBuf df;
    HostRangeIO(CUDPPHandle p, hipStream_t s, RandomSource &i, void *o)
        : st(s), src(i), out(static_cast<uint8_t *>(o)), hf(p, CT_PIN_IN0), ho(p, CT_PIN_OUT), df(p, CT_DEV_IN0) {}
    CUDPPResult small(void *dst, unsigned long long pos, size_t n) override { return src.at(dst, pos, n) ? CUDPP_SUCCESS : CUDPP_ERROR_UNKNOWN; }
    CUDPPResult frame(unsigned long long pos, unsigned long long fb, const uint8_t **fr, uint32_t fh[8]) override
    {
        CT_TRY(hf.reserve(fb)); CT_TRY(df.reserve(fb));
        if (!src.at(hf.p, pos, fb)) return CUDPP_ERROR_UNKNOWN;
        memcpy(fh, hf.p, CT_FRAME_HDR);
        CT_TRY(hipMemcpyAsync(df.p, hf.p, fb, hipMemcpyHostToDevice, st));
        *fr = static_cast<const uint8_t *>(df.p);
        return CUDPP_SUCCESS;
    }
    CUDPPResult deliver(const uint8_t *d_src, size_t n, unsigned long long out_pos) override
    {
        CT_TRY(ho.reserve(n));
        CT_TRY(hipMemcpyAsync(ho.p, d_src, n, hipMemcpyDeviceToHost, st));
        CT_TRY(hipStreamSynchronize(st));
        memcpy(out + out_pos, ho.p, n);
        return CUDPP_SUCCESS;
    }
};

// The blocks of a frame of nb blocks of bl bytes that bytes [a, b) of it need (need[blk] = 1), and with a filter the
// elements [*i0, *i1) the range form of the inverse has to produce: whole elements, from the start of the delta's run.
std::vector<uint8_t> needed_blocks(const CtFormat &fmt, uint32_t nb, uint32_t bl, unsigned long long a, unsigned long long b,
                                   unsigned long long *i0, unsigned long long *i1)
{
    std::vector<uint8_t> need(nb, 0);
    const unsigned long long F = (unsigned long long)nb * bl;
    auto mark = [&](unsigned long long lo, unsigned long long hi) {
        for (unsigned long long k = lo / bl; lo < hi && k <= (hi - 1) / bl; k++) need[k] = 1;
    };
    *i0 = *i1 = 0;
    if (!fmt.filtered()) { mark(a, b); return need; }
    const unsigned long long e = fmt.elem, q = F / e;
    const unsigned long long lo = a / e, hi = std::min(q, (b + e - 1) / e);
    if (lo < hi) {                                              // (a range inside the len % elem tail needs no element)
        *i0 = fmt.vol() ? lo - lo % ct_vol_slab(fmt.width, fmt.plane) : fmt.bytes() ? lo - lo % ct_byte_step(fmt.width) : fmt.grid() ? lo - lo % ct_grid_period(fmt.width) : fmt.delta() ? lo & ~2047ull : lo;   // (the slab's, the band's, the run's start)
        *i1 = hi;
        for (unsigned long long j = 0; j < e; j++) mark(j * q + *i0, j * q + *i1);
    }
    if (b > q * e) mark(q * e, F);
    return need;
}

CUDPPResult read_range(Decoder &D, const GlcContainerIndex *ix, RangeIO &io, unsigned long long len, unsigned long long offset,
                       unsigned long long count)
{
    const CUDPPHandle plan = D.P.h;
    if (!ix || len != ix->len || offset > ix->total || count > ix->total - offset) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    unsigned long long stats[3] = {0, 0, 0};                    // frames, blocks decoded, container bytes fetched
    auto done = [&]() {
        set_error(plan, CT_OK);
        memcpy(plan_container_reports(plan).range, stats, sizeof stats);
        return CUDPP_SUCCESS;
    };
    if (count == 0) return done();
    uint32_t hdr[8];
    if (io.small(hdr, 0, CT_HDR) != CUDPP_SUCCESS) return fail(plan, CT_TRUNCATED);
    if (memcmp(hdr, ix->hdr, CT_HDR) != 0) return fail(plan, CT_STREAM_HEADER);           // another container than the index's
    if (ix->fmt.reads() && !(plan_container_settings(plan).reader() & ix->fmt.reads())) return fail(plan, CT_STREAM_HEADER);
    stats[2] = CT_HDR;
    D.fmt = ix->fmt;
    CT_TRY(D.begin());
    const unsigned long long end = offset + count;
    size_t fi = 0, hi = ix->frames.size();                      // the last frame that starts at or before `offset`
    while (hi - fi > 1) {
        const size_t mid = fi + (hi - fi) / 2;
        if (ix->frames[mid].out_off <= offset) fi = mid; else hi = mid;
    }
    for (; fi < ix->frames.size() && ix->frames[fi].out_off < end; fi++) {
        const CtFrameRef &F = ix->frames[fi];
        const unsigned long long fbytes = (unsigned long long)F.nb * F.bl, fb = frame_bytes(F.nb, F.bl, F.pw);
        if (F.bl > D.P.n) { set_error(plan, CT_OK); return CUDPP_ERROR_ILLEGAL_CONFIGURATION; }
        const unsigned long long a = std::max(offset, F.out_off) - F.out_off, b = std::min(end, F.out_off + fbytes) - F.out_off;
        const uint8_t *fr = nullptr;
        uint32_t fh[8];
        unsigned long long pw = 0;
        CUDPPResult r = io.frame(F.pos, fb, &fr, fh);
        if (r == CUDPP_ERROR_UNKNOWN) return fail(plan, CT_TRUNCATED, fi);
        if (r != CUDPP_SUCCESS) return r;
        // the header's range check, on the bytes that are there now: it has to say what the index says
        if (!check_frame_header(fh, ix->fmt, ix->block_len, ix->total - F.out_off, &pw) || fh[1] != F.nb || fh[2] != F.bl || pw != F.pw ||
            fh[3] != F.filter)
            return fail(plan, CT_FRAME_TABLE, fi);
        const CtFormat ff = ct_frame_format(ix->fmt, F.filter);   // the frame's own filter under version 10, else the stream's
        unsigned long long i0 = 0, i1 = 0;
        const std::vector<uint8_t> need = needed_blocks(ff, F.nb, F.bl, a, b, &i0, &i1);
        uint8_t *stage = nullptr;
        if ((r = D.frame(fr, F.nb, F.bl, F.pw, F.filter, nullptr, (uint32_t)fi, need.data(), &stage, &stats[1])) != CUDPP_SUCCESS) return r;
        stats[0] += 1;
        stats[2] += fb;
        const unsigned long long at = F.out_off - offset;       // (+ a frame byte = its place in the range; never negative there)
        if (!ff.filtered()) {
            if ((r = io.deliver(stage + a, b - a, at + a)) != CUDPP_SUCCESS) return r;
            continue;
        }
        const unsigned long long e = ff.elem, q = fbytes / e;
        if (i0 < i1) {                                          // elements [i0, i1) into the second staging, [a, min(b, q e)) out of them
            uint8_t *el = nullptr;
            CT_TRY(plan_stage(plan, 1, (i1 - i0) * e, &el));
            if (ff.bytes()) CT_TRY(unbyte_delta_range_device(D.P.st, stage, el, q, ff.lag(), ff.width, i0, i1 - i0));
            else if (ff.vol()) CT_TRY(unvol_unshuffle_range_device(D.P.st, stage, el, q, (uint32_t)e, ff.width, ff.plane, ff.fold(), i0, i1 - i0));
            else if (ff.grid()) CT_TRY(ungrid_unshuffle_range_device(D.P.st, stage, el, q, (uint32_t)e, ff.width, ff.fold(), i0, i1 - i0));
            else if (ff.delta()) CT_TRY(unlag_unshuffle_range_device(D.P.st, stage, el, q, (uint32_t)e, ff.lag(), ff.fold(), i0, i1 - i0));
            else CT_TRY(unshuffle_range_device(D.P.st, stage, el, q, (uint32_t)e, i0, i1 - i0));
            const unsigned long long top = std::min(b, q * e);
            if ((r = io.deliver(el + (a - i0 * e), top - a, at + a)) != CUDPP_SUCCESS) return r;
        }
        if (b > q * e) {                                        // the len % elem tail lies in the filtered frame as it is
            const unsigned long long lo = std::max(a, q * e);
            if ((r = io.deliver(stage + lo, b - lo, at + lo)) != CUDPP_SUCCESS) return r;
        }
    }
    const CUDPPResult r = D.end(0, false);
    if (r != CUDPP_SUCCESS) return r;
    return done();
}

// the four glcContainerLast* entries: n values of the plan's reports.  Two of them (loose) tell only a bad handle: a live plan that
// is not a COMPRESS plan has no container call behind it, so they answer it with the values no call has touched.
template <class Pick>
CUDPPResult last_report(CUDPPHandle plan, bool loose, unsigned long long *out, size_t n, Pick pick)
{
    Plan P;
    const CUDPPResult bad = P.check(plan);
    if (bad == CUDPP_ERROR_INVALID_HANDLE || (bad && !loose)) return bad;
    if (!out) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const CtReports untouched;
    memcpy(out, pick(bad ? untouched : plan_container_reports(plan)), n * sizeof *out);
    return CUDPP_SUCCESS;
}

// the glcPlanSet/GetContainer* entries: the plan check, then the setter's own rule (CtSettings: false = refused, nothing changed);
// the plan check, then the null-output check, then the read
template <class Set>
CUDPPResult ct_set(CUDPPHandle plan, Set set)
{
    Plan P;
    if (const CUDPPResult bad = P.check(plan)) return bad;
    return set(plan_container_settings(plan)) ? CUDPP_SUCCESS : CUDPP_ERROR_ILLEGAL_CONFIGURATION;
}
template <class Get>
CUDPPResult ct_get(CUDPPHandle plan, unsigned int *out, Get get)
{
    Plan P;
    if (const CUDPPResult bad = P.check(plan)) return bad;
    if (!out) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    *out = get(plan_container_settings(plan));
    return CUDPP_SUCCESS;
}

} // namespace

extern "C" {

CUDPPResult glcContainerIndexDevice(CUDPPHandle plan, const void *d_in, unsigned long long len, GlcContainerIndex **index)
{
    Plan P;
    if (const CUDPPResult bad = P.check(plan)) return bad;
    if (!d_in || !index || (reinterpret_cast<uintptr_t>(d_in) & 7)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    std::unique_ptr<GlcContainerIndex> ix(new (std::nothrow) GlcContainerIndex);
    if (!ix) return CUDPP_ERROR_INSUFFICIENT_RESOURCES;
    ix->len = len;
    // no frame is smaller than one block of one byte with an empty payload, so len bounds the entries before the header is read
    const unsigned long long cap = len / frame_bytes(1, 1, 0) + 1;
    uint8_t *scratch = nullptr;
    CT_TRY(plan_codec_scratch(plan, 2, sizeof(CtIndexHead) + cap * sizeof(CtFrameRef), &scratch));
    CtIndexHead *d_head = reinterpret_cast<CtIndexHead *>(scratch);
    CtFrameRef *d_ent = reinterpret_cast<CtFrameRef *>(scratch + sizeof(CtIndexHead));
    CT_TRY(ct_index_device(P.st, static_cast<const uint8_t *>(d_in), len, P.n, plan_container_settings(plan).reader(), d_head, d_ent, cap));
    // one readback: the head and the first entries; a container of more frames than that fetches the rest
    const size_t first = (size_t)std::min<unsigned long long>(cap, CT_INDEX_FIRST);
    std::vector<uint8_t> back(sizeof(CtIndexHead) + first * sizeof(CtFrameRef));
    CT_TRY(hipMemcpyAsync(back.data(), scratch, back.size(), hipMemcpyDeviceToHost, P.st));
    CT_TRY(hipStreamSynchronize(P.st));
    CtIndexHead head;
    memcpy(&head, back.data(), sizeof(head));
    if (head.what == CT_OK) {
        if (head.frames > cap) return CUDPP_ERROR_UNKNOWN;
        ix->frames.resize(head.frames);
        const size_t got = std::min<size_t>(head.frames, first);
        if (got) memcpy(ix->frames.data(), back.data() + sizeof(CtIndexHead), got * sizeof(CtFrameRef));
        if (head.frames > got) {
            CT_TRY(hipMemcpyAsync(ix->frames.data() + got, d_ent + got, (head.frames - got) * sizeof(CtFrameRef), hipMemcpyDeviceToHost, P.st));
            CT_TRY(hipStreamSynchronize(P.st));
        }
        memcpy(ix->hdr, head.hdr, CT_HDR);
        memcpy(ix->trailer, head.trailer, CT_TRAILER);
    }
    return index_result(plan, ix, CtWalkEnd{head.what, head.frame}, CUDPP_ERROR_UNKNOWN, index);
}

CUDPPResult glcContainerIndex(CUDPPHandle plan, const void *in, unsigned long long len, GlcContainerIndex **index)
{
    if (!in) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    MemRandom src(in, len);
    return index_host(plan, src, len, index);
}

CUDPPResult glcContainerIndexFile(CUDPPHandle plan, const char *path, GlcContainerIndex **index)
{
    FileRandom src(path);
    if (src.fd < 0) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return index_host(plan, src, src.len, index);
}

void glcContainerIndexFree(GlcContainerIndex *index) { delete index; }

CUDPPResult glcContainerIndexInfo(const GlcContainerIndex *index, unsigned long long out[4])
{
    if (!index || !out) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    out[0] = index->total; out[1] = index->block_len; out[2] = index->frames.size();
    out[3] = index->fmt.version | ((unsigned long long)index->fmt.flags << 16) | ((unsigned long long)index->fmt.word3() << 32);
    return CUDPP_SUCCESS;
}

CUDPPResult glcContainerIndexPlane(const GlcContainerIndex *index, unsigned int *plane)
{
    if (!index || !plane) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    *plane = index->fmt.plane;
    return CUDPP_SUCCESS;
}

CUDPPResult glcContainerReadRangeDevice(CUDPPHandle plan, const GlcContainerIndex *index, const void *d_in, unsigned long long len,
                                        unsigned long long offset, unsigned long long count, void *d_out)
{
    Decoder D;
    if (const CUDPPResult bad = D.P.check(plan)) return bad;
    if (!d_in || (count && !d_out) || (reinterpret_cast<uintptr_t>(d_in) & 7)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    DeviceRangeIO io(D.P.st, d_in, d_out);
    return read_range(D, index, io, len, offset, count);
}

CUDPPResult glcContainerReadRange(CUDPPHandle plan, const GlcContainerIndex *index, const void *in, unsigned long long len,
                                  unsigned long long offset, unsigned long long count, void *out)
{
    Decoder D;
    if (const CUDPPResult bad = D.P.check(plan)) return bad;
    if (!in || (count && !out)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    MemRandom src(in, len);
    HostRangeIO io(D.P.h, D.P.st, src, out);
    return read_range(D, index, io, len, offset, count);
}

CUDPPResult glcContainerReadRangeFile(CUDPPHandle plan, const GlcContainerIndex *index, const char *path, unsigned long long offset,
                                      unsigned long long count, void *out)
{
    Decoder D;
    if (const CUDPPResult bad = D.P.check(plan)) return bad;
    FileRandom src(path);
    if (src.fd < 0 || (count && !out)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    HostRangeIO io(D.P.h, D.P.st, src, out);
    return read_range(D, index, io, src.len, offset, count);
}

unsigned long long glcContainerBound(unsigned long long len, size_t blockLen)
{
    if (blockLen == 0 || blockLen > MAX_BLOCK_ELEMS) return 0;
    const unsigned long long frames = (len + blockLen - 1) / blockLen;
    return CT_HDR + CT_TRAILER + len + frames * (CT_FRAME_HDR + 4 * ct_tables(1, (uint32_t)blockLen).words + 7);
}

CUDPPResult glcContainerCompressDevice(CUDPPHandle plan, const void *d_in, unsigned long long len, void *d_out,
                                       unsigned long long cap, unsigned long long *d_outLen)
{
    Encoder E;
    if (const CUDPPResult bad = E.P.check(plan)) return bad;
    if ((len && !d_in) || !d_out || !d_outLen || (reinterpret_cast<uintptr_t>(d_out) & 7)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(E.init());
    uint8_t *out = static_cast<uint8_t *>(d_out);
    uint32_t hdr[8];
    make_header(hdr, E.fmt, E.P.n, len);
    CT_TRY(ct_enc_header(E.P.st, out, cap, hdr, E.state));
    CUDPPResult r = E.frames(static_cast<const uint8_t *>(d_in), len, out, cap);
    if (r != CUDPP_SUCCESS) return r;
    plan_join(plan);
    CT_TRY(ct_enc_trailer(E.P.st, out, cap, E.state, d_outLen));
    unsigned long long total = 0;
    CT_TRY(hipMemcpyAsync(&total, d_outLen, 8, hipMemcpyDeviceToHost, E.P.st));
    CT_TRY(hipStreamSynchronize(E.P.st));
    if (total > cap) return fail(plan, CT_CAPACITY);
    return E.succeeded();
}

CUDPPResult glcContainerDecompressDevice(CUDPPHandle plan, const void *d_in, unsigned long long len, void *d_out,
                                         unsigned long long cap, unsigned long long *d_outLen)
{
    Decoder D;
    if (const CUDPPResult bad = D.P.check(plan)) return bad;
    if (!d_in || !d_outLen || (reinterpret_cast<uintptr_t>(d_in) & 7)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    DeviceFeed feed(D.P.st, d_in, d_out);
    unsigned long long total = 0;
    const CUDPPResult r = decode_walk(D, feed, len, d_out ? cap : 0, &total);     // (without an output buffer only an empty stream fits)
    if (r != CUDPP_SUCCESS) return r;
    CT_TRY(ct_put_u64(D.P.st, d_outLen, total));
    CT_TRY(hipStreamSynchronize(D.P.st));
    return CUDPP_SUCCESS;
}

CUDPPResult glcContainerCompress(CUDPPHandle plan, const void *in, unsigned long long len, void *out, unsigned long long cap,
                                 unsigned long long *outLen)
{
    if ((len && !in) || !out) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    MemSource s(in, len);
    MemSink k(out, cap);
    return compress_stream(plan, s, len, k, outLen);
}

CUDPPResult glcContainerDecompress(CUDPPHandle plan, const void *in, unsigned long long len, void *out, unsigned long long cap,
                                   unsigned long long *outLen)
{
    if (!in || (cap && !out)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    MemSource s(in, len);
    MemSink k(out, cap);
    return decompress_stream(plan, s, len, k, cap, outLen);
}

CUDPPResult glcContainerCompressFile(CUDPPHandle plan, const char *inPath, const char *outPath)
{
    return with_files(inPath, outPath, [&](Source &s, unsigned long long len, Sink &k) { return compress_stream(plan, s, len, k, nullptr); });
}

CUDPPResult glcContainerDecompressFile(CUDPPHandle plan, const char *inPath, const char *outPath)
{
    return with_files(inPath, outPath, [&](Source &s, unsigned long long len, Sink &k) { return decompress_stream(plan, s, len, k, ~0ull, nullptr); });
}

CUDPPResult glcContainerLastError(CUDPPHandle plan, unsigned long long out[3])
{
    return last_report(plan, true, out, 3, [](const CtReports &r) { return r.error; });
}

CUDPPResult glcContainerLastRangeStats(CUDPPHandle plan, unsigned long long out[3])
{
    return last_report(plan, true, out, 3, [](const CtReports &r) { return r.range; });
}

CUDPPResult glcContainerLastChoice(CUDPPHandle plan, unsigned long long out[3])
{
    return last_report(plan, false, out, 3, [](const CtReports &r) { return r.choice; });
}

CUDPPResult glcContainerLastFilters(CUDPPHandle plan, unsigned long long out[8])
{
    return last_report(plan, false, out, FILTER_CANDS + 1, [](const CtReports &r) { return r.filters; });
}

CUDPPResult glcContainerLastLagFilters(CUDPPHandle plan, unsigned long long out[4])
{
    return last_report(plan, false, out, LAG_ELEMS + 1, [](const CtReports &r) { return r.lag_filters; });
}

CUDPPResult glcContainerLastGridFilters(CUDPPHandle plan, unsigned long long out[4])
{
    return last_report(plan, false, out, LAG_ELEMS + 1, [](const CtReports &r) { return r.grid_filters; });
}

CUDPPResult glcContainerLastByteFilters(CUDPPHandle plan, unsigned long long out[3])
{
    return last_report(plan, false, out, BYTE_ROWS + 1, [](const CtReports &r) { return r.byte_filters; });
}

CUDPPResult glcPlanSetContainerShuffle(CUDPPHandle plan, unsigned int elem)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_shuffle(elem); });
}

CUDPPResult glcPlanSetContainerDelta(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_delta(on); });
}

CUDPPResult glcPlanSetContainerCodec(CUDPPHandle plan, unsigned int codec)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_codec(codec); });
}

CUDPPResult glcPlanSetContainerSparse(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_mode(CT_MODE_SPARSE, on); });
}

CUDPPResult glcPlanSetContainerRuns(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_mode(CT_MODE_RUNS, on); });
}

CUDPPResult glcPlanSetContainerAns(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_mode(CT_MODE_ANS, on); });
}

CUDPPResult glcPlanSetContainerAuto(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_mode(CT_MODE_AUTO, on); });
}

CUDPPResult glcPlanSetContainerDedup(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_mode(CT_MODE_DEDUP, on); });
}

CUDPPResult glcPlanSetContainerFilterAuto(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_filter_auto(on); });
}

CUDPPResult glcPlanSetContainerFilterLag(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_filter_lag(on); });
}

CUDPPResult glcPlanSetContainerFilterGrid(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_filter_grid(on); });
}

CUDPPResult glcPlanSetContainerFilterByte(CUDPPHandle plan, unsigned int on)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_filter_byte(on); });
}

CUDPPResult glcPlanGetContainerShuffle(CUDPPHandle plan, unsigned int *elem)
{
    return ct_get(plan, elem, [](const CtSettings &s) { return s.shuffle; });
}

CUDPPResult glcPlanGetContainerDelta(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.delta ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerCodec(CUDPPHandle plan, unsigned int *codec)
{
    return ct_get(plan, codec, [](const CtSettings &s) { return s.codec; });
}

CUDPPResult glcPlanGetContainerSparse(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.mode == CT_MODE_SPARSE ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerRuns(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.mode == CT_MODE_RUNS ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerAns(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.mode == CT_MODE_ANS ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerAuto(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.mode == CT_MODE_AUTO ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerDedup(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.mode == CT_MODE_DEDUP ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerFilterAuto(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.filter_auto ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerFilterLag(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.filter_lag ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerFilterGrid(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.filter_grid ? 1u : 0u; });
}

CUDPPResult glcPlanGetContainerFilterByte(CUDPPHandle plan, unsigned int *on)
{
    return ct_get(plan, on, [](const CtSettings &s) { return s.filter_byte ? 1u : 0u; });
}

CUDPPResult glcPlanSetContainerChooseFilters(CUDPPHandle plan, unsigned int level)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_choose_filters(level); });
}

CUDPPResult glcPlanGetContainerChooseFilters(CUDPPHandle plan, unsigned int *level)
{
    return ct_get(plan, level, [](const CtSettings &s) { return s.choose_filters; });
}

CUDPPResult glcPlanSetContainerDeltaLag(CUDPPHandle plan, unsigned int lag, unsigned int fold)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_delta_lag(lag, fold); });
}

CUDPPResult glcPlanGetContainerDeltaLag(CUDPPHandle plan, unsigned int *lag, unsigned int *fold)
{
    if (!fold) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const CUDPPResult r = ct_get(plan, lag, [](const CtSettings &s) { return s.lag; });
    return r != CUDPP_SUCCESS ? r : ct_get(plan, fold, [](const CtSettings &s) { return s.fold; });
}

CUDPPResult glcPlanSetContainerDeltaGrid(CUDPPHandle plan, unsigned int width, unsigned int fold)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_delta_grid(width, fold); });
}

CUDPPResult glcPlanGetContainerDeltaGrid(CUDPPHandle plan, unsigned int *width, unsigned int *fold)
{
    if (!fold) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const CUDPPResult r = ct_get(plan, width, [](const CtSettings &s) { return s.grid_width; });
    return r != CUDPP_SUCCESS ? r : ct_get(plan, fold, [](const CtSettings &s) { return s.grid_fold; });
}

CUDPPResult glcPlanSetContainerDeltaVolume(CUDPPHandle plan, unsigned int plane)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_delta_volume(plane); });
}

CUDPPResult glcPlanGetContainerDeltaVolume(CUDPPHandle plan, unsigned int *plane)
{
    return ct_get(plan, plane, [](const CtSettings &s) { return s.vol_plane; });
}

CUDPPResult glcPlanSetContainerByteDelta(CUDPPHandle plan, unsigned int lag, unsigned int stride)
{
    return ct_set(plan, [&](CtSettings &s) { return s.set_byte_delta(lag, stride); });
}

CUDPPResult glcPlanGetContainerByteDelta(CUDPPHandle plan, unsigned int *lag, unsigned int *stride)
{
    if (!stride) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const CUDPPResult r = ct_get(plan, lag, [](const CtSettings &s) { return s.byte_lag; });
    return r != CUDPP_SUCCESS ? r : ct_get(plan, stride, [](const CtSettings &s) { return s.byte_stride; });
}

} // extern "C"
