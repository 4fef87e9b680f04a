// segments_api.cpp -- the plan-less calls of include/glc_container.h: each takes device segments (a base, offsets and lengths) or
// one device buffer and a stream, refuses a bad argument before anything is enqueued, and enqueues the kernels of one pass -- the
// CRC of segments (container.hip), the byte-plane shuffle, the delta + shuffle and its lagged, folded form with their range forms
// (shuffle.hip, delta.hip, lag.hip), the 2-D predictor over it (grid.hip) and the 3-D predictor over that (vol.hip),
// the sparse split and join (sparse.hip), the dedup map and fill (dedup.hip), the zero-run split and join (zrun.hip), the rANS
// coder (ans.hip) and the probes (auto.hip, choose.hip, filter_probe.hip, lag_probe.hip, grid_probe.hip).  The container over a plan, which runs the same
// passes inside its frames, is container_api.cpp.
#include "../../include/glc_container.h"
#include "container_internal.h"

using namespace glc;

namespace {

bool lag_ok(unsigned int lag, unsigned int fold) { return lag >= 1 && lag <= 16 && fold <= 1; }

CUDPPResult range_filter_api(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned long long first,
                             unsigned long long count, void *stream, bool delta, unsigned int lag = 1, unsigned int fold = 0,
                             const unsigned int *width = nullptr, const unsigned int *plane = nullptr)
{
    if (!shuffle_elem_ok(elem) || !lag_ok(lag, fold) || (width && !ct_grid_width_ok(*width)) || (plane && !ct_vol_plane_ok(*width, *plane)))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const unsigned long long q = len / elem;
    const uint32_t step = plane ? ct_vol_slab(*width, *plane) : width ? ct_grid_period(*width) : 2048u;
    if (first > q || count > q - first || (delta && first % step)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (a < b + count * elem && b < a + len)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t *in = static_cast<const uint8_t *>(d_in);
    uint8_t *out = static_cast<uint8_t *>(d_out);
    if (plane) return hip_result(unvol_unshuffle_range_device(st, in, out, q, elem, *width, *plane, fold, first, count));
    if (width) return hip_result(ungrid_unshuffle_range_device(st, in, out, q, elem, *width, fold, first, count));
    return hip_result(delta ? unlag_unshuffle_range_device(st, in, out, q, elem, lag, fold, first, count)      // ((1, 0): delta.hip's)
                            : unshuffle_range_device(st, in, out, q, elem, first, count));
}

} // namespace

extern "C" {

CUDPPResult glcCrc32Segments(const void *d_base, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                             size_t count, unsigned int *d_crc, void *stream)
{
    if (count == 0) return CUDPP_SUCCESS;
    if (!d_offsets || !d_lengths || !d_crc || count > 0xFFFFFFFFull) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return hip_result(crc32_segments(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_base), d_offsets,
                                  d_lengths, (uint32_t)count, d_crc));
}

static CUDPPResult shuffle_segments_api(const void *d_inBase, void *d_outBase, const unsigned long long *d_offsets,
                                        const unsigned long long *d_lengths, size_t count, unsigned int elem, void *stream, bool inverse)
{
    // (one offset serves both bases, so equal bases are the in-place call; what else might overlap is in device memory)
    if (!shuffle_elem_ok(elem) || count > 0xFFFFFFFFull) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    if (!d_inBase || !d_outBase || d_inBase == d_outBase || !d_offsets || !d_lengths) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return hip_result(shuffle_segments(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase),
                                    static_cast<uint8_t *>(d_outBase), d_offsets, d_lengths, (uint32_t)count, elem, inverse));
}

static CUDPPResult shuffle_device_api(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream, bool inverse,
                                      bool delta = false, unsigned int lag = 1, unsigned int fold = 0, const unsigned int *width = nullptr,
                                      const unsigned int *plane = nullptr)
{
    CtFormat f;                                               // (only its filter matters here)
    f.flags = delta ? CT_FLAG_DELTA : 0; f.elem = elem;
    if (!shuffle_elem_ok(elem) || !lag_ok(lag, fold) || (width && !ct_grid_width_ok(*width)) || (plane && !ct_vol_plane_ok(*width, *plane)))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (plane) { f.version = CT_VERSION_VOL; f.flags |= (fold ? CT_FLAG_FOLD : 0u) | CT_FLAG_GRID | CT_FLAG_VOL; f.width = *width; f.plane = *plane; }
    else if (width) { f.version = CT_VERSION_GRID; f.flags |= (fold ? CT_FLAG_FOLD : 0u) | CT_FLAG_GRID; f.width = *width; }
    else if (lag != 1 || fold) { f.version = CT_VERSION_LAG; f.flags |= (fold ? CT_FLAG_FOLD : 0u) | (lag - 1) << CT_LAG_SHIFT; }
    if (len == 0) return CUDPP_SUCCESS;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (a < b ? b - a : a - b) < len) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return hip_result(filter_device(reinterpret_cast<hipStream_t>(stream), f, static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out),
                                 len, inverse));
}

CUDPPResult glcShuffleSegments(const void *d_inBase, void *d_outBase, const unsigned long long *d_offsets,
                               const unsigned long long *d_lengths, size_t count, unsigned int elem, void *stream)
{
    return shuffle_segments_api(d_inBase, d_outBase, d_offsets, d_lengths, count, elem, stream, false);
}

CUDPPResult glcUnshuffleSegments(const void *d_inBase, void *d_outBase, const unsigned long long *d_offsets,
                                 const unsigned long long *d_lengths, size_t count, unsigned int elem, void *stream)
{
    return shuffle_segments_api(d_inBase, d_outBase, d_offsets, d_lengths, count, elem, stream, true);
}

CUDPPResult glcShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, false);
}

CUDPPResult glcUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, true);
}

CUDPPResult glcDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, false, true);
}

CUDPPResult glcUndeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, true, true);
}

CUDPPResult glcUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned long long first,
                                    unsigned long long count, void *stream)
{
    return range_filter_api(d_in, d_out, len, elem, first, count, stream, false);
}

CUDPPResult glcUndeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                           unsigned long long first, unsigned long long count, void *stream)
{
    return range_filter_api(d_in, d_out, len, elem, first, count, stream, true);
}

CUDPPResult glcLagDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int lag,
                                     unsigned int fold, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, false, true, lag, fold);
}

CUDPPResult glcUnlagDeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int lag,
                                         unsigned int fold, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, true, true, lag, fold);
}

CUDPPResult glcUnlagDeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                              unsigned int lag, unsigned int fold, unsigned long long first,
                                              unsigned long long count, void *stream)
{
    return range_filter_api(d_in, d_out, len, elem, first, count, stream, true, lag, fold);
}

CUDPPResult glcGridDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                      unsigned int fold, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, false, true, 1, fold, &width);
}

CUDPPResult glcUngridDeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                          unsigned int fold, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, true, true, 1, fold, &width);
}

CUDPPResult glcUngridDeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                               unsigned int width, unsigned int fold, unsigned long long first,
                                               unsigned long long count, void *stream)
{
    return range_filter_api(d_in, d_out, len, elem, first, count, stream, true, 1, fold, &width);
}

CUDPPResult glcVolDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                     unsigned int plane, unsigned int fold, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, false, true, 1, fold, &width, &plane);
}

CUDPPResult glcUnvolDeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                         unsigned int plane, unsigned int fold, void *stream)
{
    return shuffle_device_api(d_in, d_out, len, elem, stream, true, true, 1, fold, &width, &plane);
}

CUDPPResult glcUnvolDeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                              unsigned int width, unsigned int plane, unsigned int fold, unsigned long long first,
                                              unsigned long long count, void *stream)
{
    return range_filter_api(d_in, d_out, len, elem, first, count, stream, true, 1, fold, &width, &plane);
}

// the byte predictor's three calls (byte_delta.hip): glcDeltaShuffleDevice's rules over one-byte elements
static CUDPPResult byte_delta_api(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride, void *stream,
                                  bool inverse)
{
    if (!ct_byte_lag_ok(lag) || !ct_byte_stride_ok(stride)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (len == 0) return CUDPP_SUCCESS;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (a < b ? b - a : a - b) < len) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return hip_result(byte_delta_device(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out),
                                     len, lag, stride, inverse));
}

CUDPPResult glcByteDeltaDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride, void *stream)
{
    return byte_delta_api(d_in, d_out, len, lag, stride, stream, false);
}

CUDPPResult glcUnbyteDeltaDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride, void *stream)
{
    return byte_delta_api(d_in, d_out, len, lag, stride, stream, true);
}

CUDPPResult glcUnbyteDeltaRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride,
                                      unsigned long long first, unsigned long long count, void *stream)
{
    if (!ct_byte_lag_ok(lag) || !ct_byte_stride_ok(stride)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (first > len || count > len - first || first % ct_byte_step(stride)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_in), b = reinterpret_cast<uintptr_t>(d_out);
    if (!d_in || !d_out || (a < b + count && b < a + len)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    return hip_result(unbyte_delta_range_device(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_in),
                                             static_cast<uint8_t *>(d_out), len, lag, stride, first, count));
}

// the two sparse calls: a bad argument is refused before anything is enqueued
static bool sparse_args_ok(const void *a, const void *b, const void *c, const void *d, const void *e, const void *f, size_t count, size_t maxLen)
{
    return count <= 0xFFFFFFFFull && maxLen <= GLC_SPARSE_MAX_LEN && (count == 0 || (a && b && c && d && e && f));
}

CUDPPResult glcSparseSplitSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, const unsigned int *d_fill, unsigned int *d_mask, void *d_keptBase,
                                   unsigned long long *d_keptLen, void *stream)
{
    if (!sparse_args_ok(d_inBase, d_offsets, d_lengths, d_fill, d_mask, d_keptBase, count, maxLen) || (count && !d_keptLen) ||
        (count && d_inBase == d_keptBase) || (reinterpret_cast<uintptr_t>(d_mask) & 3))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const SpSegs g{static_cast<uint8_t *>(const_cast<void *>(d_inBase)), d_offsets, d_lengths, static_cast<uint8_t *>(d_keptBase), d_offsets,
                   d_fill, d_mask, nullptr, sp_mask_words((uint32_t)maxLen), nullptr, (uint32_t)count, (uint32_t)maxLen};
    CT_TRY(sparse_mask(st, g));
    CT_TRY(sparse_count(st, g, d_keptLen));
    CT_TRY(sparse_compact(st, g));
    return CUDPP_SUCCESS;
}

CUDPPResult glcSparseJoinSegments(const void *d_keptBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                  size_t count, size_t maxLen, const unsigned int *d_fill, const unsigned int *d_mask, void *d_outBase,
                                  void *stream)
{
    if (!sparse_args_ok(d_keptBase, d_offsets, d_lengths, d_fill, d_mask, d_outBase, count, maxLen) || (count && d_keptBase == d_outBase) ||
        (reinterpret_cast<uintptr_t>(d_mask) & 3))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    const SpSegs g{static_cast<uint8_t *>(d_outBase), d_offsets, d_lengths, static_cast<uint8_t *>(const_cast<void *>(d_keptBase)), d_offsets,
                   d_fill, const_cast<unsigned int *>(d_mask), nullptr, sp_mask_words((uint32_t)maxLen), nullptr, (uint32_t)count,
                   (uint32_t)maxLen};
    CT_TRY(sparse_join(reinterpret_cast<hipStream_t>(stream), g));
    return CUDPP_SUCCESS;
}

// the dedup calls: a bad argument is refused before anything is enqueued
static size_t dedup_chunks(size_t count, size_t maxLen)
{
    if (count > GLC_DEDUP_MAX_COUNT || maxLen > GLC_DEDUP_MAX_LEN) return (size_t)-1;
    const size_t chunks = count * ((maxLen + DD_CHUNK - 1) / DD_CHUNK);
    return chunks > DD_MAX_CHUNKS ? (size_t)-1 : chunks;
}

size_t glcDedupWorkBytes(size_t count, size_t maxLen)
{
    const size_t chunks = dedup_chunks(count, maxLen);
    if (chunks == (size_t)-1 || chunks == 0) return 0;
    return (dedup_slots(chunks) + 1) * sizeof(DdSlot) + chunks * sizeof(uint64_t);
}

CUDPPResult glcDedupMapSegments(const void *d_base, const unsigned long long *d_offsets, const unsigned long long *d_lengths, size_t count,
                                size_t maxLen, unsigned int *d_src, void *d_work, size_t workBytes, void *stream)
{
    const size_t chunks = dedup_chunks(count, maxLen);
    if (chunks == (size_t)-1) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (chunks == 0) return CUDPP_SUCCESS;
    if (!d_base || !d_offsets || !d_lengths || !d_src || !d_work || (reinterpret_cast<uintptr_t>(d_src) & 3) ||
        (reinterpret_cast<uintptr_t>(d_work) & 15) || workBytes < glcDedupWorkBytes(count, maxLen))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const size_t slots = dedup_slots(chunks);
    DdSlot *table = static_cast<DdSlot *>(d_work);
    const DdSegs g{static_cast<uint8_t *>(const_cast<void *>(d_base)), d_offsets, d_lengths, reinterpret_cast<uint64_t *>(table + slots + 1),
                   table, (uint32_t)slots, d_src, (uint32_t)count, (uint32_t)maxLen, (uint32_t)((maxLen + DD_CHUNK - 1) / DD_CHUNK)};
    CT_TRY(dedup_map(reinterpret_cast<hipStream_t>(stream), g));
    return CUDPP_SUCCESS;
}

CUDPPResult glcDedupFillSegments(void *d_outBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths, size_t count,
                                 size_t maxLen, const unsigned int *d_src, void *stream)
{
    const size_t chunks = dedup_chunks(count, maxLen);
    if (chunks == (size_t)-1) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (chunks == 0) return CUDPP_SUCCESS;
    if (!d_outBase || !d_offsets || !d_lengths || !d_src || (reinterpret_cast<uintptr_t>(d_src) & 3)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    const DdSegs g{static_cast<uint8_t *>(d_outBase), d_offsets, d_lengths, nullptr, nullptr, 0, const_cast<unsigned int *>(d_src),
                   (uint32_t)count, (uint32_t)maxLen, (uint32_t)((maxLen + DD_CHUNK - 1) / DD_CHUNK)};
    CT_TRY(dedup_fill(reinterpret_cast<hipStream_t>(stream), g));
    return CUDPP_SUCCESS;
}

// the two zero-run calls: a bad argument is refused before anything is enqueued
static bool zrun_args_ok(const void *x, const void *off, const void *len, const void *a, const void *b, const void *alen, const void *blen,
                         size_t count, size_t maxLen)
{
    return count <= 0xFFFFFFFFull && maxLen <= GLC_ZERORUN_MAX_LEN && (count == 0 || (x && off && len && a && b && alen && blen)) &&
           (count == 0 || (x != a && x != b && a != b));
}

CUDPPResult glcZeroRunSplitSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                    size_t count, size_t maxLen, void *d_aBase, void *d_bBase, unsigned long long *d_aLen,
                                    unsigned long long *d_bLen, void *stream)
{
    if (!zrun_args_ok(d_inBase, d_offsets, d_lengths, d_aBase, d_bBase, d_aLen, d_bLen, count, maxLen)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    const ZrSegs g{static_cast<uint8_t *>(const_cast<void *>(d_inBase)), d_offsets, d_lengths, static_cast<uint8_t *>(d_aBase), d_offsets, d_aLen,
                   static_cast<uint8_t *>(d_bBase), d_offsets, d_bLen, nullptr, (uint32_t)count, (uint32_t)maxLen};
    CT_TRY(zrun_split(reinterpret_cast<hipStream_t>(stream), g));
    return CUDPP_SUCCESS;
}

CUDPPResult glcZeroRunJoinSegments(const void *d_aBase, const void *d_bBase, const unsigned long long *d_offsets,
                                   const unsigned long long *d_aLen, const unsigned long long *d_bLen, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, void *d_outBase, void *stream)
{
    if (!zrun_args_ok(d_outBase, d_offsets, d_lengths, d_aBase, d_bBase, d_aLen, d_bLen, count, maxLen)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    const ZrSegs g{static_cast<uint8_t *>(d_outBase), d_offsets, d_lengths, static_cast<uint8_t *>(const_cast<void *>(d_aBase)), d_offsets,
                   const_cast<unsigned long long *>(d_aLen), static_cast<uint8_t *>(const_cast<void *>(d_bBase)), d_offsets,
                   const_cast<unsigned long long *>(d_bLen), nullptr, (uint32_t)count, (uint32_t)maxLen};
    CT_TRY(zrun_join(reinterpret_cast<hipStream_t>(stream), g));
    return CUDPP_SUCCESS;
}

// the two rANS calls: a bad argument is refused before anything is enqueued.  The work space: the tables, what the batched
// histogram kernel's table step writes beside them, and the encoder's chunk slots
struct AnsWork {
    uint8_t *tab, *lens; uint16_t *codes; unsigned long long *nun; AnsScratch sc;
    size_t carve(void *base, size_t count, size_t maxLen)
    {
        Carver c(base);
        const size_t nch = ans_chunks((uint32_t)maxLen), slots = count * nch;
        c.align(256);
        tab = c.take<uint8_t>(count * ANS_TAB_BYTES);
        nun = c.take<unsigned long long>(count);
        sc.states = c.take<uint32_t>(slots * ANS_LANES);
        sc.counts = c.take<uint32_t>(slots);
        codes = c.take<uint16_t>(256 * count);
        lens = c.take<uint8_t>(256 * count);
        c.align(256);
        sc.units = c.take<uint16_t>(slots * ANS_CHUNK);
        sc.nch_max = (uint32_t)nch;
        return c.bytes();
    }
};

size_t glcAnsBoundWords(size_t len) { return len > GLC_ANS_MAX_LEN ? 0 : (size_t)ans_bound_words((uint32_t)len); }

size_t glcAnsSegmentsWorkBytes(size_t count, size_t maxLen)
{
    if (count > GLC_ANS_MAX_COUNT || maxLen > GLC_ANS_MAX_LEN) return 0;
    AnsWork w;
    return w.carve(nullptr, count, maxLen);
}

static bool ans_args_ok(const void *data, const void *off, const void *len, const void *hist, const void *rec, const void *recOff,
                        const void *recWords, const void *work, size_t workBytes, size_t count, size_t maxLen)
{
    if (count > GLC_ANS_MAX_COUNT || maxLen > GLC_ANS_MAX_LEN) return false;
    if (count == 0) return true;
    return data && off && len && hist && rec && recOff && recWords && work && data != rec && (reinterpret_cast<uintptr_t>(rec) & 3) == 0 &&
           (reinterpret_cast<uintptr_t>(hist) & 3) == 0 && workBytes >= glcAnsSegmentsWorkBytes(count, maxLen);
}

CUDPPResult glcAnsEncodeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, unsigned int *d_hist, unsigned int *d_recBase,
                                 const unsigned long long *d_recOffsets, unsigned long long *d_recWords, void *d_work, size_t workBytes,
                                 void *stream)
{
    if (!ans_args_ok(d_inBase, d_offsets, d_lengths, d_hist, d_recBase, d_recOffsets, d_recWords, d_work, workBytes, count, maxLen))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AnsWork w;
    (void)w.carve(d_work, count, maxLen);
    const HdbSegs h{static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count, (uint32_t)maxLen};
    CT_TRY(hdb_tables(st, h, true, d_hist, w.lens, w.codes, nullptr, w.nun, nullptr, nullptr));
    const AnsSegs g{static_cast<uint8_t *>(const_cast<void *>(d_inBase)), d_offsets, d_lengths, d_hist, w.tab, nullptr, (uint32_t)count,
                    (uint32_t)maxLen};
    CT_TRY(ans_tables(st, g));
    CT_TRY(ans_encode(st, g, w.sc));
    CT_TRY(ans_words(st, g, w.sc, d_recWords));
    CT_TRY(ans_place(st, g, w.sc, d_recBase, d_recOffsets, ~0ull));
    return CUDPP_SUCCESS;
}

CUDPPResult glcAnsDecodeSegments(const unsigned int *d_recBase, const unsigned long long *d_recOffsets, const unsigned long long *d_recWords,
                                 const unsigned int *d_hist, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, void *d_outBase, void *d_work, size_t workBytes, void *stream)
{
    if (!ans_args_ok(d_outBase, d_offsets, d_lengths, d_hist, d_recBase, d_recOffsets, d_recWords, d_work, workBytes, count, maxLen))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    AnsWork w;
    (void)w.carve(d_work, count, maxLen);
    const AnsSegs g{static_cast<uint8_t *>(d_outBase), d_offsets, d_lengths, d_hist, w.tab, nullptr, (uint32_t)count, (uint32_t)maxLen};
    CT_TRY(ans_tables(st, g));
    CT_TRY(ans_decode(st, g, d_recBase, d_recOffsets, d_recWords));
    return CUDPP_SUCCESS;
}

// the probe: a bad argument is refused before anything is enqueued
CUDPPResult glcProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                             size_t count, size_t maxLen, unsigned int *d_hist, unsigned int *d_uniform, void *stream)
{
    if (count > GLC_PROBE_MAX_COUNT || maxLen > GLC_PROBE_MAX_LEN) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    if (!d_inBase || !d_offsets || !d_lengths || !d_hist || !d_uniform || d_hist == d_uniform || (reinterpret_cast<uintptr_t>(d_hist) & 3) ||
        (reinterpret_cast<uintptr_t>(d_uniform) & 3)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(probe_segments(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                          (uint32_t)maxLen, d_hist, d_uniform));
    return CUDPP_SUCCESS;
}

// the bigram probe: a bad argument is refused before anything is enqueued
CUDPPResult glcBigramProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, unsigned long long *d_stats, void *stream)
{
    if (count > GLC_PROBE_MAX_COUNT || maxLen > GLC_PROBE_MAX_LEN) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    if (!d_inBase || !d_offsets || !d_lengths || !d_stats || (reinterpret_cast<uintptr_t>(d_stats) & 7)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(bigram_probe_segments(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths,
                                 (uint32_t)count, (uint32_t)maxLen, d_stats));
    return CUDPP_SUCCESS;
}

// the filter probe: a bad argument is refused before anything is enqueued
CUDPPResult glcFilterProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, unsigned int *d_planes, unsigned long long *d_costs, void *stream)
{
    if (count > GLC_PROBE_MAX_COUNT || maxLen > GLC_FILTER_PROBE_MAX_LEN) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    if (!d_inBase || !d_offsets || !d_lengths || !d_planes || !d_costs || (reinterpret_cast<uintptr_t>(d_planes) & 15) ||
        (reinterpret_cast<uintptr_t>(d_costs) & 7) || static_cast<void *>(d_planes) == static_cast<void *>(d_costs))
        return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(filter_probe_segments(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths,
                                 (uint32_t)count, (uint32_t)maxLen, d_planes, d_costs));
    return CUDPP_SUCCESS;
}

// the two lag probes and the two grid probes: a bad argument is refused before anything is enqueued
static bool lag_probe_args_ok(const void *in, const void *off, const void *len, size_t count, size_t maxLen, const void *a, unsigned aAlign,
                              const void *b, unsigned bAlign)
{
    if (count > GLC_PROBE_MAX_COUNT || maxLen > GLC_FILTER_PROBE_MAX_LEN) return false;
    if (count == 0) return true;
    return in && off && len && a && b && a != b && !(reinterpret_cast<uintptr_t>(a) & (aAlign - 1)) && !(reinterpret_cast<uintptr_t>(b) & (bAlign - 1));
}

CUDPPResult glcLagProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                size_t count, size_t maxLen, unsigned long long *d_sums, unsigned int *d_lags, void *stream)
{
    if (!lag_probe_args_ok(d_inBase, d_offsets, d_lengths, count, maxLen, d_sums, 8, d_lags, 4)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    CT_TRY(lag_probe_sums(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                          (uint32_t)maxLen, d_sums, d_lags));
    return CUDPP_SUCCESS;
}

CUDPPResult glcLagPlanesSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, const unsigned int *d_lags, unsigned int *d_planes,
                                 unsigned long long *d_costs, void *stream)
{
    if (!lag_probe_args_ok(d_inBase, d_offsets, d_lengths, count, maxLen, d_planes, 16, d_costs, 8)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    // (the lags are read while the outputs are written: neither output may be them)
    if (!d_lags || (reinterpret_cast<uintptr_t>(d_lags) & 3) || static_cast<const void *>(d_lags) == d_planes ||
        static_cast<const void *>(d_lags) == d_costs) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(lag_probe_planes(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                            (uint32_t)maxLen, d_lags, d_planes, d_costs));
    return CUDPP_SUCCESS;
}

CUDPPResult glcGridProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, unsigned int *d_sums, unsigned int *d_widths, void *stream)
{
    if (!lag_probe_args_ok(d_inBase, d_offsets, d_lengths, count, maxLen, d_sums, 4, d_widths, 4)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    CT_TRY(grid_probe_sums(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                           (uint32_t)maxLen, d_sums, d_widths));
    return CUDPP_SUCCESS;
}

CUDPPResult glcGridPlanesSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                  size_t count, size_t maxLen, const unsigned int *d_widths, unsigned int *d_planes,
                                  unsigned long long *d_costs, void *stream)
{
    if (!lag_probe_args_ok(d_inBase, d_offsets, d_lengths, count, maxLen, d_planes, 16, d_costs, 8)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    // (the widths are read while the outputs are written: neither output may be them)
    if (!d_widths || (reinterpret_cast<uintptr_t>(d_widths) & 3) || static_cast<const void *>(d_widths) == d_planes ||
        static_cast<const void *>(d_widths) == d_costs) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(grid_probe_planes(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                             (uint32_t)maxLen, d_widths, d_planes, d_costs));
    return CUDPP_SUCCESS;
}

// the two byte probes: a bad argument is refused before anything is enqueued
CUDPPResult glcByteProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, unsigned long long *d_lagSums, unsigned int *d_strideSums,
                                 unsigned int *d_winners, void *stream)
{
    if (!lag_probe_args_ok(d_inBase, d_offsets, d_lengths, count, maxLen, d_lagSums, 8, d_strideSums, 4)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    if (!d_winners || (reinterpret_cast<uintptr_t>(d_winners) & 3) || static_cast<void *>(d_winners) == d_lagSums ||
        d_winners == d_strideSums) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(byte_probe_sums(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                           (uint32_t)maxLen, d_lagSums, d_strideSums, d_winners));
    return CUDPP_SUCCESS;
}

CUDPPResult glcBytePlanesSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                  size_t count, size_t maxLen, const unsigned int *d_words, unsigned int *d_planes,
                                  unsigned long long *d_costs, void *stream)
{
    if (!lag_probe_args_ok(d_inBase, d_offsets, d_lengths, count, maxLen, d_planes, 16, d_costs, 8)) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    if (count == 0) return CUDPP_SUCCESS;
    // (the words are read while the outputs are written: neither output may be them)
    if (!d_words || (reinterpret_cast<uintptr_t>(d_words) & 3) || static_cast<const void *>(d_words) == d_planes ||
        static_cast<const void *>(d_words) == d_costs) return CUDPP_ERROR_ILLEGAL_CONFIGURATION;
    CT_TRY(byte_probe_planes(reinterpret_cast<hipStream_t>(stream), static_cast<const uint8_t *>(d_inBase), d_offsets, d_lengths, (uint32_t)count,
                             (uint32_t)maxLen, d_words, d_planes, d_costs));
    return CUDPP_SUCCESS;
}

} // extern "C"
