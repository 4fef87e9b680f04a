/*
 * glc_container.h -- a CRC-checked, self-describing container around the BWT codec (cudppCompress path): any length in,
 * one stream out, read back bit-exactly or refused.  Format: INTEGRATION.md section 4b.
 *
 * The input is cut into blocks of the plan's n bytes; up to `rows` of them make a frame, one batched encode; a ragged tail is
 * a frame of one block.  A block whose Huffman record would not fit the format (a 4096-symbol sub-block needing more than 1536
 * words) or would not save a quarter (4 * words >= block bytes) is stored raw.  Every block carries the CRC-32 of its bytes
 * and of its record, every frame the CRC of its tables, the stream the CRC of the whole input (CRC-32/IEEE, = zlib.crc32).
 *
 * Typed data (float32, float64, 16-bit codes): an optional byte-plane shuffle filter, off by default.  With an element size of
 * 2, 4 or 8 set on the encoding plan, every frame is shuffled as one segment on the device before its blocks are cut -- byte j of
 * every element gathered into plane j -- and the stream is written as format version 2, whose header names the element size; the
 * decoder reads it there, whatever its own plan's setting, and hands back the original bytes.  A block's CRC is then that of
 * the shuffled block, the stream's still that of the original input.  With the filter off the container is version 1, byte for
 * byte what it always was.  Choose rows as a multiple of the element size so that blocks and planes coincide.
 *
 * A second codec, chosen by the caller: GLC_CONTAINER_CODEC_HUFF0 codes every block with an order-0 canonical Huffman table of
 * its own (at most 11 bits, the CUHD-shaped stream of include/glc_hd.h) instead of suffix sort + move-to-front + Huffman.  It does
 * no sort, and is smaller on data without context structure (i.i.d. symbols, quantised or shuffled numeric data); text and logs
 * want the BWT codec.  Measured on one MI355X on 4 GiB of Zipf(1.0) bytes in 1 MiB blocks (profiles/container_codec.md): ratio
 * 1.275 against 1.121, encode 533 against 103 GB/s, decode 100 against 45 GB/s; sizes for other inputs in INTEGRATION.md 4b.
 * Such a stream is format version 3, with or without the filter.
 *
 * Integer series (timestamps, sorted ids, offsets, counters, ADC samples): the filter's delta mode, off by default.  With
 * glcPlanSetContainerDelta on, a frame's elements are replaced by their differences to the element in front (modulo 2^(8 elem),
 * restarting every 2048 elements of the frame) before the planes are gathered, in the same single pass over the frame; the stream
 * is format version 4 with either codec.  Slowly varying integers have flat byte histograms after the shuffle alone and peaked ones
 * after the delta, which is what the order-0 codec needs: the model's sizes are in INTEGRATION.md 4b.  It hurts
 * noise-like data.  The decoder reads what was done from the stream header.
 *
 * Sparse data (zero pages, masks, tensors with few non-zeros, the all-zero byte planes of a shuffled integer series): the sparse
 * mode of the order-0 codec, off by default.  A Huffman code spends at least one bit per byte, so a block of one repeated byte
 * still costs an eighth of its size.  With glcPlanSetContainerSparse on, a block is cut into chunks of 64 bytes, the chunks that
 * consist of the block's most frequent byte are left out, a mask of one bit per chunk says which, and only the kept chunks are
 * Huffman-coded (record kind 3); a block with fewer than one such chunk in 32 stays an ordinary order-0 record.  The stream is
 * format version 5.  The model's sizes are in INTEGRATION.md 4b ("sparse: when").  Measured on one MI355X on 1 GiB of int64
 * timestamps in 1 MiB blocks with delta + shuffle 8 (profiles/sparse_mode.md): ratio 6.771 against 4.192 with the mode off, encode
 * 460 against 417 GB/s, decode 174 against 134 GB/s; uint32 counters 9.999 against 5.280, 468 against 424 and 199 against 146.
 *
 * Text and logs, further: the runs mode of the BWT codec, off by default.  The move-to-front output of text is mostly zeros, a
 * Huffman code spends at least a bit on each, and the reference's stream has a new table every 4096 symbols, so the BWT codec
 * stopped at 8 : 1 on anything.  With glcPlanSetContainerRuns on, a block's move-to-front bytes are split into A (the non-zero
 * bytes and one zero per run of zeros) and B (the run lengths; a run ends at a 256-byte tile edge), and each is coded with one
 * order-0 table of its own (record kind 4).  The stream is format version 6.  The model's sizes are in INTEGRATION.md 4b
 * ("runs: when"): 1 MiB blocks of text 4.687 against 3.715, of logs 6.622 against 4.187, a repeated page 287.1 against 7.816.
 * A plan reads version 6 only with the mode on, and version 5 only with the sparse mode on, which needs the other codec: no
 * single plan reads both.  Measured on one MI355X on 1 GiB of device-generated data in 1 MiB blocks, rows 512
 * (profiles/runs_mode.md; ratio / encode / decode GB/s, medians of 5 interleaved rounds): text-like, mode off 3.715 / 24.7 /
 * 41.2, on 4.872 / 23.1 / 29.4; log-like, off 3.916 / 17.3 / 41.9, on 5.867 / 16.6 / 29.9. With the mode off the rates equal
 * the parent commit's within the spread of the rounds. Decode is slower with the mode on: the batched order-0 decoder's
 * k_hdb_span_functions takes 5 ms per GiB where the kind-0 record's sub-block offsets let k_dec_huff take 1.7. The split alone
 * moves 316 GB/s and the join 638-820, a device-to-device copy 2542.
 *
 * Scattered skew (quantised gradients and activations, delta'd planes that are mostly 0 and +-1, masks with isolated set bytes):
 * the rANS mode of the order-0 codec, off by default.  No 64-byte chunk of such data is one byte, so the sparse mode elides
 * nothing and the stream stays at Huffman's one bit per byte at best.  With glcPlanSetContainerAns on, a block is coded by
 * interleaved range-ANS against 12-bit probabilities derived from its byte counts (record kind 5): chunks of 32768 bytes, 64
 * interleaved 32-bit states a chunk, 16-bit units, the states stored -- so a symbol of probability q / 4096 costs log2(4096 / q)
 * bits and one wave decodes one chunk straight through, with no synchronisation pass.  The stream is format version 7.  The
 * model's sizes are in INTEGRATION.md 4b ("ans: when"): 1 MiB of bytes that are 90 % zeros, scattered, 7.648 against 5.223 with
 * the mode off or the sparse mode on; the integer series within 3 % of the sparse mode; data that is one byte over whole
 * regions stays the sparse mode's (38.96 against 44.30 on regular-step timestamps); Zipf bytes gain nothing.
 * Measured on one MI355X on 1 GiB of device-generated data in 1 MiB blocks, rows 512 (profiles/ans_mode.md; ratio / encode /
 * decode GB/s, medians of 5 interleaved rounds): scattered 90 % zeros, mode off 5.677 / 552 / 171, on 8.670 / 501 / 450; int64
 * timestamps with delta + shuffle 8, off 4.192 / 415 / 134, sparse 6.771 / 456 / 173, rANS 6.809 / 385 / 359; uint32 counters with
 * delta + shuffle 4, off 5.280 / 418 / 145, sparse 9.999 / 459 / 200, rANS 9.835 / 394 / 365.  Decode with the mode on is 2.5 to
 * 2.7 times faster than the order-0 path with the mode off: k_ans_table + k_ans_decode take about 1.1 ms per GiB where
 * k_hdb_span_functions + k_hdb_emit take about 6.5.  Encode is 6 to 9 % slower: the coder and its placing pass stand where
 * k_hdb_enc_* stood.  With the mode off the rates equal the parent commit's within the spread of the rounds.  The kernels alone:
 * encode 782 GB/s, decode 968, a device-to-device copy 2674.
 *
 * Mixtures, and callers who do not know their data: the auto mode of the order-0 codec, off by default.  The sparse mode stops at
 * 5.223 on scattered skew where rANS reaches 7.648, rANS gets 38.96 on regular-step timestamps where the sparse mode gets 44.30, and
 * a frame of typed data behind delta + shuffle holds planes of both sorts and planes of noise.  With glcPlanSetContainerAuto on, one
 * probe pass over a frame (glcProbeSegments) gives every block's byte counts and its 64-byte chunks of one byte, and each block
 * is coded as the smaller of what the sparse mode's writer would make of it (kinds 3, 2, 1; size known exactly from the counts)
 * and an rANS record (kind 5; size estimated from the counts by integer arithmetic); the mask, compaction and rANS passes run only on
 * the blocks that chose them.  The stream is format version 8, whose frames may mix kinds 0, 1, 2, 3 and 5; no record changes.  The
 * model's sizes are in INTEGRATION.md 4b ("auto: when"): never below the better of the two modes on nine inputs, above both on
 * mixed frames (int64 timestamps 6.412 against 6.188 and 6.261).  A plan with the mode on reads versions 1 to 5, 7 and 8: it is the
 * one reader for everything the order-0 codec has written in versions 1 to 8 (version 9, the dedup mode's, is read by a plan with
 * that mode on).  Measured on one MI355X on 1 GiB of device-generated data in 1 MiB
 * blocks, rows 512 (profiles/auto_mode.md; ratio / encode / decode GB/s, medians of 5 interleaved rounds): int64 timestamps with
 * delta + shuffle 8, sparse 6.771 / 449 / 172, rANS 6.809 / 383 / 353, auto 7.008 / 396 / 291; uint32 counters with delta +
 * shuffle 4, sparse 9.999 / 450 / 198, rANS 9.835 / 387 / 360, auto 10.218 / 401 / 301; scattered 90 % zeros, sparse 5.677 / 470 /
 * 169, rANS 8.670 / 489 / 441, auto 8.670 / 472 / 443.  With the mode off the sizes equal the parent commit's and the rates differ
 * from it by no more than two runs of one build do.  The probe alone: 4864 GB/s on zeros, 3356 on scattered skew, 4038 on noise, where
 * the call that holds the histogram pass alone moves 4081, 3070 and 3724; a device-to-device copy 2584.
 *
 * Callers who do not know their data's type either: filter-auto, off by default.  The filter above is one per stream and has to be
 * known in advance, and a wrong guess costs up to 5 : 1.  With glcPlanSetContainerFilterAuto on (it needs the order-0 codec and the
 * auto mode) one probe pass over every frame (glcFilterProbeSegments) counts the byte planes of all seven candidates -- no filter,
 * the shuffle over 2, 4 or 8 bytes, each with or without the delta -- and the writer gives the frame the cheapest by a margin and
 * names it in the frame header.  The stream is format version 10; nothing else changes.  Measured on one MI355X on 1 GiB of
 * device-generated data in 1 MiB blocks, rows 512 (profiles/filter_auto.md; ratio / encode / decode GB/s, medians of 5 interleaved
 * rounds): int64 timestamps 7.008 / 209 / 295 against 7.008 / 395 / 294 with delta + shuffle 8 set by hand and 1.548 / 435 / 113
 * without a filter; uint32 counters 10.218 / 209 / 304 against 10.218 / 399 / 303; float32 1.198 / 199 / 118 against 1.198 / 362 / 118;
 * text-like 1.884 / 221 / 127 against 1.884 / 441 / 127.  The probe alone moves 506 to 518 GB/s (1475 on zeros; a device-to-device
 * copy 2544 to 2590).  With the setting off the bytes equal the parent commit's and the rates differ from it by no more than two runs
 * of one build do.
 *
 * Plans are CUDPP_COMPRESS plans (include/cudpp.h).  Work is queued on the plan's stream, with or without
 * glcPlanSetPipelining; every call below returns with its outputs complete.  Results: CUDPP_SUCCESS,
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION (bad arguments, a capacity too small -- nothing is ever written past `cap` --, a plan
 * whose n is smaller than the container's blocks), CUDPP_ERROR_UNKNOWN (a container that fails a check, or a failed HIP
 * call); glcContainerLastError says which check.
 */
#ifndef GLC_CONTAINER_H
#define GLC_CONTAINER_H

#include <stddef.h>

#include "cudpp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what glcContainerLastError reports in out[0] */
enum GlcContainerError
{
    GLC_CONTAINER_OK = 0,
    GLC_CONTAINER_STREAM_HEADER = 1,    /* stream header or trailer (magic, version, CRC, frame count, stray bytes) */
    GLC_CONTAINER_FRAME_TABLE = 2,      /* a frame header or its tables: table CRC or a field out of range */
    GLC_CONTAINER_RECORD_CRC = 3,       /* a block's payload record */
    GLC_CONTAINER_DECODED_CRC = 4,      /* the bytes a block decoded to, or the whole output against the trailer */
    GLC_CONTAINER_TRUNCATED = 5,        /* the container ends inside a frame or before its trailer */
    GLC_CONTAINER_CAPACITY = 6          /* the output does not fit `cap` */
};

/* Worst-case container size for `len` input bytes in blocks of `blockLen` (<= 1048576; 0 for a bad blockLen).  Depends
 * on its arguments only; about len + 1.1 KB per block. */
unsigned long long glcContainerBound(unsigned long long len, size_t blockLen);

/* Device buffers.  d_out (and the container d_in of the decoder) must be 8-byte aligned.  *d_outLen is a DEVICE word that
 * receives the container's (decoded) length; after a capacity failure of the encoder it holds the length that was needed.
 * The decoder takes any COMPRESS plan whose n is at least the container's block length, whatever its rows. */
CUDPPResult glcContainerCompressDevice(CUDPPHandle plan, const void *d_in, unsigned long long len, void *d_out,
                                       unsigned long long cap, unsigned long long *d_outLen);
CUDPPResult glcContainerDecompressDevice(CUDPPHandle plan, const void *d_in, unsigned long long len, void *d_out,
                                         unsigned long long cap, unsigned long long *d_outLen);

/* Host buffers (any alignment), staged frame by frame through pinned memory; *outLen is a host word. */
CUDPPResult glcContainerCompress(CUDPPHandle plan, const void *in, unsigned long long len, void *out,
                                 unsigned long long cap, unsigned long long *outLen);
CUDPPResult glcContainerDecompress(CUDPPHandle plan, const void *in, unsigned long long len, void *out,
                                   unsigned long long cap, unsigned long long *outLen);

/* Files, streamed: host and device memory stay proportional to one frame, not to the file. */
CUDPPResult glcContainerCompressFile(CUDPPHandle plan, const char *inPath, const char *outPath);
CUDPPResult glcContainerDecompressFile(CUDPPHandle plan, const char *inPath, const char *outPath);

/* CRC-32/IEEE of `count` device segments [d_base + d_offsets[i], + d_lengths[i]) into d_crc[i], queued on `stream` (a
 * hipStream_t; NULL = default).  Any length and byte alignment.  d_base may be NULL when the offsets are addresses. */
CUDPPResult glcCrc32Segments(const void *d_base, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                             size_t count, unsigned int *d_crc, void *stream);

/* Byte-plane shuffle of device memory, queued on `stream` (a hipStream_t; NULL = default): with q = len / elem whole elements,
 * out[j * q + i] = in[i * elem + j] for 0 <= j < elem, 0 <= i < q, and the last len % elem bytes copied in place; the Unshuffle
 * forms are the inverse.  elem is 2, 4 or 8; any length and byte alignment; out of place only.  The single-segment forms
 * refuse overlapping buffers.  The batched forms take `count` segments [base + d_offsets[i], + d_lengths[i]) with ONE offset
 * array for both bases (offsets and lengths are device arrays); equal bases are refused, and segments must not overlap each
 * other.  A refused call (CUDPP_ERROR_ILLEGAL_CONFIGURATION) has written nothing. */
CUDPPResult glcShuffleSegments(const void *d_inBase, void *d_outBase, const unsigned long long *d_offsets,
                               const unsigned long long *d_lengths, size_t count, unsigned int elem, void *stream);
CUDPPResult glcUnshuffleSegments(const void *d_inBase, void *d_outBase, const unsigned long long *d_offsets,
                                 const unsigned long long *d_lengths, size_t count, unsigned int elem, void *stream);
CUDPPResult glcShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream);
CUDPPResult glcUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream);

/* Delta + shuffle in one pass, and its inverse: with x[i] element i of the segment as a little-endian unsigned integer of `elem`
 * bytes, d[i] = x[i] where i is a multiple of 2048 and x[i] - x[i - 1] modulo 2^(8 elem) elsewhere; out[j * q + i] = byte j of
 * d[i]; the last len % elem bytes copied in place.  The inverse gathers d and sums it from the last multiple of 2048 up to i.
 * The rules of glcShuffleDevice: elem 2, 4 or 8, any length and byte alignment, out of place, overlapping buffers and a bad elem
 * refused (CUDPP_ERROR_ILLEGAL_CONFIGURATION) with nothing written.  Single segment only. */
CUDPPResult glcDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream);
CUDPPResult glcUndeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, void *stream);

/* The delta with a lag and a folded sign (csrc/lag.hip), for interleaved channels and for series whose differences change sign:
 * with W = 8 elem and r = i mod 2048, d[i] = x[i] where r < lag and x[i] - x[i - lag] modulo 2^W elsewhere; f[i] = d[i], or with
 * fold = 1 (d[i] << 1) ^ (0 - (d[i] >> (W - 1))) modulo 2^W (the sign in bit 0, so the upper planes of a small difference of
 * either sign are zero); out[j * q + i] = byte j of f[i]; the last len % elem bytes copied in place.  The inverse gathers f, undoes
 * the fold, d = (f >> 1) ^ (0 - (f & 1)), and sums every lag-th element back to the one with r < lag.  lag is the channel count,
 * 1 to 16; (lag, fold) = (1, 0) is glcDeltaShuffleDevice, byte for byte.  The rules of glcDeltaShuffleDevice; a lag outside 1..16
 * and a fold above 1 are refused like a bad elem.  The range form is glcUndeltaUnshuffleRangeDevice's: `first` a multiple of 2048. */
CUDPPResult glcLagDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int lag,
                                     unsigned int fold, void *stream);
CUDPPResult glcUnlagDeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int lag,
                                         unsigned int fold, void *stream);
CUDPPResult glcUnlagDeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                              unsigned int lag, unsigned int fold, unsigned long long first,
                                              unsigned long long count, void *stream);

/* The 2-D (row-stride) predictor (csrc/grid.hip), for row-major gridded data -- 16-bit images and depth maps, detector frames, 2-D
 * slices of float32 or float64 fields, integer rasters: the delta with a folded sign over the differences to the element one row
 * above.  With arithmetic modulo 2^(8 elem), `width` the row width in elements, 2..65536, and P = 2048 * ceil(width / 64):
 * v[i] = x[i] where i mod P < width and x[i] - x[i - width] elsewhere; d[i] = v[i] where i mod 2048 == 0 and v[i] - v[i - 1]
 * elsewhere; f[i] = d[i], or with fold = 1 (d[i] << 1) ^ (0 - (d[i] >> (8 elem - 1))); out[j * q + i] = byte j of f[i]; the last
 * len % elem bytes copied in place.  The rule is linear in i: a segment needs no row alignment.  The inverse undoes the fold, sums
 * d along every run of 2048 and then adds the row above up every band of P elements.  The rules of glcDeltaShuffleDevice; a width
 * outside 2..65536 and a fold above 1 are refused like a bad elem.  The range form is glcUndeltaUnshuffleRangeDevice's with `first`
 * a multiple of P. */
CUDPPResult glcGridDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                      unsigned int fold, void *stream);
CUDPPResult glcUngridDeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                          unsigned int fold, void *stream);
CUDPPResult glcUngridDeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                               unsigned int width, unsigned int fold, unsigned long long first,
                                               unsigned long long count, void *stream);

/* The byte predictor (csrc/byte_delta.hip), for 8-bit sample data -- greyscale, RGB and RGBA images, masks and label maps, 8-bit
 * depth or detector frames, u8 audio: one-byte elements, so there are no planes, no tail and no fold, and out has the length and the
 * positions of in.  With arithmetic modulo 256, `lag` 1..16 (the channel count), `stride` 0 (none) or 2..65536 (the row length in
 * bytes, channels * width) and P = 2048 * ceil(stride / 64): v[i] = x[i] where stride == 0 or i mod P < stride and
 * x[i] - x[i - stride] elsewhere; out[i] = v[i] where i mod 2048 < lag and v[i] - v[i - lag] elsewhere.  The rule is linear in i: a
 * segment needs no row alignment.  The inverse sums down every chain (i, i - lag, ...) of a run of 2048 and then adds the row above
 * up every band of P bytes.  The rules of glcDeltaShuffleDevice: any length and alignment, out of place, overlapping buffers
 * refused, len 0 succeeds; a lag outside 1..16 and a stride of 1 or above 65536 are CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing
 * written.  The range form writes bytes [first, first + count) of glcUnbyteDeltaDevice's output to d_out[0 .. count): first a
 * multiple of 2048 with stride 0 and of P otherwise, first + count <= len. */
CUDPPResult glcByteDeltaDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride, void *stream);
CUDPPResult glcUnbyteDeltaDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride, void *stream);
CUDPPResult glcUnbyteDeltaRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int lag, unsigned int stride,
                                      unsigned long long first, unsigned long long count, void *stream);

/* The 3-D (plane-stride) predictor (csrc/vol.hip), for row-major volumes -- 3-D float32 or float64 fields, stacks of detector
 * frames, CT and MRI stacks: the 2-D predictor over the differences to the element one plane behind.  With `width` and P as
 * above, `plane` the plane stride S in elements, width < S <= 2^24, and the slab Q = P * ceil(16 S / P): w[i] = x[i] where
 * i mod Q < S and x[i] - x[i - S] elsewhere; then glcGridDeltaShuffleDevice's rule on w.  The rule is linear in i: a segment needs
 * no row or plane alignment and S need not be a multiple of width.  With S >= len / elem the output is glcGridDeltaShuffleDevice's.
 * The inverse is glcUngridDeltaUnshuffleDevice's followed by the sums of the plane behind up every slab.  The rules of
 * glcGridDeltaShuffleDevice; a plane <= width or above 2^24 is refused like a bad width, with nothing written.  The range form is
 * glcUngridDeltaUnshuffleRangeDevice's with `first` a multiple of Q. */
CUDPPResult glcVolDeltaShuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                     unsigned int plane, unsigned int fold, void *stream);
CUDPPResult glcUnvolDeltaUnshuffleDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned int width,
                                         unsigned int plane, unsigned int fold, void *stream);
CUDPPResult glcUnvolDeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                              unsigned int width, unsigned int plane, unsigned int fold, unsigned long long first,
                                              unsigned long long count, void *stream);

/* The two passes of the sparse mode as batched calls (csrc/sparse.hip).  Segment i is [d_offsets[i], + min(d_lengths[i], maxLen)) of
 * its base, cut into chunks of 64 bytes (the last may be short); d_fill[i] & 255 is its fill byte, given by the caller; its mask is
 * row i of d_mask, rows of ceil(ceil(maxLen / 64) / 32) words: bit c % 32 of word c / 32 is 1 when chunk c is kept, 0 when every
 * byte of it equals the fill, and 0 past the last chunk.  Split writes the mask words of every segment, its kept chunks in order
 * at d_keptBase + d_offsets[i] (at most the segment's length) and their byte count to d_keptLen[i].  Join takes the mask, the fill
 * and the kept bytes (exactly the bytes the mask asks for: 64 per kept chunk, fewer for a kept short last chunk) and writes
 * d_lengths[i] bytes at d_outBase + d_offsets[i].  Any length up to GLC_SPARSE_MAX_LEN, any byte alignment, out of place; the calls
 * only enqueue on `stream`.  A bad argument (a null pointer with count > 0, equal bases, a mask not 4-byte aligned, a maxLen
 * or count too large) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_SPARSE_MAX_LEN ((size_t)1 << 28)
CUDPPResult glcSparseSplitSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, const unsigned int *d_fill, unsigned int *d_mask, void *d_keptBase,
                                   unsigned long long *d_keptLen, void *stream);
CUDPPResult glcSparseJoinSegments(const void *d_keptBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                  size_t count, size_t maxLen, const unsigned int *d_fill, const unsigned int *d_mask, void *d_outBase,
                                  void *stream);

/* The two passes of frame-wide chunk dedup as batched calls (csrc/dedup.hip; the hash and the writer's rule are INTEGRATION.md 4b,
 * "dedup").  The segments are the blocks of one frame, in order: segment i is [d_offsets[i], + min(d_lengths[i], maxLen)) of its
 * base, cut into chunks of 512 bytes from its start (the last may be short); with nch = ceil(maxLen / 512), chunk c of segment i has
 * the id i * nch + c.  Map writes d_src[id] for every id below count * nch: the id of the chunk's source under the writer's rule --
 * the smallest id whose chunk has the same 64-bit hash, when that id is smaller and the two chunks agree in length and in every
 * byte -- and the chunk's own id otherwise (a kept chunk; also the entry of an id past its segment's end).  A source is therefore
 * always a kept chunk.  d_work: glcDedupWorkBytes(count, maxLen) bytes of device memory, 16-byte aligned, for the duration of the
 * call's work (a hash table of 16 bytes a slot, at least two slots a chunk, and 8 bytes of hash per chunk).  Fill is the inverse, in
 * place: every chunk whose entry is not its own id is copied from the chunk the entry names.  It is tolerant: an entry that is not
 * smaller than the chunk's id, or whose source has another length, is skipped, so nothing is read or written outside the segments
 * whatever d_src holds (an entry that names a chunk which is itself copied gives that chunk's bytes of before or after its copy).
 * Any byte alignment of the segments; the calls only enqueue on `stream`.  A bad argument (a null pointer with work to do, d_src
 * not 4-byte or d_work not 16-byte aligned, a work space too small, a maxLen above GLC_DEDUP_MAX_LEN, a count above
 * GLC_DEDUP_MAX_COUNT, more than 2^30 chunks in all) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written; glcDedupWorkBytes
 * returns 0 for such sizes. */
#define GLC_DEDUP_MAX_LEN ((size_t)1 << 20)
#define GLC_DEDUP_MAX_COUNT ((size_t)1 << 22)
size_t glcDedupWorkBytes(size_t count, size_t maxLen);
CUDPPResult glcDedupMapSegments(const void *d_base, const unsigned long long *d_offsets, const unsigned long long *d_lengths, size_t count,
                                size_t maxLen, unsigned int *d_src, void *d_work, size_t workBytes, void *stream);
CUDPPResult glcDedupFillSegments(void *d_outBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths, size_t count,
                                 size_t maxLen, const unsigned int *d_src, void *stream);

/* The two passes of the runs mode as batched calls (csrc/zrun.hip; the split is defined in INTEGRATION.md 4b).  Segment i is
 * x = [d_offsets[i], + n) of its base, n = min(d_lengths[i], maxLen), cut into tiles of 256 bytes.  Position p is a run start
 * when x[p] = 0 and (p % 256 = 0 or x[p - 1] != 0).  A is x at the positions that are non-zero or run starts, in order; B has one
 * byte per run start: the zeros from there up to the next non-zero byte, tile edge or n, minus one.  Split writes A and B of
 * segment i at d_offsets[i] of their bases (at most n bytes each) and their byte counts to d_aLen[i] and d_bLen[i].  Join walks A:
 * a non-zero byte is copied, the z-th zero becomes B[z] + 1 zeros; it writes n bytes at d_outBase + d_offsets[i].  It is
 * tolerant: it does not ask for the tile rule, a zero of A beyond d_bLen[i] is a run of one, output beyond n is dropped and the
 * rest of a short output is zeros, so it never reads outside A or B and never writes outside the segment.  Any length up to
 * GLC_ZERORUN_MAX_LEN, any byte alignment, out of place; the calls only enqueue on `stream`.  A bad argument (a null pointer with
 * count > 0, two equal bases, a maxLen or count too large) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_ZERORUN_MAX_LEN ((size_t)1 << 20)
CUDPPResult glcZeroRunSplitSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                    size_t count, size_t maxLen, void *d_aBase, void *d_bBase, unsigned long long *d_aLen,
                                    unsigned long long *d_bLen, void *stream);
CUDPPResult glcZeroRunJoinSegments(const void *d_aBase, const void *d_bBase, const unsigned long long *d_offsets,
                                   const unsigned long long *d_aLen, const unsigned long long *d_bLen, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, void *d_outBase, void *stream);

/* The rANS coder of the order-0 codec's rANS mode as batched calls (csrc/ans.hip; the record is INTEGRATION.md 4b's kind 5).  Segment
 * i is [d_offsets[i], + min(d_lengths[i], maxLen)) of its base, at most GLC_ANS_MAX_LEN bytes at any byte alignment, cut into chunks
 * of 32768 bytes that 64 interleaved states code.  Encode writes row i of d_hist (256 byte counts), the record at d_recBase +
 * d_recOffsets[i] WORDS (the caller leaves glcAnsBoundWords(length) words of room: chunk unit counts, then every chunk's 64 states
 * and its 16-bit units) and its size to d_recWords[i].  Decode takes the counts, the records and their sizes and writes the
 * segments; it is tolerant -- whatever a record or d_recWords holds, nothing is read outside [record, + d_recWords[i]) and nothing
 * written outside the segment; a segment whose counts are not its own decodes to garbage.  d_work: glcAnsSegmentsWorkBytes(count,
 * maxLen) bytes of device memory for the duration of the call's work (the tables, 6 KiB a segment; the encoder's chunk slots,
 * 64 KiB per chunk of maxLen per segment); the calls only enqueue on `stream`.  A bad argument (a null pointer with count > 0, equal
 * data and record bases, records or counts not 4-byte aligned, a work space too small, a maxLen or count too large) is
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written; the two size functions return 0 for such a maxLen or count. */
#define GLC_ANS_MAX_LEN ((size_t)1 << 20)
#define GLC_ANS_MAX_COUNT ((size_t)1 << 22)
size_t glcAnsBoundWords(size_t len);
size_t glcAnsSegmentsWorkBytes(size_t count, size_t maxLen);
CUDPPResult glcAnsEncodeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, unsigned int *d_hist, unsigned int *d_recBase,
                                 const unsigned long long *d_recOffsets, unsigned long long *d_recWords, void *d_work, size_t workBytes,
                                 void *stream);
CUDPPResult glcAnsDecodeSegments(const unsigned int *d_recBase, const unsigned long long *d_recOffsets, const unsigned long long *d_recWords,
                                 const unsigned int *d_hist, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, void *d_outBase, void *d_work, size_t workBytes, void *stream);

/* The element size the container ENCODER of this plan shuffles by: 0 or 1 = off (the default), 2, 4, 8; anything else is
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leaves the setting as it was.  All six container entry points honour it; the decoder
 * ignores it (the stream header says what was done).  The first filtered call allocates device staging of one frame (rows * n
 * bytes; two with pipelining on), the first filtered decode staging of the largest frame seen; both live as long as the plan. */
CUDPPResult glcPlanSetContainerShuffle(CUDPPHandle plan, unsigned int elem);
CUDPPResult glcPlanGetContainerShuffle(CUDPPHandle plan, unsigned int *elem);

/* The delta mode of the ENCODER's filter: on = 1 stages every frame through delta + shuffle instead of the shuffle and writes
 * format version 4 (flags = 1), with either codec; 0 (the default) writes versions 1 to 3 byte for byte as ever.  on = 1 while
 * the plan's shuffle is off, and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was.
 * glcPlanSetContainerShuffle(plan, 0 or 1) also switches the delta off; a change among 2, 4 and 8 keeps it.  The decoder
 * ignores the setting and reads every version. */
CUDPPResult glcPlanSetContainerDelta(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerDelta(CUDPPHandle plan, unsigned int *on);

/* The codec the container ENCODER of this plan uses.  GLC_CONTAINER_CODEC_BWT (the default) writes format version 1, or 2 with
 * the shuffle filter on, byte for byte as ever.  GLC_CONTAINER_CODEC_HUFF0 writes version 3: a block is an order-0 Huffman
 * record (its histogram in the tables, the table rebuilt from it) or, when 4 * words >= block bytes, raw.  Any other value is
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leaves the setting as it was.  All six container entry points honour it, with
 * pipelining on or off; the decoder ignores it (the stream says what was done) and reads every version.  The first HUFF0
 * encode allocates about 3 KiB of device scratch per row, the first version-3 decode 4 KiB per block of the largest frame plus
 * up to 256 MiB of span-function prefixes; both live as long as the plan, and a plan that only uses the BWT codec has neither.
 * The order-0 path never touches the sorter's scratch or statistics.
 *
 * GLC_CONTAINER_CODEC_CHOOSE (value 4: 2 and 3 stay refused, the values callers have used to see a bad codec refused) picks one of
 * the two per block ("choose"; csrc/choose_rule.h).  What is one frame
 * with the other codecs -- up to `rows` blocks, the ragged tail on its own -- is probed first (glcBigramProbeSegments below), its
 * stats rows are read back in one copy and one wait, and a block goes to the BWT codec exactly when it has at least 2048 bytes,
 * SR > 0, SC > 0 and 2 * S2 * M * (M - 1) >= 3 * SR * SC (128-bit integers); every other block goes to the order-0 codec.  Each
 * maximal run of blocks of one choice becomes one frame, written by that codec's own path, so a stream holds frames of any
 * nb <= rows with kinds 0 and 1, or 2 and 1.  That is format version 3 as readers have accepted it since it exists: there is no
 * new version, and any plan, a default one included, decodes, indexes and range-reads the stream.  The statistic sees local
 * dependence only: a block that repeats a far-away region of noise stays order-0 (or raw).  CHOOSE needs the filter and every
 * mode off: it is refused while the shuffle is on and otherwise clears the mode as every codec change does, and
 * glcPlanSetContainerShuffle(plan, 2, 4 or 8) and every mode setter with on = 1 are refused while it is the codec (composing it
 * with them is left open: a filter is per frame, a mode belongs to one codec).  All six container entry points honour it, with
 * pipelining on or off, with the same bytes.  It allocates what both codecs allocate, 32 bytes per row for the probe, and for
 * the host forms rows * (one block's worst frame) of output staging.  On one MI355X, 1 GiB in 1 MiB blocks, rows 512
 * (profiles/choose_mode.md; ratio / encode / decode GB/s): text and Zipf bytes half and half in runs of 64 blocks 1.899 / 33.4 /
 * 26.0 against BWT 1.723 / 35.8 / 41.5 and order-0 1.521 / 450.5 / 100.3 (BWT frames of 64 blocks decode slower than frames of
 * 512); Zipf bytes alone the order-0 bytes at 291.7 GB/s against 434.9; text alone the BWT bytes at 24.1 against 25.0; the probe
 * alone 1178 to 1199 GB/s. */
enum GlcContainerCodec
{
    GLC_CONTAINER_CODEC_BWT = 0,
    GLC_CONTAINER_CODEC_HUFF0 = 1,
    GLC_CONTAINER_CODEC_CHOOSE = 4                              /* (2 and 3 stay refused values, as callers have long relied on) */
};
CUDPPResult glcPlanSetContainerCodec(CUDPPHandle plan, unsigned int codec);
CUDPPResult glcPlanGetContainerCodec(CUDPPHandle plan, unsigned int *codec);

/* The sparse mode of the ENCODER's order-0 codec: on = 1 writes format version 5, where a block whose most frequent byte fills
 * at least one 64-byte chunk in 32 becomes a sparse record (kind 3: fill byte, chunk mask, the order-0 stream of the kept
 * chunks) and every other block an order-0 or raw record as in version 3 / 4; 0 (the default) writes versions 1 to 4 byte for
 * byte as ever.  on = 1 while the plan's codec is not GLC_CONTAINER_CODEC_HUFF0, and any other value, are
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; glcPlanSetContainerCodec(plan, GLC_CONTAINER_CODEC_BWT) also
 * switches it off.  All six container entry points honour it, with pipelining on or off and with any filter setting.  The setting
 * is also the version the plan speaks: a plan with it on reads versions 1 to 5, a plan with it off is a version-4 reader to which a
 * version-5 stream is a stream-header failure, as it was before version 5 existed (so a reader of sparse streams sets the
 * HUFF0 codec and the mode on; its other settings stay ignored).  The first sparse encode allocates rows * n bytes of compaction space and the masks, the
 * first version-5 decode as much for the blocks of one decoder chunk; both are kept with the plan and freed with it. */
CUDPPResult glcPlanSetContainerSparse(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerSparse(CUDPPHandle plan, unsigned int *on);

/* Range reads: bytes [offset, offset + count) of the original input out of a container, decoding only the blocks they need.
 * No format change: every frame header gives the size of its frame, so a walk over the headers alone -- 32 bytes per frame --
 * yields a FRAME INDEX: per frame its position in the stream, nb, blk_len, payload words and the output offset of its first byte,
 * with copies of the stream header and the trailer.  The index is an opaque host object, built once per container and freed with
 * glcContainerIndexFree (NULL is fine).  Building it makes exactly the checks the full decode makes before it touches a frame's
 * tables -- stream header (a plan with the sparse mode off is a version-4 reader), every frame header's range check, truncation,
 * the trailer and stray bytes behind it, a plan whose n is below the blocks' length -- and fails with the same result and the same
 * glcContainerLastError triple as glcContainerDecompress* on the same bytes; table CRCs, table fields and records are left to
 * reading.  An empty input's container gives an index of zero frames.  The host and file forms fetch the headers and nothing else
 * (the file form by pread); the device form walks the chain on the GPU in one launch (d_in 8-byte aligned) and reads the result
 * back once, twice for a container of more than 1022 frames.
 *
 * A read takes the index and the container it was built from (`len`, and the stream header now at position 0, must be the
 * index's: a different len is CUDPP_ERROR_ILLEGAL_CONFIGURATION, a different header CUDPP_ERROR_UNKNOWN with
 * {GLC_CONTAINER_STREAM_HEADER, ~0, ~0}).  count == 0 succeeds and writes nothing; offset + count beyond the input's length and a
 * NULL index are CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written.  d_out / out receive exactly `count` bytes, at any
 * alignment, and the call returns with them complete.
 * WHAT A RANGE READ CHECKS.  A frame the range does not overlap is not read at all.  A frame it overlaps is fetched whole and gets
 * the full decode's checks in the full decode's order -- the header's range check (it must still say what the index says), the
 * table CRC, every field check, the CRC of EVERY record of the frame -- with the same failure triples; then only the blocks the
 * range needs are decoded, each checked against its CRC in the tables.  With a filter of element size e over a frame of F bytes,
 * q = F / e, the needed blocks of bytes [a, b) of the frame are those that hold a byte of one of the e plane runs [j q + i0,
 * j q + i1), i0 = a / e (rounded down to a multiple of 2048 with the delta on), i1 = min(q, ceil(b / e)), and those of the last
 * F % e bytes when b reaches into them; without a filter the blocks that intersect [a, b).
 * WHAT IT DOES NOT CHECK.  The trailer's crc_all is the CRC of the whole input and cannot be checked by a partial read; frames
 * outside the range are not looked at, so damage there goes unnoticed until a read that touches it.
 * The host and file forms keep host and device memory proportional to one frame.  A range read decodes into the plan's frame
 * staging (one frame, allocated on the first read and kept with the plan), a filtered one also into the second staging.
 * glcContainerLastRangeStats: for the plan's last successful range read, {frames fetched, blocks decoded, container bytes fetched
 * (the 32-byte stream header and the frames)}.  Measured on one MI355X on 1 GiB in 1 MiB blocks, rows 512, so two frames
 * (tools/bench_range.py, profiles/range_read.md; medians): a read inside one frame costs the frame's checks whatever its size --
 * BWT codec 2.2 ms for 4 KiB or 1 MiB and 3.8 ms for 64 MiB against 25.5 ms for the full decode; int64 timestamps with the order-0
 * codec, delta + shuffle 8 and the sparse mode 2.1-2.4 ms and 2.6 ms against 6.2 ms -- a read across the frame edge twice that, and
 * the index of the device container 0.07 ms. */
typedef struct GlcContainerIndex GlcContainerIndex;
CUDPPResult glcContainerIndexDevice(CUDPPHandle plan, const void *d_in, unsigned long long len, GlcContainerIndex **index);
CUDPPResult glcContainerIndex(CUDPPHandle plan, const void *in, unsigned long long len, GlcContainerIndex **index);
CUDPPResult glcContainerIndexFile(CUDPPHandle plan, const char *path, GlcContainerIndex **index);
void glcContainerIndexFree(GlcContainerIndex *index);
/* out: total_len, block_len, frame count, version | flags << 16 | elem << 32 */
CUDPPResult glcContainerIndexInfo(const GlcContainerIndex *index, unsigned long long out[4]);
/* the plane stride the stream header's word 7 holds: 0 but of a version-17 stream (glcPlanSetContainerDeltaVolume) */
CUDPPResult glcContainerIndexPlane(const GlcContainerIndex *index, unsigned int *plane);
CUDPPResult glcContainerReadRangeDevice(CUDPPHandle plan, const GlcContainerIndex *index, const void *d_in, unsigned long long len,
                                        unsigned long long offset, unsigned long long count, void *d_out);
CUDPPResult glcContainerReadRange(CUDPPHandle plan, const GlcContainerIndex *index, const void *in, unsigned long long len,
                                  unsigned long long offset, unsigned long long count, void *out);
CUDPPResult glcContainerReadRangeFile(CUDPPHandle plan, const GlcContainerIndex *index, const char *path, unsigned long long offset,
                                      unsigned long long count, void *out);
CUDPPResult glcContainerLastRangeStats(CUDPPHandle plan, unsigned long long out[3]);

/* Range forms of the two inverse filters, queued on `stream`: d_in is a filtered segment of `len` bytes (plane stride q = len /
 * elem); d_out receives count * elem bytes, elements first .. first + count - 1 as glcUnshuffleDevice / glcUndeltaUnshuffleDevice
 * over the whole segment would have produced them.  first + count <= q; the delta form wants `first` a multiple of 2048 (a run
 * start); any other `first`, any count and any byte alignment of either buffer are fine.  Only the aligned 16-byte granules that
 * hold a byte of one of the elem plane runs [j q + first, + count) are read, and exactly the output bytes are written.  elem 2, 4
 * or 8; a bad elem, a range past q, a delta `first` off a run start, a NULL buffer and an output that overlaps the segment are
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
CUDPPResult glcUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem, unsigned long long first,
                                    unsigned long long count, void *stream);
CUDPPResult glcUndeltaUnshuffleRangeDevice(const void *d_in, void *d_out, unsigned long long len, unsigned int elem,
                                           unsigned long long first, unsigned long long count, void *stream);

/* The runs mode of the ENCODER's BWT codec: on = 1 writes format version 6, where every block is a zero-run record (kind 4: the
 * BWT index, the byte counts of A, the non-zero counts of B, the order-0 streams of A and B) or, when 4 * words >= block bytes,
 * raw; 0 (the default) writes versions 1 to 5 byte for byte as ever.  on = 1 while the plan's codec is not
 * GLC_CONTAINER_CODEC_BWT, and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; setting
 * the codec to GLC_CONTAINER_CODEC_HUFF0 also switches it off.  All six container entry points and the range reads honour it,
 * with pipelining on or off (a runs frame is queued on the plan's stream alone) and with any filter setting.  The setting is also
 * the version the plan speaks: a plan with it on reads versions 1 to 4 and 6, every other plan refuses version 6 as a
 * stream-header failure, as it was before version 6 existed.  Version 5 needs the sparse mode and with it the other codec, so no
 * single plan reads both 5 and 6.  The first runs encode allocates 2 * rows * n bytes for A and B, the first version-6 decode as
 * much for the blocks of one decoder chunk plus the BWT decoder's scratch; both are kept with the plan and freed with it. */
CUDPPResult glcPlanSetContainerRuns(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerRuns(CUDPPHandle plan, unsigned int *on);

/* The rANS mode of the ENCODER's order-0 codec: on = 1 writes format version 7, where every block is an rANS record (kind 5: the
 * block's byte counts in the tables, the 12-bit probabilities derived from them, and per chunk of 32768 bytes 64 interleaved
 * 32-bit states with their 16-bit units) or, when 4 * words >= block bytes, raw; 0 (the default) writes versions 1 to 6 byte for
 * byte as ever.  A Huffman code spends at least one bit per byte; this coder spends log2(4096 / q) bits on a symbol of quantised
 * probability q / 4096, so scattered skew (quantised gradients, delta'd planes of 0 and +-1) that no fill-byte chunk and no table
 * can shorten codes below one bit.  on = 1 needs the codec GLC_CONTAINER_CODEC_HUFF0 and the sparse mode off: on = 1 without them,
 * and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; glcPlanSetContainerCodec(plan,
 * GLC_CONTAINER_CODEC_BWT) also switches it off, and glcPlanSetContainerSparse(plan, 1) is refused while it is on.  All six
 * container entry points and the range reads honour it, with pipelining on or off and with any filter setting.  The setting is
 * also the version the plan speaks: a plan with it on reads versions 1 to 4 and 7, every other plan refuses a version-7 stream as
 * a stream-header failure, as it did before version 7 existed.  The first rANS encode allocates about 2 * rows * n bytes of chunk
 * slots and 6 KiB of tables per row, the first version-7 decode 6 KiB of tables per block of one decoder chunk beside what a
 * version-3 decode allocates (a version-7 frame may hold kind 2); the kind-5 blocks themselves use the tables alone -- a chunk starts
 * from stored states, so one wave decodes it straight through and no span-function prefixes are computed.  Both are kept with the
 * plan and freed with it.  The new kernels have no slot in the plan's kernel profile. */
CUDPPResult glcPlanSetContainerAns(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerAns(CUDPPHandle plan, unsigned int *on);

/* The probe of the auto mode as a batched call (csrc/auto.hip).  Segment i is [d_offsets[i], + min(d_lengths[i], maxLen)) of its
 * base, at most GLC_PROBE_MAX_LEN bytes at any byte alignment.  One pass over it writes row i of d_hist, its 256 byte counts, and
 * row i of d_uniform: d_uniform[256 i + v] is the number of its 64-byte chunks -- cut from the segment's start, not by address;
 * the last may be short -- whose bytes all equal v.  The rows (256 words each) need not be zeroed by the caller.  The call only
 * enqueues on `stream`.  A bad argument (a null pointer with count > 0, rows not 4-byte aligned, the two row arrays equal, a
 * maxLen or count too large) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_PROBE_MAX_LEN ((size_t)1 << 20)
#define GLC_PROBE_MAX_COUNT ((size_t)1 << 22)
CUDPPResult glcProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                             size_t count, size_t maxLen, unsigned int *d_hist, unsigned int *d_uniform, void *stream);

/* The bigram probe of GLC_CONTAINER_CODEC_CHOOSE as a batched call (csrc/choose.hip).  The segments are those of glcProbeSegments.
 * For 2 <= p < L the key of position p of a segment x of L bytes is the context (31 * x[p-2] + x[p-1]) & 255 and the symbol
 * x[p]; N[a][b] counts the positions with context a and symbol b, R[a] and C[b] are its row and column sums.  Row i of d_stats is
 * four 64-bit words {S2, SR, SC, M}: the sums of N (N - 1), R (R - 1) and C (C - 1), and the number of positions M = L - 2 (0 for
 * L < 2), all exact.  S2 * M * (M - 1) / (SR * SC) is 1 for i.i.d. bytes at any length and grows with the dependence of a byte
 * on the two before it.  Every row is written whole.  The call only enqueues on `stream`.  A bad argument (a null pointer with
 * count > 0, rows not 8-byte aligned, a maxLen or count too large) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
CUDPPResult glcBigramProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, unsigned long long *d_stats, void *stream);

/* The filter probe as a batched call (csrc/filter_probe.hip, csrc/filter_rule.h): which byte-plane filter -- element size 2, 4 or 8,
 * with or without the delta of glcDeltaShuffleDevice, or none -- a segment wants, from one read of it.  The segments are those of
 * glcProbeSegments, but up to GLC_FILTER_PROBE_MAX_LEN bytes each; with L = min(d_lengths[i], maxLen) only the first P = L - L % 8
 * bytes x[0 .. P) of segment i are counted.  Row i of d_planes is 22 histograms of 256 words (GLC_FILTER_PROBE_ROWS):
 *   rows 0..7    A_k[v]: the positions p < P with p % 8 == k and x[p] == v.  Plane j of the plain shuffle over elements of e bytes
 *                is the sum of the A_k with k = j modulo e; the unfiltered bytes are the sum of all eight;
 *   rows 8..9    D_2[j][v], rows 10..13 D_4[j][v], rows 14..21 D_8[j][v]: the elements i < P / e whose delta d_e[i] has byte j equal to
 *                v, with d_e[i] = x_e[i] where i % 2048 == 0 and x_e[i] - x_e[i-1] modulo 2^(8 e) elsewhere, elements little-endian and
 *                counted from the segment's start: the planes glcDeltaShuffleDevice makes of these bytes.
 * Row i of d_costs is seven 64-bit words, the costs of the candidates (elem, delta) = (1,0) (2,0) (2,1) (4,0) (4,1) (8,0) (8,1) in
 * this order, (1,0) being no filter: the sum over the candidate's planes of sum_s H[s] * cost(q(s)) with H the plane's counts, N their
 * sum, q(s) = clamp(floor(H[s] * 4096 / N), 1, 4096) and cost(q) = 12 - log2 q in 1/256 bit rounded up (the table of the auto mode,
 * csrc/auto_rule.h) -- exact integers below 2^43.  The rule that reads them (csrc/filter_rule.h) walks the candidates in order from
 * pick = 0 and lets candidate i replace the pick exactly when 33 * cost[i] < 32 * cost[pick]: more planes never raise an empirical
 * entropy, so a later candidate has to win by a margin.  The rows need not be zeroed by the caller.  The call only enqueues on
 * `stream`.  A bad argument (a null pointer with count > 0, d_planes not 16-byte or d_costs not 8-byte aligned, the two equal, a
 * maxLen or count too large) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_FILTER_PROBE_MAX_LEN ((size_t)1 << 31)
#define GLC_FILTER_PROBE_ROWS 22
#define GLC_FILTER_CANDIDATES 7
CUDPPResult glcFilterProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                   size_t count, size_t maxLen, unsigned int *d_planes, unsigned long long *d_costs, void *stream);

/* The lag probe as two batched calls (csrc/lag_probe.hip, csrc/lag_rule.h): which lag of glcLagDeltaShuffleDevice's lagged, folded
 * delta a segment wants at each element size, and what the planes of that filter would cost.  The segments are those of
 * glcFilterProbeSegments: with L = min(d_lengths[i], maxLen) only the first P = L - L % 8 bytes of segment i are counted.  With
 * x_e[i] the elements of e = 2, 4 or 8 bytes and f_{e,l}[i] the folded difference at lag l = 1 .. 16 -- d = x_e[i] where
 * i % 2048 < l, else x_e[i] - x_e[i - l] modulo 2^(8 e); f = (d << 1) ^ (0 - (d >> (8 e - 1))), run heads included: what
 * glcLagDeltaShuffleDevice(e, l, fold = 1) builds its planes from --
 *   glcLagProbeSegments   row i of d_sums is 48 64-bit words (GLC_LAG_PROBE_SUMS), S[e][l] = sum_i bitlen(f_{e,l}[i]) at word
 *                         (log2 e - 1) * 16 + (l - 1), bitlen(0) = 0 and bitlen(v) = floor(log2 v) + 1, exact; row i of d_lags is
 *                         three words, for e = 2, 4 and 8 the l with the smallest sum, ties to the smallest l (P = 0: 1, 1, 1).
 *   glcLagPlanesSegments  row i of d_planes is 14 histograms of 256 words (GLC_LAG_PROBE_ROWS): rows 0..1 E_2[j][v], rows 2..5
 *                         E_4[j][v], rows 6..13 E_8[j][v] = the elements whose f_{e,l_e}[i] has byte j equal to v, with l_e read from
 *                         row i of d_lags in device memory and used as ((word - 1) & 15) + 1; row i of d_costs is three 64-bit
 *                         words, the cost of glcFilterProbeSegments summed over the planes of E_2, of E_4 and of E_8.
 * The second call takes the first's d_lags without the host between them.  The rule that reads the costs (csrc/lag_rule.h) is
 * glcFilterProbeSegments' walk over ten candidates: its seven, then (2, l_2), (4, l_4) and (8, l_8) with the fold, under the same
 * margin.  No output need be zeroed by the caller.  Both calls only enqueue on `stream`.  A bad argument (a null pointer with
 * count > 0, d_sums or d_costs not 8-byte or d_planes not 16-byte aligned, two of a call's arrays equal, a maxLen above
 * GLC_FILTER_PROBE_MAX_LEN or a count above GLC_PROBE_MAX_COUNT) is CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_LAG_PROBE_SUMS 48
#define GLC_LAG_PROBE_ROWS 14
CUDPPResult glcLagProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                size_t count, size_t maxLen, unsigned long long *d_sums, unsigned int *d_lags, void *stream);
CUDPPResult glcLagPlanesSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, const unsigned int *d_lags, unsigned int *d_planes,
                                 unsigned long long *d_costs, void *stream);

/* The grid probe as two batched calls (csrc/grid_probe.hip, csrc/grid_rule.h): which row width of glcGridDeltaShuffleDevice's 2-D
 * predictor a segment wants at each element size, and what the planes of that filter would cost.  The segments are those of
 * glcFilterProbeSegments: with L = min(d_lengths[i], maxLen) only the first P = L - L % 8 bytes of segment i are counted.  With
 * x_e[i] the N = P / e elements of e = 2, 4 or 8 bytes: an element size with N < 1024 has no candidate.  Otherwise
 * Wmax = min(65536, N / 2), and the sample is 32 tiles of 256 target elements at b_t = Wmax + floor(t (N - Wmax - 256) / 31) --
 *   glcGridProbeSegments   row i of d_sums is 3 * 65537 32-bit words (GLC_GRID_PROBE_SUMS): at word k * 65537 + W, k = log2 e - 1,
 *                          S_e[W] = sum over t and j < 256 of bitlen(fold(x_e[b_t + j] - x_e[b_t + j - W])) for W = 2 .. Wmax, the
 *                          difference modulo 2^(8 e), fold and bitlen those of glcLagProbeSegments, exact; 0xFFFFFFFF at W < 2, at
 *                          W > Wmax and where there is no candidate.  Row i of d_widths is three words, for e = 2, 4 and 8 the W
 *                          with the smallest sum, ties to the smallest W, or 0 where there is no candidate.
 *   glcGridPlanesSegments  row i of d_planes is 14 histograms of 256 words in glcLagPlanesSegments' layout, over the bytes of what
 *                          glcGridDeltaShuffleDevice(e, w_e, fold = 1) builds from the counted bytes, bands and run heads
 *                          included, with w_e read from row i of d_widths in device memory; row i of d_costs is three 64-bit words,
 *                          the cost of glcFilterProbeSegments summed over the planes of e.  A width word outside 2..65536 names no
 *                          width: its rows are zero, its cost is 2^56 (which the rule never picks), and it is never used as a
 *                          distance.
 * The second call takes the first's d_widths without the host between them.  The rule that reads the costs (csrc/grid_rule.h) is
 * glcLagProbeSegments' walk over thirteen candidates: its ten, then the grid filter at (2, w_2), (4, w_4) and (8, w_8) with the
 * fold, under the same margin.  The first call costs the same for every segment length: about 1.6e9 (target, width) pairs where
 * all three element sizes reach Wmax = 65536.  No output need be zeroed by the caller.  Both calls only enqueue on `stream`.  A
 * bad argument (a null pointer with count > 0, d_sums or d_widths not 4-byte, d_costs not 8-byte or d_planes not 16-byte aligned,
 * two of a call's arrays equal, a maxLen above GLC_FILTER_PROBE_MAX_LEN or a count above GLC_PROBE_MAX_COUNT) is
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_GRID_PROBE_SUMS (3 * 65537)
CUDPPResult glcGridProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, unsigned int *d_sums, unsigned int *d_widths, void *stream);
CUDPPResult glcGridPlanesSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                  size_t count, size_t maxLen, const unsigned int *d_widths, unsigned int *d_planes,
                                  unsigned long long *d_costs, void *stream);

/* The byte probe as two batched calls (csrc/byte_probe.hip, csrc/byte_rule.h): which lag and which row stride of glcByteDeltaDevice's
 * byte predictor a segment wants, and what its output would cost.  The segments are those of glcFilterProbeSegments: with
 * L = min(d_lengths[i], maxLen) only the first P = L - L % 8 bytes x[j] of segment i are counted.
 *   glcByteProbeSegments   row i of d_lagSums is sixteen 64-bit words: at word l - 1 the sum over j < P of m((x[j] - p) mod 256)
 *                          for the lag l = 1 .. 16, p = x[j - l] where j mod 2048 >= l and 0 elsewhere, m(d) = d below 128 and
 *                          255 - d otherwise, exact.  Row i of d_strideSums is 65537 32-bit words (GLC_BYTE_PROBE_ROW): with
 *                          P >= 1024, Wmax = min(65536, P / 2) and glcGridProbeSegments' 32 tiles of 256 targets at element size 1,
 *                          at word W the sum of bitlen(fold((x[j] - x[j - W]) mod 256)) for W = 17 .. Wmax; 0xFFFFFFFF at every
 *                          other word.  Row i of d_winners is two words: the lag with the smallest sum and the stride with the
 *                          smallest sum, ties to the smallest, the stride 0 where P < 1024.
 *   glcBytePlanesSegments  row i of d_planes is two histograms of 256 words: of the bytes glcByteDeltaDevice(lag, 0) and of the
 *                          bytes glcByteDeltaDevice(lag, stride) write from the counted bytes, bands and run heads included,
 *                          with {lag, stride} read from row i of d_words in device memory; row i of d_costs is two 64-bit words,
 *                          the cost of glcFilterProbeSegments of each histogram.  The lag word is used as ((v - 1) & 15) + 1.  A
 *                          stride word outside 17..65536 names no stride: its row is zero, its cost is 2^56 (which the rule never
 *                          picks), and it is never used as a distance.  With P < 1024 both rows are zero and both costs 2^56.
 * The second call takes the first's d_winners without the host between them.  The rule that reads the costs (csrc/byte_rule.h) is
 * glcGridProbeSegments' walk over fifteen candidates: its thirteen, then the byte predictor at (lag, 0) and at (lag, stride), under
 * the same margin.  No output need be zeroed by the caller.  Both calls only enqueue on `stream`.  A bad argument (a null pointer
 * with count > 0, d_strideSums, d_winners or d_words not 4-byte, d_lagSums or d_costs not 8-byte or d_planes not 16-byte aligned, two
 * of a call's arrays equal, a maxLen above GLC_FILTER_PROBE_MAX_LEN or a count above GLC_PROBE_MAX_COUNT) is
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION with nothing written. */
#define GLC_BYTE_PROBE_ROW 65537
CUDPPResult glcByteProbeSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                 size_t count, size_t maxLen, unsigned long long *d_lagSums, unsigned int *d_strideSums,
                                 unsigned int *d_winners, void *stream);
CUDPPResult glcBytePlanesSegments(const void *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                                  size_t count, size_t maxLen, const unsigned int *d_words, unsigned int *d_planes,
                                  unsigned long long *d_costs, void *stream);

/* {blocks given to the BWT codec, blocks given to the order-0 codec, frames written} of the plan's last successful container
 * compress, whatever its codec; with GLC_CONTAINER_CODEC_CHOOSE the first two are the rule's choices, counted before the record
 * rule stores a block raw.  {0, 0, 0} before the first. */
CUDPPResult glcContainerLastChoice(CUDPPHandle plan, unsigned long long out[3]);

/* The auto mode of the ENCODER's order-0 codec: on = 1 writes format version 8, whose frames may hold kinds 0, 1, 2, 3 and 5 in any
 * mix (not 4), and picks a kind per block from the block's statistics alone ("the auto mode's rule").  One probe
 * pass gives every block's byte counts H and, per byte value, its 64-byte chunks of that byte alone.  Candidate S is what the sparse
 * mode's writer would make (kind 3, 2 or 1) and wS its exact words, known from the counts and the Huffman tables' code lengths;
 * candidate A is kind 5 and wA = 65 * ceil(n / 32768) + ceil(sum H[s] * (12 - log2 q[s]) / 32) an estimate of its words, with the
 * logarithm in 1/256 bit rounded up by exact integer arithmetic (csrc/auto_rule.h).  The block is coded as kind 5 when wA < wS and
 * then falls under kind 5's raw rule on its actual words; otherwise it is candidate S.  Every record and every reader check is
 * that of the version that introduced its kind.  The mask and compaction passes then run on the kind-3 blocks only, the rANS
 * coder on the kind-5 blocks only, the Huffman encoder on kind 2 and on the kept bytes of kind 3.  0 (the default) writes versions
 * 1 to 7 byte for byte as ever.  on = 1 needs the codec GLC_CONTAINER_CODEC_HUFF0 with the sparse and the rANS mode off: on = 1
 * without that, and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was;
 * glcPlanSetContainerCodec(plan, GLC_CONTAINER_CODEC_BWT) also switches it off, and glcPlanSetContainerSparse(plan, 1) and
 * glcPlanSetContainerAns(plan, 1) are refused while it is on.  All six container entry points, the index and the range reads
 * honour it, with pipelining on or off and with any filter setting.  The setting is also the version the plan speaks: a plan with
 * it on reads versions 1 to 5, 7 and 8 -- everything the order-0 codec has ever written -- and refuses version 6; every other
 * plan refuses a version-8 stream as a stream-header failure, as it did before version 8 existed.  The first auto encode allocates
 * the scratch of the sparse and of the rANS mode together -- about 3 * rows * n bytes (rows * n of compaction space, 2 * rows * n
 * of chunk slots) plus the masks and 6 KiB of rANS tables and 2 KiB of probe counts per row -- and the first version-8 decode what
 * a version-5 and a version-7 decode allocate; both are kept with the plan and freed with it.  The new kernels have no slot in the
 * plan's kernel profile. */
CUDPPResult glcPlanSetContainerAuto(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerAuto(CUDPPHandle plan, unsigned int *on);

/* The dedup mode of the ENCODER's order-0 codec: on = 1 writes format version 9, whose frames may hold kinds 0, 1, 2 and 6 (the
 * writer makes 6, 2 or 1).  Every record kind before it looks no further than one block; here a block is cut into chunks of 512
 * bytes and a chunk that repeats an EARLIER chunk of the same frame -- up to rows * n bytes away -- is elided: the record (kind 6)
 * holds a chunk mask, one 32-bit source id per elided chunk and the order-0 stream of the kept chunks ("dedup";
 * the passes are glcDedupMapSegments and glcDedupFillSegments above).  The writer's rule is deterministic: a 64-bit hash per chunk,
 * the smallest chunk id of the frame with that hash as the candidate, a byte compare, so a source is always a kept chunk and one
 * copy pass behind the blocks' decoders completes a frame.  A block with E elided chunks becomes kind 6 when 15 * E >= its mask
 * words (then the record cannot be longer than the block's kind-2 record) and kind 2 otherwise, raw under the record rule either
 * way.  It is for page- or sector-aligned repeats (snapshots, images, archives that hold a file twice, tied tensors); it finds
 * nothing in data whose repeats are not 512-aligned, and a frame of zeros costs 128 : 1 of what the sparse mode makes of it (one
 * ref per chunk).  0 (the default) writes versions 1 to 8 byte for byte as ever.  on = 1 needs the codec
 * GLC_CONTAINER_CODEC_HUFF0 with the sparse, rANS and auto modes off: on = 1 without that, and any other value, are
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; glcPlanSetContainerCodec(plan, GLC_CONTAINER_CODEC_BWT or
 * _CHOOSE) also switches it off, and the three other order-0 mode setters with on = 1 are refused while it is on.  All six container
 * entry points honour it, with pipelining on or off and with any filter setting, with the same bytes.  The setting is also the
 * version the plan speaks: a plan with it on reads versions 1 to 4 and 9; to every other plan, the auto-mode plan included, a
 * version-9 stream is a stream-header failure, as it always was.  A range read of a kind-6 block b also decodes the blocks
 * [bwt_index[b], b) of its frame as sources (decoded, not compared with their own crc_raw; the block's own crc_raw covers what was
 * copied); glcContainerLastRangeStats counts them among the blocks decoded.  The first dedup encode allocates, beside the sparse
 * mode's rows * n bytes of compaction space, a hash table of 16 bytes a slot with at least two slots per chunk of a frame and 16
 * bytes per chunk (about 40 MiB for rows 512, n 1 MiB; one set whether pipelining is on or off, since a dedup frame runs wholly on
 * the plan's stream); the first version-9 decode the compaction space of one decoder chunk and 4
 * bytes per chunk of the largest frame; both are kept with the plan and freed with it. */
CUDPPResult glcPlanSetContainerDedup(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerDedup(CUDPPHandle plan, unsigned int *on);

/* Filter-auto: the ENCODER picks every frame's filter itself.  on = 1 writes format version 10: the stream header's triple is
 * (10, 0, 0), the record kinds are version 8's (0, 1, 2, 3 and 5), and word 3 of every FRAME header (byte 12; 0 in versions 1 to 9)
 * names that frame's filter as elem | flags << 16 -- elem 0, 2, 4 or 8, flags 0 or 1 (the delta), flags 1 only with an elem.  The
 * frame's bytes went through that filter as one segment before its blocks were cut, exactly as a stream-level filter does; crc_raw
 * is of the filtered blocks, crc_all of the original input, table_crc covers the word, frames are cut as ever and tables, records,
 * payload and trailer are unchanged: a version-10 stream has the size of the version-8 stream with the same filters.  Per frame
 * (the ragged tail included) the writer probes the frame in place (glcFilterProbeSegments), reads the seven costs back with one
 * wait -- the one host read per frame, as the CHOOSE codec reads its stats --, applies the rule of csrc/filter_rule.h, stages the
 * frame through the chosen filter (not at all for no filter) and runs the auto mode's frame on it.  A frame longer than
 * GLC_FILTER_PROBE_MAX_LEN is judged by its first 2^31 bytes.  A checkpoint shard, an archive or a column file that holds float32,
 * int64 and text sections behind each other gets each frame's own filter; the sizes are in INTEGRATION.md 4b ("filter: when").
 * 0 (the default) writes versions 1 to 9 byte for byte as ever.  on = 1 needs the codec GLC_CONTAINER_CODEC_HUFF0, the auto mode on
 * and the plan's shuffle off: on = 1 without all three, and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the
 * setting as it was.  While it is on glcPlanSetContainerShuffle(plan, 2, 4 or 8) is refused; glcPlanSetContainerAuto(plan, 0) and a
 * codec change that ends the auto mode switch it off.  All six container entry points write the same bytes, with pipelining on or
 * off; the index keeps every frame's filter, and range reads use it for the blocks a range needs and for the range inverse filters
 * (the delta's rounding to 2048 elements included); glcContainerIndexInfo's fourth word reports what the stream header says.  The
 * setting is also the version the plan speaks: a plan with it on reads versions 1 to 5, 7, 8 and 10; every other plan refuses a
 * version-10 stream as a stream-header failure.  A frame word that is none of the above is a frame-table failure naming the frame,
 * found by the header's range check before the tables are touched.  Not combined with the BWT codec, the CHOOSE codec or the other
 * order-0 modes; element sizes other than 2, 4 and 8, a sampled probe and a choice per block are not offered. */
CUDPPResult glcPlanSetContainerFilterAuto(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerFilterAuto(CUDPPHandle plan, unsigned int *on);

/* The lag and fold of the ENCODER's delta (glcLagDeltaShuffleDevice), (1, 0) = off, the default.  Anything else needs the order-0
 * codec, the auto mode on, the shuffle at 2, 4 or 8, the delta on and filter-auto off; any other state, a lag outside 1..16 and a
 * fold above 1 are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was.  Whatever ends one of those prerequisites
 * puts it back to (1, 0); a change among elem 2, 4 and 8 keeps it.  The stream is format version 11: version 8's frames, the
 * header's flags 1 | fold << 1 | (lag - 1) << 8.  (1, 0) writes version 8 byte for byte.  Decode, index and range reads take lag and
 * fold from the stream header, never from the plan; glcContainerIndexInfo's fourth word carries the flags.  The setting is also the
 * version the plan speaks: with it on the plan reads versions 1 to 5, 7, 8 and 11; every other plan refuses a version-11 stream as
 * a stream-header failure.  Not combined with filter-auto, the BWT codec, the CHOOSE codec or the other order-0 modes. */
CUDPPResult glcPlanSetContainerDeltaLag(CUDPPHandle plan, unsigned int lag, unsigned int fold);
CUDPPResult glcPlanGetContainerDeltaLag(CUDPPHandle plan, unsigned int *lag, unsigned int *fold);

/* The row width and fold of the ENCODER's 2-D predictor (glcGridDeltaShuffleDevice); width 0 = off, the default.  Any other width
 * needs what glcPlanSetContainerDeltaLag needs -- the order-0 codec, the auto mode on, the shuffle at 2, 4 or 8, the delta on and
 * filter-auto off -- and the delta-lag setting at (1, 0); any other state, a width outside 2..65536 and a fold above 1 are
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was.  While it is on, glcPlanSetContainerDeltaLag with anything but
 * (1, 0) is refused.  Whatever ends one of the prerequisites puts it back to off; a change among elem 2, 4 and 8 keeps it.  The
 * stream is format version 12: version 8's frames, the header's flags 1 | fold << 1 | 4 and its word 3 elem | width << 8.  Decode,
 * index and range reads take width and fold from the stream header, never from the plan; glcContainerIndexInfo's fourth word
 * carries word 3 as it stands.  The setting is also the version the plan speaks: with it on the plan reads versions 1 to 5, 7, 8
 * and 12 (not 11); every other plan refuses a version-12 stream as a stream-header failure.  With it off every stream is written
 * as before. */
CUDPPResult glcPlanSetContainerDeltaGrid(CUDPPHandle plan, unsigned int width, unsigned int fold);
CUDPPResult glcPlanGetContainerDeltaGrid(CUDPPHandle plan, unsigned int *width, unsigned int *fold);

/* Filter-lag: filter-auto also picks the delta's lag per frame.  on = 1 writes format version 13: version 10 whose frame word
 * (word 3 of every frame header, elem | flags << 16) may also carry flags 1 | fold << 1 | (lag - 1) << 8 with elem 2, 4 or 8, the
 * flags of format version 11: that frame went through glcLagDeltaShuffleDevice(elem, lag, fold) as one segment.  The stream
 * header's triple is (13, 0, 0), the kinds are version 8's, frames, tables, records and trailer version 10's; table_crc covers the
 * word as ever.  Per frame the writer enqueues the filter probe and behind it the lag probe (glcLagProbeSegments and
 * glcLagPlanesSegments, the winners staying in device memory between them), reads ten costs and three lags back with the one wait
 * filter-auto has, and walks the ten candidates of csrc/lag_rule.h: filter-auto's seven in their order, then (2, l_2), (4, l_4)
 * and (8, l_8) with the fold, under the same margin.  The writer makes only fold = 1 lag words; the reader takes the whole family,
 * (lag > 1, fold 0) included.  A stream whose every pick is among the first seven differs from the version-10 stream only in the
 * header's version and its CRC.  Interleaved channels -- stereo audio, an 8-channel ADC dump, xyz points -- get their channel
 * count as the lag, and single series the fold, frame by frame ("filter-lag: when").  on = 1 needs filter-auto
 * on: on = 1 without it, and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; whatever
 * switches filter-auto off switches this off.  0 (the default) writes every stream byte for byte as before.  All six container
 * entry points write the same bytes, with pipelining on or off.  Range reads of a lag frame use the delta's rounding to 2048
 * elements and glcUnlagDeltaUnshuffleRangeDevice with the frame's lag and fold.  The setting is also the version the plan speaks:
 * with it on the plan reads versions 1 to 5, 7, 8, 10 and 13; every other plan, a filter-auto plan included, refuses a version-13
 * stream as a stream-header failure.  A lag word under a version-10 header, and any word outside the family above, is a
 * frame-table failure naming the frame.  The 2-D predictor's width is glcPlanSetContainerFilterGrid's; a lag above 16, the
 * unfolded delta at lag > 1 as a candidate of its own and a choice per block are not offered. */
CUDPPResult glcPlanSetContainerFilterLag(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerFilterLag(CUDPPHandle plan, unsigned int *on);

/* Filter-grid: filter-lag also finds the row width of the 2-D predictor per frame.  on = 1 writes format version 14: version 13
 * whose frame word may also name glcGridDeltaShuffleDevice's filter.  A frame word with bit 31 clear is version 13's, unchanged; one
 * with bit 31 set is elem | width << 8 | fold << 30 | 1 << 31 -- format version 12's header word 3 with the fold in bit 30 -- with
 * elem 2, 4 or 8, width 2..65536 and bits 25..29 zero: that frame went through glcGridDeltaShuffleDevice(elem, width, fold) as one
 * segment.  (Under version 13 every word with bit 31 set is illegal, so the two families cannot collide.)  The stream header's
 * triple is (14, 0, 0); kinds, frames, tables, records and trailer are version 13's.  Per frame the writer enqueues the filter
 * probe, the lag probe and the grid probe (glcGridProbeSegments and glcGridPlanesSegments, the widths staying in device memory
 * between them), reads thirteen costs, three lags and three widths back with the one wait filter-auto has, and walks the thirteen
 * candidates of csrc/grid_rule.h: filter-lag's ten in their order, then the grid filter at (2, w_2), (4, w_4) and (8, w_8) with the
 * fold, under the same margin.  The writer makes only fold = 1 grid words; the reader takes fold 0 as well.  A stream whose every
 * pick is among the first ten differs from the version-13 stream only in the header's version and its CRC.  A stream that holds
 * images of different widths, 1-D series and text behind each other gets each frame's own filter (INTEGRATION.md 4b,
 * "filter-grid: when").  The probe's cost is constant per frame, so small frames pay most.  on = 1 needs filter-lag on: on = 1
 * without it, and any other value, are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; whatever switches
 * filter-lag off switches this off.  0 (the default) writes every stream byte for byte as before.  All six container entry points
 * write the same bytes, with pipelining on or off.  Range reads of a grid frame start at a band of that frame's width
 * (2048 ceil(width / 64) elements) and use glcUngridDeltaUnshuffleRangeDevice.  The setting is also the version the plan speaks:
 * with it on the plan reads versions 1 to 5, 7, 8, 10, 13 and 14; every other plan, a filter-lag plan included, refuses a
 * version-14 stream as a stream-header failure.  A grid word under a version-13 or version-10 header, and any bit-31 word outside
 * the family above, is a frame-table failure naming the frame.  Widths above 65536, a width per block, the unfolded grid as a
 * candidate of its own and a 3-D predictor are not offered. */
CUDPPResult glcPlanSetContainerFilterGrid(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerFilterGrid(CUDPPHandle plan, unsigned int *on);

/* Filter-byte: filter-grid also finds the lag and the row stride of the byte predictor per frame, for 8-bit samples.  on = 1 writes
 * format version 16: version 14 whose frame word may also name glcByteDeltaDevice's filter.  A frame word is version 14's,
 * unchanged, or a byte word 1 | stride << 8 | (lag - 1) << 25 | 1 << 31: the low byte 1, stride 0 or 2..65536, lag 1..16, bits 29
 * and 30 zero; that frame went through glcByteDeltaDevice(lag, stride) as one segment and is format version 15's frame of its
 * bytes but for the word and the table CRC.  (Under version 14 every word with bit 31 set and the low byte 1 is illegal, so the
 * families cannot collide.)  The stream header's triple is (16, 0, 0); kinds, frames, tables, records and trailer are version
 * 14's.  Per frame the writer enqueues the byte probe behind the grid probe (glcByteProbeSegments and glcBytePlanesSegments, the
 * winners staying in device memory between them), reads fifteen costs, three lags, three widths and the byte lag and stride back
 * with the one wait filter-auto has, and walks the fifteen candidates of csrc/byte_rule.h: filter-grid's thirteen in their order,
 * then the byte predictor at (lag, 0) and at (lag, stride), under the same margin.  The writer makes strides of 0 or at least 17;
 * the reader takes version 15's whole family.  A stream whose every pick is among the first thirteen differs from the version-14
 * stream only in the header's version and its CRC.  on = 1 needs filter-grid on: on = 1 without it, and any other value, are
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was; whatever switches filter-grid off switches this off.
 * 0 (the default) writes every stream byte for byte as before.  All six container entry points write the same bytes, with
 * pipelining on or off.  Range reads of a byte frame start at a run, or at a band of that frame's stride, and use
 * glcUnbyteDeltaRangeDevice.  The setting is also the version the plan speaks: with it on the plan reads versions 1 to 5, 7, 8, 10,
 * 13, 14 and 16; every other plan, a filter-grid plan and a byte-delta plan included, refuses a version-16 stream as a
 * stream-header failure.  A byte word under an older header, and any bit-31 word outside the two families, is a frame-table
 * failure naming the frame.  glcPlanSetContainerByteDelta stays exclusive with filter-auto. */
CUDPPResult glcPlanSetContainerFilterByte(CUDPPHandle plan, unsigned int on);
CUDPPResult glcPlanGetContainerFilterByte(CUDPPHandle plan, unsigned int *on);

/* What the CHOOSE codec's order-0 frames take (INTEGRATION.md 4b "choose with filters"): level 0, the default, is CHOOSE as it is
 * (version 3); level 1 gives those frames the auto mode (record kinds 2, 3 and 5; version 8); levels 2 to 5 add filter-auto,
 * filter-lag, filter-grid and filter-byte (versions 10, 13, 14 and 16), and the writer then sorts every block into a class --
 * typed with an element size (the filter rule picks a filter for the block), BWT (the bigram rule), or order-0 -- and cuts a
 * frame wherever the class changes; an order-0 frame's filter is picked by the level's own probes over the whole frame, a BWT
 * frame has none.  Legal only while the codec is GLC_CONTAINER_CODEC_CHOOSE (else CUDPP_ERROR_ILLEGAL_CONFIGURATION, nothing
 * changed), level 0 to 5; every glcPlanSetContainerCodec call, one that sets CHOOSE again included, puts it back to 0.  The mode
 * and filter settings keep answering as they do under CHOOSE: off, and refused.  The streams are those versions' own: an order-0
 * plan with the level's settings reads them, and a plan with this level reads what that plan reads. */
CUDPPResult glcPlanSetContainerChooseFilters(CUDPPHandle plan, unsigned int level);
CUDPPResult glcPlanGetContainerChooseFilters(CUDPPHandle plan, unsigned int *level);

/* The lag and row stride of the ENCODER's byte predictor (glcByteDeltaDevice); lag 0 = off, the default.  On needs the order-0
 * codec, the auto mode on, the shuffle off (hence the delta, the delta-lag and the grid settings off) and filter-auto off; any other
 * state, a lag above 16 and a stride of 1 or above 65536 are CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was.
 * While it is on, glcPlanSetContainerShuffle with 2, 4 or 8 and glcPlanSetContainerFilterAuto(plan, 1) are refused; a codec change
 * or switching the auto mode off switches it off.  The stream is format version 15: version 8's frames, the header's flags
 * 1 | (stride ? 4 : 0) | (lag - 1) << 8 and its word 3 1 | stride << 8.  Decode, index and range reads take lag and stride from the
 * stream header, never from the plan; a range read decodes from the run (stride 0) or the band that holds its first byte.  The
 * setting is also the version the plan speaks: with it on the plan reads versions 1 to 5, 7, 8 and 15; every other plan refuses a
 * version-15 stream as a stream-header failure.  With it off every stream is written as before. */
CUDPPResult glcPlanSetContainerByteDelta(CUDPPHandle plan, unsigned int lag, unsigned int stride);
CUDPPResult glcPlanGetContainerByteDelta(CUDPPHandle plan, unsigned int *lag, unsigned int *stride);

/* The plane stride of the ENCODER's 3-D predictor (glcVolDeltaShuffleDevice); 0 = off, the default.  Any other plane needs the
 * grid setting (glcPlanSetContainerDeltaGrid) on at a width below it; any other state and a plane above 2^24 are
 * CUDPP_ERROR_ILLEGAL_CONFIGURATION and leave the setting as it was.  While it is on, glcPlanSetContainerDeltaGrid with a width
 * >= plane is refused.  Whatever switches the grid setting off switches this off; a change among elem 2, 4 and 8 keeps it.  The
 * stream is format version 17: version 12's stream with the header's flags 1 | fold << 1 | 4 | 8, word 3 elem | width << 8 and
 * word 7 the plane stride (0 under every other version); under version 17 the header's word 6 is the CRC-32 of words 0..5 followed
 * by word 7.  Decode, index and range reads take width, plane and fold from the stream header, never from the plan; a range read
 * starts at a slab.  The setting is also the version the plan speaks: with it on the plan reads versions 1 to 5, 7, 8, 12 and 17;
 * every other plan refuses a version-17 stream as a stream-header failure.  With it off every stream is written as before.  Not
 * offered: a stride chosen by the writer, the setting under filter-auto or CHOOSE, the byte predictor in 3-D. */
CUDPPResult glcPlanSetContainerDeltaVolume(CUDPPHandle plan, unsigned int plane);
CUDPPResult glcPlanGetContainerDeltaVolume(CUDPPHandle plan, unsigned int *plane);

/* Frames per filter of the plan's last successful container compress: out[i], i < 7, counts the frames that went through candidate
 * i of glcFilterProbeSegments' order -- (1,0) (2,0) (2,1) (4,0) (4,1) (8,0) (8,1), (1,0) being no filter -- and out[7] all frames.
 * With filter-auto off every frame counts for the plan's own filter; a frame that took a lag candidate of filter-lag, a grid
 * candidate of filter-grid or a byte candidate of filter-byte counts in out[7] only.  Zeros before the first. */
CUDPPResult glcContainerLastFilters(CUDPPHandle plan, unsigned long long out[8]);

/* Frames of the plan's last successful container compress that took the lag candidate of elem 2, of elem 4 and of elem 8
 * (glcPlanSetContainerFilterLag), and their sum.  Zeros before the first and with the setting off. */
CUDPPResult glcContainerLastLagFilters(CUDPPHandle plan, unsigned long long out[4]);

/* Frames of the plan's last successful container compress that took the grid candidate of elem 2, of elem 4 and of elem 8
 * (glcPlanSetContainerFilterGrid), and their sum.  Zeros before the first and with the setting off. */
CUDPPResult glcContainerLastGridFilters(CUDPPHandle plan, unsigned long long out[4]);

/* Frames of the plan's last successful container compress that took the byte candidate at (lag, 0) and at (lag, stride)
 * (glcPlanSetContainerFilterByte), and their sum.  Zeros before the first and with the setting off. */
CUDPPResult glcContainerLastByteFilters(CUDPPHandle plan, unsigned long long out[3]);

/* {what, frame, block} of the plan's last container failure (what = GlcContainerError; frame / block = ~0 where the
 * failure is not tied to one).  A successful call resets it to {0, ~0, ~0}. */
CUDPPResult glcContainerLastError(CUDPPHandle plan, unsigned long long out[3]);

#ifdef __cplusplus
}
#endif
#endif /* GLC_CONTAINER_H */
