/*
 * glc_hd.h -- C ABI of the CUHD-style Huffman-only encoder and decoder (BASELINE.json configs[4],
 * SURVEY.md 8(f)3).
 *
 * Replaces, for the same stream shape, the C++ interface of the reference
 *   cuhd::CUHDGPUDecoder::decode(...)            cuhd-icpp/include/cuhd_gpu_decoder.h,
 *                                                 src/cuhd_gpu_decoder.cu:422-523
 *   cuhd::CUHDCodetable / LLHuffmanEncoder        cuhd-icpp/src/cuhd_codetable.cc,
 *                                                 encoder/src/llhuffman_encoder.cc:160-262
 * Stream shape (cuhd_constants.h:15-24, cuhd_input_buffer.cc:20-27): symbols are
 * bytes, codewords are at most 11 bits (length-limited by package-merge), packed
 * MSB-first into 32-bit units, followed by one zero pad unit.  The reference's own
 * code assignment depends on libstdc++ sort/hash order (llhuffman_encoder.cc:48-51,
 * 143-155), so parity for this path is "decoded bytes == original bytes"
 * (demo.cc:176-178); this library fixes the assignment to plain canonical order
 * (by length, then symbol).
 *
 * The decoder does not iterate to self-synchronise (phase 2 of the reference loops with
 * a device->host flag copy per iteration, cuhd_gpu_decoder.cu:459-495).  Every 32-unit
 * span is summarised as a function {start offset 0..10} -> {offset into the next span,
 * symbols decoded}; those 11-entry functions compose associatively, so a scan gives the
 * exact start offset and output index of every span in a fixed number of passes.
 *
 * The reference encodes on the host (llhuffman_encoder.cc:200-238), as glcHdEncodeHost does.  glcHdHistogramDevice,
 * glcHdBuildTableDevice and glcHdEncodeDevice do the same work on the device: histogram -> table -> encode ->
 * glcHdDecodeDeviceTableOnDevice is a round trip that never leaves the device.  These calls only enqueue on `stream`
 * (a hipStream_t, or NULL), never wait on the host and keep no global state: encodes on different streams with
 * separate work buffers may overlap.  Each returns 1 when its arguments are valid and the work was enqueued, else 0,
 * and then nothing was launched.
 */
#ifndef GLC_HD_H
#define GLC_HD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLC_HD_MAX_LEN 11

/* Length-limited canonical Huffman table from a 256-bin histogram (host).
 * lens[s] = 0 for absent symbols.  Returns the number of coded symbols (0 on error). */
int glcHdBuildTable(const unsigned long long hist[256], unsigned char lens[256], unsigned short codes[256]);

/* Host encoder (the reference's encoder is CPU code too): returns units written incl. the
 * zero pad unit, or 0 if out_units (capacity cap_units) is too small. */
size_t glcHdEncodeHost(const unsigned char *in, size_t nsym, const unsigned char lens[256],
                       const unsigned short codes[256], unsigned int *out_units, size_t cap_units);

/* Units a stream of nsym symbols can need, pad unit included: ceil(11 * nsym / 32) + 1. */
size_t glcHdEncodeBound(size_t nsym);

/* Device scratch glcHdEncodeDevice needs for nsym symbols. */
size_t glcHdEncodeWorkBytes(size_t nsym);

/* d_hist[256] (u64, device) = byte counts of d_in[0 .. nsym).  Overwrites d_hist; d_in may have any alignment.
 * nsym < 2^40. */
int glcHdHistogramDevice(const unsigned char *d_in, size_t nsym, unsigned long long *d_hist, void *stream);

/* glcHdBuildTable on the device: d_lens[256] / d_codes[256] bit-identical to the host builder's for the same histogram
 * (histogram total below 2^56).  d_table2048 (optional, may be NULL; 4-byte aligned): the reference's decoder table,
 * {num_bits, symbol} byte pairs indexed by the next 11 stream bits (cuhd_codetable.h:20-23); entries no codeword
 * reaches are {0, 0}.  An empty histogram gives all-zero lens, codes and table. */
int glcHdBuildTableDevice(const unsigned long long *d_hist, unsigned char *d_lens, unsigned short *d_codes,
                          unsigned char *d_table2048, void *stream);

/* The stream glcHdEncodeHost writes, word for word (MSB-first 32-bit units, zero bits after the last code, one zero pad
 * unit), from a table in device memory (codes[s] holds lens[s] bits; higher bits are ignored).  *d_nunits (device u64)
 * = units written, pad included; 0 when a symbol of the input has lens == 0 or lens > 11, or when the stream needs more
 * than cap_units units -- and then NOTHING is written to d_units.  d_units must be 4-byte aligned; nsym < 2^40;
 * nsym == 0 writes the pad unit alone.  d_work: glcHdEncodeWorkBytes(nsym) bytes, one per encode in flight.
 * The decoders above take at most 2^31 units, i.e. streams of up to 2^36 bits. */
int glcHdEncodeDevice(const unsigned char *d_in, size_t nsym, const unsigned char *d_lens, const unsigned short *d_codes,
                      unsigned int *d_units, size_t cap_units, unsigned long long *d_nunits, void *d_work, void *stream);

/* Device scratch needed by glcHdDecodeDevice for a stream of `nunits` units. */
size_t glcHdWorkBytes(size_t nunits);

/* d_units: nunits 32-bit units in device memory (incl. the pad unit); d_out: nsym bytes.
 * Returns 1 on success.  stream = hipStream_t or NULL.  nunits <= 2^31. */
int glcHdDecodeDevice(const unsigned int *d_units, size_t nunits, const unsigned char lens[256],
                      const unsigned short codes[256], unsigned char *d_out, size_t nsym,
                      void *d_work, void *stream);

/* Same, with the decoder table exactly as the reference holds it: cuhd::CUHDCodetableItemSingle[2048], i.e.
 * {num_bits, symbol} byte pairs indexed by the next 11 stream bits (cuhd_codetable.h:20-23, built by
 * LLHuffmanEncoder::get_decoder_table, llhuffman_encoder.cc:240-262).  This is the call
 * cuhd::CUHDGPUDecoder::decode (cuhd_gpu_decoder.cu:422-431) maps to: units, table, output. */
int glcHdDecodeDeviceTable(const unsigned int *d_units, size_t nunits, const unsigned char *table2048,
                           unsigned char *d_out, size_t nsym, void *d_work, void *stream);

/* Same again, with the table where cuhd::CUHDGPUCodetable keeps it -- in DEVICE memory (its get() pointer).  Nothing is
 * copied and the host is not held: the decode is only enqueued on `stream`.  include/glc_cuhd_adapter.hpp wraps this in
 * the reference's own call signature. */
int glcHdDecodeDeviceTableOnDevice(const unsigned int *d_units, size_t nunits, const unsigned char *d_table2048,
                                   unsigned char *d_out, size_t nsym, void *d_work, void *stream);

/* The batched form of the device calls above: `count` segments [d_inBase + d_offsets[i], + d_lengths[i]) with ONE TABLE
 * EACH, thousands per launch (the container's order-0 codec, include/glc_container.h, is built from these).  Any byte
 * alignment; offsets, lengths and unit offsets are u64 arrays in DEVICE memory; no segment is longer than maxLen, and
 * maxLen <= 1048576 (a larger maxLen is refused; a longer d_lengths[i] is read as maxLen); count <= 4194304 per call.  Like the calls above they
 * only enqueue on `stream`, never wait on the host, keep no global state and return 1 when the arguments are valid and the
 * work was enqueued, else 0 with nothing launched; count == 0 is a success that does nothing.
 *
 * d_work: glcHdSegmentsWorkBytes(count, maxLen) bytes, one per call in flight; it serves either direction.  The encoder
 * needs 2 KiB of it per segment.  The decoder needs 4 KiB of tables per segment plus the span-function prefixes of every
 * stream at its longest -- 48 bytes per 128 bytes of 11-bit stream, 541 KiB per segment at maxLen = 1 MiB -- so for
 * thousands of large segments decode in chunks of segments rather than in one call.  The encoder loads a tile's symbols 16
 * bytes per lane when the segment starts on a 16-byte boundary and byte by byte when it does not (rate not measured). */
size_t glcHdSegmentsWorkBytes(size_t count, size_t maxLen);

/* Per segment: d_hist[i][256] (u32) = its byte counts; d_lens[i][256] / d_codes[i][256] = the table glcHdBuildTable gives
 * for them (all zero for an empty segment); d_nunits[i] = the units its stream needs, pad unit included:
 * ceil(sum hist * lens / 32) + 1, so 1 for an empty segment.  No pass over the data is needed for that number, which is
 * what lets a caller lay the streams out (d_unitOffsets below) before anything is encoded. */
int glcHdSegmentsTablesDevice(const unsigned char *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                              size_t count, size_t maxLen, unsigned int *d_hist, unsigned char *d_lens, unsigned short *d_codes,
                              unsigned long long *d_nunits, void *stream);

/* Segment i's stream, word for word what glcHdEncodeHost writes for it with table i, at d_unitsBase + d_unitOffsets[i]
 * (d_unitsBase 4-byte aligned; units, not bytes): d_nunits[i] units, every one of them written -- the destination need not
 * be zeroed -- and none outside them, whatever order the workgroups run in.  d_skip (may be NULL): a segment whose
 * d_skip[i] != 0 is left alone.  A segment whose stream would end past capUnits (counted from d_unitsBase), or whose bytes
 * no longer give d_nunits[i] units with its table, is not written at all. */
int glcHdSegmentsEncodeDevice(const unsigned char *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                              size_t count, size_t maxLen, const unsigned char *d_lens, const unsigned short *d_codes,
                              const unsigned long long *d_nunits, unsigned int *d_unitsBase, const unsigned long long *d_unitOffsets,
                              unsigned long long capUnits, const unsigned int *d_skip, void *d_work, void *stream);

/* The inverse: the tables are rebuilt on the device from d_hist[i][256] (u32; what glcHdSegmentsTablesDevice wrote), and
 * d_lengths[i] symbols of the stream of d_nunits[i] units at d_unitsBase + d_unitOffsets[i] are written to
 * d_outBase + d_outOffsets[i].  Whatever the units hold, nothing is read outside a segment's d_nunits[i] units and nothing
 * written outside its d_lengths[i] bytes.  d_skip as above. */
int glcHdSegmentsDecodeDevice(const unsigned int *d_unitsBase, const unsigned long long *d_unitOffsets, const unsigned long long *d_nunits,
                              const unsigned int *d_hist, unsigned char *d_outBase, const unsigned long long *d_outOffsets,
                              const unsigned long long *d_lengths, size_t count, size_t maxLen, const unsigned int *d_skip,
                              void *d_work, void *stream);

/* Measurement aid: live per-kernel profile of the two decode entry points (hipEvent pairs on the call's stream around
 * k_hd_span_functions / the three k_hd_walk launches / k_hd_emit).  glcHdEnableProfile(1) switches it on and resets it;
 * glcHdKernelProfile(i, name, cap, out3) waits for the device and returns 1 with the slot's name and
 * out3 = {sum of launch durations in ms, launches, decoded bytes}, 0 past the last slot. */
int glcHdEnableProfile(int on);
int glcHdKernelProfile(int index, char *name, size_t nameCap, double *out3);

#ifdef __cplusplus
}
#endif
#endif
