// hd_batch.hip -- the batched form of the CUHD-shaped Huffman-only kernels (hd_encode.hip, hd_decode.hip): one table per
// segment, thousands of segments per launch.  The container's order-0 codec (format version 3, kind 2) and the
// glcHdSegments* calls of include/glc_hd.h.  gfx950 / wave64.  The per-tile and per-span code is hd_device.h's; what is
// here is the batch dimension: segments are at most 1 MiB, so a segment has at most 256 tiles of 4096 symbols and its
// stream at most 45 workgroups of 8192 units, and every scan over them is a short one inside the segment.
//   k_hdb_hist            (segment, slice of 64 KiB): LDS counters in 16 copies, u32 atomics into the segment's histogram
//   k_hdb_table           one workgroup per segment: the table builder's body; lens, codes, the decoder's u16 table, and
//                         from hist and lens the units of the segment's stream -- no pass over the data
//   k_hdb_enc_count       (segment, 4 tiles): bits of every tile
//   k_hdb_enc_scan        one workgroup per segment: bit offset of each of its <= 256 tiles; the segment's verdict (the
//                         stream has the announced length and ends inside the capacity); zeroes the units two tiles
//                         share, the last data unit and the pad unit -- the destination is not pre-zeroed
//   k_hdb_enc_pack        (segment, 4 tiles): the LDS merge, interior words stored, shared words ORed onto the zeros
//   k_hdb_span_functions  (segment, workgroup of 8192 units): the span functions, scanned inside the workgroup
//   k_hdb_emit            (same grid): each workgroup walks the <= 44 workgroup functions before it in its own segment
//                         (staged in LDS), then every lane decodes its span to its exact output index
#include "hd_device.h"
#include "glc_internal.h"

namespace glc {

constexpr uint32_t HB_SLICE_VEC = 4096;                 // 16-byte vectors per histogram workgroup (64 KiB)
constexpr uint32_t HB_MAX_TILES = HDB_MAX_LEN / HE_TILE;                                        // 256
constexpr uint32_t HB_MAX_UNITS = (GLC_HD_MAX_LEN * HDB_MAX_LEN + 31) / 32 + 1;                 // 360449
constexpr uint32_t HB_MAX_WG = (HB_MAX_UNITS + HD_WG_UNITS - 1) / HD_WG_UNITS;                  // 45
constexpr int HH_COPIES = 16;                           // lane & 15: 4 lanes of a wave share a copy
constexpr int HH_PITCH = 257;                           // copy c starts c banks further on

__device__ __forceinline__ uint32_t hb_len(const unsigned long long *len, uint32_t b, uint32_t max_len)
{
    const unsigned long long l = len[b];
    return l > max_len ? max_len : (uint32_t)l;
}

// ---------------------------------------------------------------------------------------------------------------------
// histogram and table
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hdb_hist(HdbSegs g, const uint32_t *__restrict__ skip, uint32_t *__restrict__ hist)
{
    // a segment [p, p + L): head bytes before the first 16-byte aligned address (< 16), nvec aligned vectors, a tail of
    // < 16 bytes.  Workgroup y of a segment counts vectors [y * 4096, + 4096); workgroup 0 also the head and the tail.
    __shared__ uint32_t s_h[HH_COPIES * HH_PITCH];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[b]) return;
    const uint32_t L = hb_len(g.len, b, g.max_len);
    const uint8_t *in = hdb_seg(g, b);
    uint32_t head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(in) & 15)) & 15u;
    if (head > L) head = L;
    const uint32_t nvec = (L - head) / 16;
    const uint32_t v0 = blockIdx.y * HB_SLICE_VEC, v1 = min(nvec, v0 + HB_SLICE_VEC);
    if (blockIdx.y && v0 >= nvec) return;
    for (uint32_t i = tid; i < HH_COPIES * HH_PITCH; i += 256) s_h[i] = 0;
    __syncthreads();
    uint32_t *H = s_h + (tid & (HH_COPIES - 1)) * HH_PITCH;
    const uint4 *V = reinterpret_cast<const uint4 *>(in + head);
    auto count4 = [&](uint32_t w) {
        atomicAdd(&H[w & 0xFFu], 1u);
        atomicAdd(&H[(w >> 8) & 0xFFu], 1u);
        atomicAdd(&H[(w >> 16) & 0xFFu], 1u);
        atomicAdd(&H[w >> 24], 1u);
    };
    uint32_t v = v0 + tid;
    for (; v + 3 * 256 < v1; v += 4 * 256) {            // four loads in flight per lane
        uint4 q[4];
#pragma unroll
        for (int r = 0; r < 4; r++) q[r] = V[v + r * 256];
#pragma unroll
        for (int r = 0; r < 4; r++) { count4(q[r].x); count4(q[r].y); count4(q[r].z); count4(q[r].w); }
    }
    for (; v < v1; v += 256) { const uint4 q = V[v]; count4(q.x); count4(q.y); count4(q.z); count4(q.w); }
    if (blockIdx.y == 0) {
        if (tid < head) atomicAdd(&H[in[tid]], 1u);
        const uint32_t t0 = head + nvec * 16;
        if (tid < 16 && t0 + tid < L) atomicAdd(&H[in[t0 + tid]], 1u);
    }
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < HH_COPIES; k++) c += s_h[k * HH_PITCH + tid];
    if (c) atomicAdd(&hist[(size_t)b * 256 + tid], c);
}

__global__ __launch_bounds__(HT_NT) void k_hdb_table(const uint32_t *__restrict__ hist, uint32_t count,
                                                     const uint32_t *__restrict__ skip, uint8_t *__restrict__ lens,
                                                     uint16_t *__restrict__ codes, uint32_t *__restrict__ lut,
                                                     unsigned long long *__restrict__ nunits)
{
    const uint32_t b = blockIdx.x;
    if (skip && skip[b]) return;
    const unsigned long long bits = hd_table_body<uint32_t, true>(hist + (size_t)b * 256, lens ? lens + (size_t)b * 256 : nullptr,
                                                                  codes ? codes + (size_t)b * 256 : nullptr,
                                                                  lut ? lut + (size_t)b * 1024 : nullptr);
    if (threadIdx.x == 0 && nunits) nunits[b] = (bits + 31) / 32 + 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// encode.  work: tile_bits[count][256], tile_off[count][256] (bits from the segment's start), ok[count]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HE_NT) void k_hdb_enc_count(HdbSegs g, const uint32_t *__restrict__ skip,
                                                         const uint8_t *__restrict__ lens, const uint16_t *__restrict__ codes,
                                                         uint32_t *__restrict__ tile_bits)
{
    __shared__ uint32_t s_cl[256];
    __shared__ uint32_t s_tmp[HE_NT / WAVE + 1];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (skip && skip[b]) return;
    const uint32_t L = hb_len(g.len, b, g.max_len), ntiles = (L + HE_TILE - 1) / HE_TILE;
    if (blockIdx.y * HE_TPW >= ntiles) return;
    const uint8_t *in = hdb_seg(g, b);
    he_load_table(lens + (size_t)b * 256, codes + (size_t)b * 256, s_cl);
    __syncthreads();
    for (uint32_t k = 0; k < HE_TPW; k++) {
        const uint32_t t = blockIdx.y * HE_TPW + k;
        if (t >= ntiles) break;
        const uint32_t bits = he_count_tile(in, L, (size_t)t * HE_TILE + tid * HE_SPT, s_cl, s_tmp);
        if (tid == 0) tile_bits[(size_t)b * HB_MAX_TILES + t] = bits;
    }
}

__global__ __launch_bounds__(256) void k_hdb_enc_scan(HdbSegs g, const uint32_t *__restrict__ skip,
                                                      const uint32_t *__restrict__ tile_bits, uint32_t *__restrict__ tile_off,
                                                      uint32_t *__restrict__ ok, const unsigned long long *__restrict__ nunits,
                                                      uint32_t *units_base, const unsigned long long *__restrict__ unit_off,
                                                      unsigned long long cap_units)
{
    __shared__ uint32_t s_tmp[256 / WAVE + 1];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const bool skipped = skip && skip[b];
    if (skipped) { if (tid == 0) ok[b] = 0; return; }
    const uint32_t L = hb_len(g.len, b, g.max_len), ntiles = (L + HE_TILE - 1) / HE_TILE;
    const uint32_t tb = tid < ntiles ? tile_bits[(size_t)b * HB_MAX_TILES + tid] : 0u;
    const bool anybad = __syncthreads_or((int)(tb == HE_BAD)) != 0;
    uint32_t total = 0;                                 // <= 2^20 * 11 bits
    const uint32_t ex = block_excl_add<256>(tb == HE_BAD ? 0u : tb, s_tmp, &total);
    if (tid < ntiles) tile_off[(size_t)b * HB_MAX_TILES + tid] = ex;
    const unsigned long long nun = ((unsigned long long)total + 31) / 32 + 1, uo = unit_off[b];
    // the announced length is what the offsets behind this segment were laid out with: a stream of another length (the
    // bytes changed since the histogram) or one that ends past the capacity is not written at all
    const bool good = !anybad && nun == nunits[b] && uo + nun <= cap_units;
    if (tid == 0) ok[b] = good ? 1u : 0u;
    if (!good) return;
    uint32_t *units = units_base + uo;
    if (tid > 0 && tid < ntiles && (ex & 31u)) units[ex >> 5] = 0u;     // the unit a tile boundary falls inside
    if (tid == 0) {
        if (total & 31u) units[total >> 5] = 0u;        // the last data unit: zero bits after the last code
        units[nun - 1] = 0u;                            // the pad unit
    }
}

__global__ __launch_bounds__(HE_NT) void k_hdb_enc_pack(HdbSegs g, const uint32_t *__restrict__ ok,
                                                        const uint8_t *__restrict__ lens, const uint16_t *__restrict__ codes,
                                                        const uint32_t *__restrict__ tile_bits, const uint32_t *__restrict__ tile_off,
                                                        uint32_t *units_base, const unsigned long long *__restrict__ unit_off)
{
    __shared__ uint32_t s_cl[256];
    __shared__ __attribute__((aligned(16))) uint32_t s_words[HE_MAXW];
    __shared__ uint32_t s_tmp[HE_NT / WAVE + 1];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (!ok[b]) return;                                 // skipped or refused: no store at all
    const uint32_t L = hb_len(g.len, b, g.max_len), ntiles = (L + HE_TILE - 1) / HE_TILE;
    if (blockIdx.y * HE_TPW >= ntiles) return;
    const uint8_t *in = hdb_seg(g, b);
    uint32_t *units = units_base + unit_off[b];
    he_load_table(lens + (size_t)b * 256, codes + (size_t)b * 256, s_cl);
    for (uint32_t k = 0; k < HE_TPW; k++) {
        const uint32_t t = blockIdx.y * HE_TPW + k;
        if (t >= ntiles) break;
        const uint32_t o = tile_off[(size_t)b * HB_MAX_TILES + t], want = tile_bits[(size_t)b * HB_MAX_TILES + t];
        const uint32_t sh = o & 31u;
        __syncthreads();                                // the table is in place / the previous tile's words have been read
        const uint32_t total = he_merge_tile(in, L, (size_t)t * HE_TILE + tid * HE_SPT, sh, s_cl, s_words, s_tmp);
        if (total != want) continue;                    // the bytes changed since the count: nothing outside the tile's own bits
        he_store_tile(s_words, sh, total, units + (o >> 5));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// decode.  work: pexcl[count][wgmax][256][12], fwg[count][wgmax][12]
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hb_nunits(const unsigned long long *nunits, uint32_t b, uint32_t wgmax)
{
    const unsigned long long n = nunits[b], cap = (unsigned long long)wgmax * HD_WG_UNITS;
    return (uint32_t)(n > cap ? cap : n);
}

__global__ __launch_bounds__(HD_LANES) void k_hdb_span_functions(const uint32_t *__restrict__ units_base,
                                                                 const unsigned long long *__restrict__ unit_off,
                                                                 const unsigned long long *__restrict__ nunits,
                                                                 const uint16_t *__restrict__ lut, const uint32_t *__restrict__ skip,
                                                                 uint32_t wgmax, uint32_t *__restrict__ pexcl, uint32_t *__restrict__ fwg)
{
    __shared__ uint32_t s_u[HD_LANES * HD_PITCH];
    __shared__ uint16_t s_lut[2048];
    __shared__ uint32_t s_tab[2][HD_LANES][HD_NOFF];
    __shared__ uint16_t s_chk[HD_LANES * HD_CHK_PITCH];
    const uint32_t b = blockIdx.x, wg = blockIdx.y, tid = threadIdx.x;
    if (skip && skip[b]) return;
    const uint32_t nu = hb_nunits(nunits, b, wgmax);
    if ((unsigned long long)wg * HD_WG_UNITS >= nu) return;
    hd_stage(units_base + unit_off[b], nu, (size_t)wg * HD_WG_UNITS, s_u, lut + (size_t)b * 2048, s_lut);
    const int src = hd_span_scan(s_u, s_lut, s_chk, s_tab);
    const size_t w = (size_t)b * wgmax + wg;
    uint32_t *P = pexcl + (w * HD_LANES + tid) * HD_TSTRIDE;
    for (uint32_t o = 0; o < HD_NOFF; o++) P[o] = tid ? s_tab[src][tid - 1][o] : o;   // exclusive; identity for lane 0
    if (tid < HD_NOFF) fwg[w * HD_TSTRIDE + tid] = s_tab[src][HD_LANES - 1][tid];
}

__global__ __launch_bounds__(HD_LANES) void k_hdb_emit(const uint32_t *__restrict__ units_base,
                                                       const unsigned long long *__restrict__ unit_off,
                                                       const unsigned long long *__restrict__ nunits,
                                                       const uint16_t *__restrict__ lut, const uint32_t *__restrict__ skip,
                                                       uint32_t wgmax, const uint32_t *__restrict__ pexcl,
                                                       const uint32_t *__restrict__ fwg, HdbOut g)
{
    __shared__ uint32_t s_u[HD_LANES * HD_PITCH];
    __shared__ uint16_t s_lut[2048];
    __shared__ uint32_t s_f[HB_MAX_WG * HD_TSTRIDE];
    const uint32_t b = blockIdx.x, wg = blockIdx.y, tid = threadIdx.x;
    if (skip && skip[b]) return;
    const uint32_t nu = hb_nunits(nunits, b, wgmax);
    if ((unsigned long long)wg * HD_WG_UNITS >= nu) return;
    const size_t w0 = (size_t)b * wgmax;
    for (uint32_t i = tid; i < wg * HD_TSTRIDE; i += HD_LANES) s_f[i] = fwg[w0 * HD_TSTRIDE + i];   // the functions before this one
    hd_stage(units_base + unit_off[b], nu, (size_t)wg * HD_WG_UNITS, s_u, lut + (size_t)b * 2048, s_lut);
    uint32_t o = 0, first = 0;                          // the segment starts at bit 0 / symbol 0; every lane walks (LDS broadcasts)
    for (uint32_t i = 0; i < wg; i++) {
        const uint32_t e = s_f[i * HD_TSTRIDE + (o < HD_NOFF ? o : 0)];
        first += e >> 4; o = e & 15;
    }
    const uint32_t p = pexcl[((w0 + wg) * HD_LANES + tid) * HD_TSTRIDE + (o < HD_NOFF ? o : 0)];
    const uint32_t L = hb_len(g.len, b, g.max_len);
    const size_t base = (size_t)first + (p >> 4);
    if (base >= L) return;
    hd_emit_span(s_u + tid * HD_PITCH, s_lut, p & 15, reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.base) + g.off[b]), base, L);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static uint32_t hb_wgmax(size_t max_len)
{
    const size_t units = (GLC_HD_MAX_LEN * max_len + 31) / 32 + 1;
    return (uint32_t)((units + HD_WG_UNITS - 1) / HD_WG_UNITS);
}

size_t hdb_encode_work_bytes(size_t count) { return 2 * up256(count * HB_MAX_TILES * 4) + up256(count * 4); }

size_t hdb_decode_work_bytes(size_t count, size_t max_len)
{
    const size_t w = count * hb_wgmax(max_len);
    return up256(w * HD_LANES * HD_TSTRIDE * 4) + up256(w * HD_TSTRIDE * 4);
}

hipError_t hdb_tables(hipStream_t st, const HdbSegs &g, bool make_hist, uint32_t *hist, uint8_t *lens, uint16_t *codes,
                      uint16_t *lut, unsigned long long *nunits, const uint32_t *skip, KernelProf *prof)
{
    if (g.count == 0) return hipSuccess;
    const double bytes = (double)g.count * g.max_len;
    if (make_hist) {
        hipError_t e = hipMemsetAsync(hist, 0, (size_t)g.count * 1024, st);
        if (e != hipSuccess) return e;
        const uint32_t nv = (g.max_len / 16 + HB_SLICE_VEC - 1) / HB_SLICE_VEC, nslice = nv ? nv : 1u;
        ProfScope ps(prof, PROF_HDB_HIST, st, bytes);
        hipLaunchKernelGGL(k_hdb_hist, dim3(g.count, nslice), dim3(256), 0, st, g, skip, hist);
    }
    {
        ProfScope ps(prof, PROF_HDB_TABLE, st, bytes);
        hipLaunchKernelGGL(k_hdb_table, dim3(g.count), dim3(HT_NT), 0, st, (const uint32_t *)hist, g.count, skip, lens, codes,
                           reinterpret_cast<uint32_t *>(lut), nunits);
    }
    return hipGetLastError();
}

hipError_t hdb_encode(hipStream_t st, const HdbSegs &g, const uint8_t *lens, const uint16_t *codes,
                      const unsigned long long *nunits, uint32_t *units_base, const unsigned long long *unit_off,
                      unsigned long long cap_units, const uint32_t *skip, void *work, KernelProf *prof)
{
    if (g.count == 0) return hipSuccess;
    uint8_t *W = static_cast<uint8_t *>(work);
    uint32_t *tile_bits = reinterpret_cast<uint32_t *>(W);
    uint32_t *tile_off = reinterpret_cast<uint32_t *>(W + up256((size_t)g.count * HB_MAX_TILES * 4));
    uint32_t *ok = reinterpret_cast<uint32_t *>(W + 2 * up256((size_t)g.count * HB_MAX_TILES * 4));
    const uint32_t ntiles = (g.max_len + HE_TILE - 1) / HE_TILE, nwg = (ntiles + HE_TPW - 1) / HE_TPW;
    const double bytes = (double)g.count * g.max_len;
    if (nwg) {
        ProfScope ps(prof, PROF_HDB_COUNT, st, bytes);
        hipLaunchKernelGGL(k_hdb_enc_count, dim3(g.count, nwg), dim3(HE_NT), 0, st, g, skip, lens, codes, tile_bits);
    }
    {
        ProfScope ps(prof, PROF_HDB_SCAN, st, bytes);
        hipLaunchKernelGGL(k_hdb_enc_scan, dim3(g.count), dim3(256), 0, st, g, skip, (const uint32_t *)tile_bits, tile_off, ok,
                           nunits, units_base, unit_off, cap_units);
    }
    if (nwg) {
        ProfScope ps(prof, PROF_HDB_PACK, st, bytes);
        hipLaunchKernelGGL(k_hdb_enc_pack, dim3(g.count, nwg), dim3(HE_NT), 0, st, g, (const uint32_t *)ok, lens, codes,
                           (const uint32_t *)tile_bits, (const uint32_t *)tile_off, units_base, unit_off);
    }
    return hipGetLastError();
}

hipError_t hdb_decode(hipStream_t st, const uint32_t *units_base, const unsigned long long *unit_off,
                      const unsigned long long *nunits, const uint16_t *lut, const HdbOut &g, const uint32_t *skip,
                      void *work, KernelProf *prof)
{
    if (g.count == 0) return hipSuccess;
    const uint32_t wgmax = hb_wgmax(g.max_len);
    uint8_t *W = static_cast<uint8_t *>(work);
    uint32_t *pexcl = reinterpret_cast<uint32_t *>(W);
    uint32_t *fwg = reinterpret_cast<uint32_t *>(W + up256((size_t)g.count * wgmax * HD_LANES * HD_TSTRIDE * 4));
    const double bytes = (double)g.count * g.max_len;
    {
        ProfScope ps(prof, PROF_HDB_SPANS, st, bytes);
        hipLaunchKernelGGL(k_hdb_span_functions, dim3(g.count, wgmax), dim3(HD_LANES), 0, st, units_base, unit_off, nunits, lut,
                           skip, wgmax, pexcl, fwg);
    }
    {
        ProfScope ps(prof, PROF_HDB_EMIT, st, bytes);
        hipLaunchKernelGGL(k_hdb_emit, dim3(g.count, wgmax), dim3(HD_LANES), 0, st, units_base, unit_off, nunits, lut, skip,
                           wgmax, (const uint32_t *)pexcl, (const uint32_t *)fwg, g);
    }
    return hipGetLastError();
}

} // namespace glc

using namespace glc;

extern "C" {

// work of one call: the encoder's tile tables, or the decoder's tables and span-function prefixes, whichever is larger
size_t glcHdSegmentsWorkBytes(size_t count, size_t maxLen)
{
    if (maxLen > HDB_MAX_LEN) return 0;
    const size_t enc = hdb_encode_work_bytes(count), dec = up256(count * 4096) + hdb_decode_work_bytes(count, maxLen);
    return enc > dec ? enc : dec;
}

static bool segs_ok(size_t count, size_t maxLen) { return count <= HDB_MAX_COUNT && maxLen <= HDB_MAX_LEN; }

int glcHdSegmentsTablesDevice(const unsigned char *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                              size_t count, size_t maxLen, unsigned int *d_hist, unsigned char *d_lens, unsigned short *d_codes,
                              unsigned long long *d_nunits, void *stream)
{
    if (!segs_ok(count, maxLen)) return 0;
    if (count == 0) return 1;
    if (!d_inBase || !d_offsets || !d_lengths || !d_hist || !d_lens || !d_codes || !d_nunits) return 0;
    const HdbSegs g{d_inBase, d_offsets, d_lengths, (uint32_t)count, (uint32_t)maxLen};
    return hdb_tables((hipStream_t)stream, g, true, d_hist, d_lens, d_codes, nullptr, d_nunits, nullptr, nullptr) == hipSuccess ? 1 : 0;
}

int glcHdSegmentsEncodeDevice(const unsigned char *d_inBase, const unsigned long long *d_offsets, const unsigned long long *d_lengths,
                              size_t count, size_t maxLen, const unsigned char *d_lens, const unsigned short *d_codes,
                              const unsigned long long *d_nunits, unsigned int *d_unitsBase, const unsigned long long *d_unitOffsets,
                              unsigned long long capUnits, const unsigned int *d_skip, void *d_work, void *stream)
{
    if (!segs_ok(count, maxLen)) return 0;
    if (count == 0) return 1;
    if (!d_inBase || !d_offsets || !d_lengths || !d_lens || !d_codes || !d_nunits || !d_unitsBase || !d_unitOffsets || !d_work) return 0;
    if (reinterpret_cast<uintptr_t>(d_unitsBase) & 3) return 0;
    const HdbSegs g{d_inBase, d_offsets, d_lengths, (uint32_t)count, (uint32_t)maxLen};
    return hdb_encode((hipStream_t)stream, g, d_lens, d_codes, d_nunits, d_unitsBase, d_unitOffsets, capUnits, d_skip, d_work,
                      nullptr) == hipSuccess ? 1 : 0;
}

int glcHdSegmentsDecodeDevice(const unsigned int *d_unitsBase, const unsigned long long *d_unitOffsets, const unsigned long long *d_nunits,
                              const unsigned int *d_hist, unsigned char *d_outBase, const unsigned long long *d_outOffsets,
                              const unsigned long long *d_lengths, size_t count, size_t maxLen, const unsigned int *d_skip,
                              void *d_work, void *stream)
{
    if (!segs_ok(count, maxLen)) return 0;
    if (count == 0) return 1;
    if (!d_unitsBase || !d_unitOffsets || !d_nunits || !d_hist || !d_outBase || !d_outOffsets || !d_lengths || !d_work) return 0;
    if (reinterpret_cast<uintptr_t>(d_unitsBase) & 3) return 0;
    hipStream_t st = (hipStream_t)stream;
    const HdbOut g{d_outBase, d_outOffsets, d_lengths, (uint32_t)count, (uint32_t)maxLen};
    const HdbSegs none{nullptr, nullptr, nullptr, (uint32_t)count, (uint32_t)maxLen};
    uint16_t *lut = static_cast<uint16_t *>(d_work);
    if (hdb_tables(st, none, false, const_cast<unsigned int *>(d_hist), nullptr, nullptr, lut, nullptr, d_skip, nullptr) != hipSuccess) return 0;
    return hdb_decode(st, d_unitsBase, d_unitOffsets, d_nunits, lut, g, d_skip, static_cast<uint8_t *>(d_work) + up256(count * 4096),
                      nullptr) == hipSuccess ? 1 : 0;
}

} // extern "C"
