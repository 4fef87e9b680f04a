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
#include "hd_device.h"

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
// table: glcHdBuildTable (hd_decode.hip) restated for one workgroup of 512 lanes (hd_device.h)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HT_NT) void k_hd_table(const unsigned long long *__restrict__ hist, uint8_t *__restrict__ lens,
                                                    uint16_t *__restrict__ codes, uint32_t *__restrict__ table2048)
{
    (void)hd_table_body<unsigned long long, false>(hist, lens, codes, table2048);
}

// ---------------------------------------------------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HS_NT = 1024;
constexpr int HS_TPT = 16;                              // tiles per scan lane and pass

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
        const uint32_t bits = he_count_tile(in, nsym, t * HE_TILE + (size_t)tid * HE_SPT, s_cl, s_tmp);
        if (tid == 0) tile_bits[t] = bits;
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
        const uint32_t total = he_merge_tile(in, nsym, t * HE_TILE + (size_t)tid * HE_SPT, sh, s_cl, s_words, s_tmp);
        // the count pass and this one read the same bytes; if they disagree (the input changed in between) nothing of
        // the tile is stored, so no unit outside [tb, te) can be touched
        if ((unsigned long long)total != te - tb) continue;
        he_store_tile(s_words, sh, total, units + (tb >> 5));
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
