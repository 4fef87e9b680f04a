// vol.hip -- the 3-D (plane-stride) predictor of the container's typed-data filter (INTEGRATION.md 4b "Delta: volume", format
// version 17): grid.hip's 2-D predictor over the differences to the element one PLANE behind, for row-major volumes (3-D float
// fields, stacks of detector frames, CT and MRI stacks).  With x[i] element i of a segment as a little-endian unsigned integer of
// ELEM = 2, 4 or 8 bytes, arithmetic modulo 2^(8 ELEM), RUN = 2048, the row width 2 <= W <= 65536, P = 2048 ceil(W / 64), the
// plane stride W < S <= 2^24 elements and the slab Q = P ceil(16 S / P) (about 16 planes, whole bands, at most 2^28 + 2^21):
//   forward   w[i] = x[i] where i mod Q < S, else x[i] - x[i - S]; v[i] = w[i] where i mod P < W, else w[i] - w[i - W];
//             d[i] = v[i] where i mod RUN == 0, else v[i] - v[i - 1]; the fold and the planes of grid.hip
//   inverse   grid.hip's inverse gives w; then x[i] = w[i] + x[i - S] for i mod Q >= S, up every slab
// The rule is linear in i: a frame needs no row or plane alignment, S need not be a multiple of W.  Slabs are independent, bands
// nest inside slabs and runs inside bands.  With S >= q no element has a plane behind it: the output is grid.hip's.
//
// Forward, one pass on grid.hip's tile, no pre-pass and no frame-sized scratch: a tile takes FOUR raw images, its own bytes and
// the bytes W ELEM, S ELEM and (S + W) ELEM in front of them, each at its own alignment as aligned 16-byte granules; no granule
// that lies wholly in front of the segment is read (its elements belong to differences that the slab or the band predicate
// zeroes).  A lane needs w at i, i - 1, i - W and i - W - 1 for its granule: each is x[k] - x[k - S] under the slab predicate of
// its OWN index k, stated on the slab-relative index of i (i - W and i - W - 1 are only used where they lie in i's band, so in
// its slab; i - 1 only where it lies in i's run); the four then combine as in grid.hip's forward.
// LDS: the four raw images, 65664 bytes, and nothing else: two workgroups per CU.  A thread keeps the four result granules of
// its tile in registers across a barrier and then builds the padded image (18432 bytes) over the raw images, which are dead by
// then.  A fifth array for the padded image would come to 84096 bytes and one workgroup per CU.
//
// Inverse, nothing fused: grid.hip's two kernels, then grid.hip's k_grid_vsum once more with (S, Q) in the place of (W, P): a
// lane owns a column slice of a slab and walks its planes; the 16-byte path where S ELEM and the address are multiples of 16,
// the element path otherwise.  The kernel is reused as it is: its band-relative indices are 32-bit and stay below
// Q + 4 S < 2^29.
#include "grid_tile.h"

namespace glc {

constexpr uint32_t VL_GPT = SH_TILE / 16 / SH_THREADS;         // granules of a tile per thread: 4

// w = x - (the element S back, where `keep` says the element has one): c -= select(z)
template <uint32_t ELEM, class Keep>
__device__ __forceinline__ void vl_plane(uint32_t (&c)[4], uint32_t (&z)[4], Keep keep)
{
    gd_select<ELEM>(z, keep);
    lg_combine<ELEM, true>(c, z);
}

// the aligned granules of the `cnt * ELEM` bytes at byte `at` of the segment (at may be negative) into an image; sh: at's alignment
__device__ __forceinline__ void vl_load(const uint8_t *in, long long at, uint32_t sh, uint32_t bytes, uint32_t *image, uint32_t tid)
{
    const uint32_t ng = (sh + bytes + 15) / 16;                // <= SH_NGI
    for (uint32_t g = tid; g < ng; g += SH_THREADS) {
        const long long off = at - (long long)sh + 16ll * g;   // the aligned granule's first byte in the segment
        if (off > -16) reinterpret_cast<uint4 *>(image + GD_FRONT)[g] = *reinterpret_cast<const uint4 *>(in + off);
    }
}

// forward: elements [i0, i0 + cnt) of a segment whose q whole elements start at `in`; i0 is a multiple of RUN
template <uint32_t ELEM>
__device__ __forceinline__ void vl_tile_forward(const uint8_t *in, uint8_t *out, unsigned long long q, unsigned long long i0,
                                                uint32_t cnt, uint32_t W, uint32_t P, uint32_t S, uint32_t Q, uint32_t fold, uint32_t *lds)
{
    constexpr uint32_t E = 16 / ELEM;                          // elements of a granule
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t *raw = lds, *above = lds + GD_RAW_WORDS, *back = lds + 2 * GD_RAW_WORDS, *backabove = lds + 3 * GD_RAW_WORDS;
    const unsigned long long base = (unsigned long long)(uintptr_t)in;
    // the tile's byte in the segment, the row above's, the plane behind's and its row above's
    const long long a = (long long)(i0 * ELEM), ab = a - (long long)W * ELEM, az = a - (long long)S * ELEM, azb = az - (long long)W * ELEM;
    const uint32_t s = (uint32_t)((base + (unsigned long long)a) & 15), sb = (uint32_t)((base + (unsigned long long)ab) & 15);
    const uint32_t sz = (uint32_t)((base + (unsigned long long)az) & 15), szb = (uint32_t)((base + (unsigned long long)azb) & 15);
    vl_load(in, a, s, cnt * ELEM, raw, tid);
    vl_load(in, ab, sb, cnt * ELEM, above, tid);
    vl_load(in, az, sz, cnt * ELEM, back, tid);
    vl_load(in, azb, szb, cnt * ELEM, backabove, tid);
    __syncthreads();
    const uint32_t nge = (cnt * ELEM + 15) / 16;               // <= 1024
    const uint32_t rt = (uint32_t)(i0 % P), zt = (uint32_t)(i0 % Q);      // the tile's first element within its band, its slab
    uint32_t res[VL_GPT][4];
#pragma unroll
    for (uint32_t n = 0; n < VL_GPT; n++) {
        const uint32_t g = tid + n * SH_THREADS;
        if (g < nge) {
            // c: the granule, p: the 16 bytes one element back; ca, pa: the same of the row above; z: what lies a plane behind c.
            // r, t: the band- and the slab-relative index of the granule's first element (P and Q are multiples of E, so a
            // granule leaves neither)
            uint32_t (&c)[4] = res[n];
            uint32_t p[4], ca[4], pa[4], z[4];
            const uint32_t r = (rt + g * E) % P, t = (zt + g * E) % Q;
            lg_read16(raw + GD_FRONT, (int)(s + 16 * g), c);
            lg_read16(back + GD_FRONT, (int)(sz + 16 * g), z);
            vl_plane<ELEM>(c, z, [&](uint32_t k) { return t + k >= S; });
            lg_read16(raw + GD_FRONT, (int)(s + 16 * g) - (int)ELEM, p);
            lg_read16(back + GD_FRONT, (int)(sz + 16 * g) - (int)ELEM, z);
            vl_plane<ELEM>(p, z, [&](uint32_t k) { return t + k > S; });           // (element i - 1: slab-relative t + k - 1)
            lg_read16(above + GD_FRONT, (int)(sb + 16 * g), ca);
            lg_read16(backabove + GD_FRONT, (int)(szb + 16 * g), z);
            vl_plane<ELEM>(ca, z, [&](uint32_t k) { return t + k >= S + W; });     // (element i - W: t + k - W)
            lg_read16(above + GD_FRONT, (int)(sb + 16 * g) - (int)ELEM, pa);
            lg_read16(backabove + GD_FRONT, (int)(szb + 16 * g) - (int)ELEM, z);
            vl_plane<ELEM>(pa, z, [&](uint32_t k) { return t + k > S + W; });
            gd_select<ELEM>(ca, [&](uint32_t k) { return r + k >= W; });
            gd_select<ELEM>(pa, [&](uint32_t k) { return r + k > W; });
            lg_combine<ELEM, true>(c, ca);
            lg_combine<ELEM, true>(p, pa);
            lg_mask<ELEM>(p, (16 * g) & (LG_RUN * ELEM - 1), ELEM);
            lg_combine<ELEM, true>(c, p);
            lg_fold<ELEM, false>(c, fold);
        }
    }
    __syncthreads();                                           // (every read of the raw images is done: the padded image goes over them)
#pragma unroll
    for (uint32_t n = 0; n < VL_GPT; n++) {
        const uint32_t g = tid + n * SH_THREADS;
        if (g < nge) lg_img_store<ELEM>(lds, g, res[n]);
    }
    __syncthreads();
    lg_planes<ELEM>(lds, out, q, i0, cnt, tid, lane, wave);
}

template <uint32_t ELEM>
__global__ __launch_bounds__(SH_THREADS) void k_vol_forward(const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t W, uint32_t P,
                                                            uint32_t S, uint32_t Q, uint32_t fold)
{
    using G = ShGeom<ELEM>;
    __shared__ __attribute__((aligned(16))) uint32_t lds[4 * GD_RAW_WORDS];
    static_assert(G::TQ % LG_RUN == 0, "a tile holds whole runs");
    static_assert(4 * GD_RAW_WORDS >= LG_IMG_WORDS && (GD_RAW_WORDS * 4) % 16 == 0, "the padded image fits over the raw images, each 16-byte aligned");
    static_assert(VL_GPT * SH_THREADS * 16 == SH_TILE, "a thread's granules cover the tile");
    const unsigned long long q = len / ELEM, nt = q ? (q + G::TQ - 1) / G::TQ : 1;
    for (unsigned long long t = blockIdx.x; t < nt; t += gridDim.x) {
        const unsigned long long i0 = t * G::TQ;
        const uint32_t cnt = (uint32_t)min((unsigned long long)G::TQ, q - i0);
        if (cnt) vl_tile_forward<ELEM>(in, out, q, i0, cnt, W, P, S, Q, fold, lds);
        if (t + 1 == nt && threadIdx.x < (uint32_t)(len - q * ELEM)) out[q * ELEM + threadIdx.x] = in[q * ELEM + threadIdx.x];
        __syncthreads();                                       // (the next tile of this workgroup reuses the LDS images)
    }
}

template <uint32_t ELEM>
static hipError_t vl_launch_forward(hipStream_t st, uint32_t grid, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t W,
                                    uint32_t S, uint32_t fold)
{
    hipLaunchKernelGGL(k_vol_forward<ELEM>, dim3(grid), dim3(SH_THREADS), 0, st, in, out, len, W, ct_grid_period(W), S, ct_vol_slab(W, S), fold);
    return hipGetLastError();
}

hipError_t vol_shuffle_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long len, uint32_t elem, uint32_t width,
                              uint32_t plane, uint32_t fold, bool inverse)
{
    if (!shuffle_elem_ok(elem) || !ct_grid_width_ok(width) || !ct_vol_plane_ok(width, plane) || fold > 1) return hipErrorInvalidValue;
    if (len == 0) return hipSuccess;
    if (inverse) {
        const hipError_t e = grid_shuffle_device(st, in, out, len, elem, width, fold, true);
        return e != hipSuccess ? e : grid_vsum_device(st, out, len / elem, elem, plane, ct_vol_slab(width, plane));
    }
    const unsigned long long tq = SH_TILE / elem, q = len / elem, nt = q ? (q + tq - 1) / tq : 1;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(nt, 1u << 24);     // (one workgroup per tile up to 256 GiB)
    switch (elem) {
    case 2: return vl_launch_forward<2>(st, grid, in, out, len, width, plane, fold);
    case 4: return vl_launch_forward<4>(st, grid, in, out, len, width, plane, fold);
    default: return vl_launch_forward<8>(st, grid, in, out, len, width, plane, fold);
    }
}

// the range form of the inverse: `first` is a multiple of Q, so out[0] is the first element of a slab (and of a band)
hipError_t unvol_unshuffle_range_device(hipStream_t st, const uint8_t *in, uint8_t *out, unsigned long long q, uint32_t elem,
                                        uint32_t width, uint32_t plane, uint32_t fold, unsigned long long first, unsigned long long count)
{
    if (!shuffle_elem_ok(elem) || !ct_grid_width_ok(width) || !ct_vol_plane_ok(width, plane) || fold > 1) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    if (first % ct_vol_slab(width, plane)) return hipErrorInvalidValue;
    const hipError_t e = ungrid_unshuffle_range_device(st, in, out, q, elem, width, fold, first, count);
    return e != hipSuccess ? e : grid_vsum_device(st, out, count, elem, plane, ct_vol_slab(width, plane));
}

} // namespace glc
