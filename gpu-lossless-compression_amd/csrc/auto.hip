// auto.hip -- the auto mode of the container's order-0 codec (format version 8): the probe and the small
// kernels that pick a record kind per block from the probe's statistics.  gfx950 / wave64.
//   k_au_probe    one read of a segment gives hist[256], its byte counts, and uniform[256], uniform[v] = its 64-byte chunks (cut
//                 from the segment's start; the last may be short) that hold byte v alone.  A workgroup of 256 lanes owns a tile
//                 of 64 KiB; a lane holds 16 bytes, four lanes a chunk, a wave 1 KiB a pass.  A lane's granule is uniform when
//                 its four dwords equal its first byte repeated; a chunk is when its lanes' granules are and agree with the
//                 quad's first lane (a DPP quad broadcast and one ballot).  Counts go to LDS counters in 16 copies as in
//                 k_hdb_hist, but a uniform chunk adds its length with ONE atomic instead of 64 on one address, and a pass of
//                 sixteen uniform chunks of one byte adds 1024 with one: the long runs of one byte, where same-address atomics
//                 are slowest, cost the least.  16-byte loads where the segment's address allows, a byte path where it does not.
//   k_au_cand     one wave per block: candidate S (what the sparse mode's writer would make: kind 3 when 32 E >= nch with
//                 E = uniform[fill], else kind 2) with K's counts and length from the statistics, and the estimate wA of the
//                 block's rANS record from its counts and the q of its rANS table (auto_rule.h)
//   k_au_choose   behind the Huffman tables of candidate S's counts: wS, the choice, the skip masks of the passes that follow
// Behind those passes k_ct_kind0<auto> (container.hip) gives the actual record sizes and the encoders' skip masks.
// Any segment length up to 2^20, any byte alignment.
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t AU_THREADS = 256, AU_TILE = 65536, AU_PASS = 1024, AU_PASSES = AU_TILE / AU_PASS;
constexpr uint32_t AU_COPIES = 16, AU_PITCH = 257;         // (k_hdb_hist's: lane & 15, copy c starts c banks further on)

__device__ __forceinline__ uint32_t au_len(const unsigned long long *len, uint32_t i, uint32_t max_len)
{
    const unsigned long long l = len[i];
    return l > max_len ? max_len : (uint32_t)l;
}

// n (1 .. 16) bytes at p as four dwords; the bytes from n on repeat the first, so that they never break a uniform granule
__device__ __forceinline__ uint4 au_load16(const uint8_t *p, uint32_t n, bool aligned)
{
    if (aligned && n == 16) return *reinterpret_cast<const uint4 *>(p);
    const uint32_t first = p[0];
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) w[k >> 2] |= (k < n ? (uint32_t)p[k] : first) << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(AU_THREADS) void k_au_probe(const uint8_t *data, const unsigned long long *__restrict__ data_off,
                                                         const unsigned long long *__restrict__ data_len, uint32_t max_len,
                                                         uint32_t *__restrict__ hist, uint32_t *__restrict__ uniform)
{
    __shared__ uint32_t s_h[AU_COPIES * AU_PITCH];
    __shared__ uint32_t s_u[256];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t L = au_len(data_len, b, max_len);
    const uint32_t t0 = blockIdx.y * AU_TILE;
    if (t0 >= L) return;
    const uint8_t *in = reinterpret_cast<const uint8_t *>(reinterpret_cast<uintptr_t>(data) + data_off[b]);
    const bool al = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    for (uint32_t i = tid; i < AU_COPIES * AU_PITCH; i += AU_THREADS) s_h[i] = 0;
    s_u[tid] = 0;
    __syncthreads();
    uint32_t *H = s_h + (tid & (AU_COPIES - 1)) * AU_PITCH;
    auto count4 = [&](uint32_t w) {
        atomicAdd(&H[w & 0xFFu], 1u);
        atomicAdd(&H[(w >> 8) & 0xFFu], 1u);
        atomicAdd(&H[(w >> 16) & 0xFFu], 1u);
        atomicAdd(&H[w >> 24], 1u);
    };
    // one pass: the wave's 1 KiB at segment offset o0 (wave-uniform, < L), this lane's granule v of n valid bytes (0: none)
    auto pass = [&](uint32_t o0, uint4 v, uint32_t n) {
        const bool active = n != 0;
        const uint32_t b0 = v.x & 0xFFu, rep = b0 * 0x01010101u;
        const bool own = v.x == rep && v.y == rep && v.z == rep && v.w == rep;
        const uint32_t q0 = GLC_DPP(b0, 0x00, 0xf);            // quad_perm [0, 0, 0, 0]: the byte of the chunk's first lane
        const uint64_t bad = __ballot(active && !(own && b0 == q0));
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
        if (o0 + AU_PASS <= L && bad == 0 && __ballot(b0 != first) == 0) {     // sixteen whole chunks of one byte
            if (lane == 0) { atomicAdd(&H[first], AU_PASS); atomicAdd(&s_u[first], AU_PASS / SP_CHUNK); }
            return;
        }
        const bool chunk_bad = ((bad >> (lane & ~3u)) & 0xFull) != 0;
        if (!active) return;
        if (!chunk_bad) {                                      // a uniform chunk: its first lane adds its length
            if ((lane & 3u) == 0) {
                const uint32_t c0 = o0 + 16 * lane;
                atomicAdd(&H[b0], min(SP_CHUNK, L - c0));
                atomicAdd(&s_u[b0], 1u);
            }
        } else if (n == 16) {
            count4(v.x); count4(v.y); count4(v.z); count4(v.w);
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (uint32_t k = 0; k < n; k++) atomicAdd(&H[(w[k >> 2] >> (8 * (k & 3))) & 0xFFu], 1u);
        }
    };
    // the wave's passes of the tile: wave, wave + 4, ...; four loads in flight
    for (uint32_t p = wave; p < AU_PASSES; p += 16) {
        if (t0 + p * AU_PASS >= L) break;
        uint4 q[4];
        uint32_t n[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t o = t0 + (p + 4 * r) * AU_PASS + 16 * lane;
            n[r] = o < L ? min(16u, L - o) : 0u;
            q[r] = n[r] ? au_load16(in + o, n[r], al) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t o0 = t0 + (p + 4 * r) * AU_PASS;
            if (o0 < L) pass(o0, q[r], n[r]);
        }
    }
    __syncthreads();
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < AU_COPIES; k++) c += s_h[k * AU_PITCH + tid];
    if (c) atomicAdd(&hist[(size_t)b * 256 + tid], c);
    if (s_u[tid]) atomicAdd(&uniform[(size_t)b * 256 + tid], s_u[tid]);
}

hipError_t probe_segments(hipStream_t st, const uint8_t *data, const unsigned long long *data_off, const unsigned long long *data_len,
                          uint32_t count, uint32_t max_len, uint32_t *hist, uint32_t *uniform)
{
    if (count == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)count * 1024, st);
    if (e == hipSuccess) e = hipMemsetAsync(uniform, 0, (size_t)count * 1024, st);
    if (e != hipSuccess || max_len == 0) return e;
    hipLaunchKernelGGL(k_au_probe, dim3(count, (max_len + AU_TILE - 1) / AU_TILE), dim3(AU_THREADS), 0, st, data, data_off, data_len,
                       max_len, hist, uniform);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the container encoder's steps around it (container_api.cpp, Encoder::frame_auto)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_au_cand(SpSegs g, CtEncSparse sp, CtEncAuto au, const uint32_t *__restrict__ hist,
                                                 const uint8_t *__restrict__ ans_tab, unsigned long long *in_off,
                                                 unsigned long long *in_len)
{
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= g.count) return;
    const uint32_t L = au_len(g.data_len, b, g.max_len), nch = (L + SP_CHUNK - 1) / SP_CHUNK;
    const uint32_t fill = g.fill[b] & 255u;
    uint8_t *data = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.data) + g.data_off[b]);
    uint8_t *K = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.kept) + g.kept_off[b]);
    // E counts the last chunk when it is all fill; whether it is says how many bytes the elided chunks hold
    const uint32_t E = min(au.uniform[(size_t)b * 256 + fill], nch);
    const uint32_t last0 = nch ? (nch - 1) * SP_CHUNK : 0u, last_n = L - last0;
    const bool last_kept = __ballot(lane < last_n && data[last0 + lane] != fill) != 0;
    const uint32_t kept = nch - E;
    const uint32_t klen = SP_CHUNK * kept - (last_kept ? SP_CHUNK * nch - L : 0u);
    const bool is3 = 32ull * E >= nch;
    // candidate S's counts (K's: only the fill's change, by the elided bytes) and the cost of the block's own at its rANS q
    const uint32_t *tw = reinterpret_cast<const uint32_t *>(ans_tab + (size_t)b * ANS_TAB_BYTES);
    uint32_t cost = 0;                                         // sum H cost <= 2^20 * 3072: 32 bits
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t s = 4 * lane + k, h = hist[(size_t)b * 256 + s];
        au.hist_s[(size_t)b * 256 + s] = is3 && s == fill ? h - (L - klen) : h;
        cost += h * auto_cost(ans_f(tw[s]));
    }
    cost = wave_sum(cost);
    if (lane) return;
    au.wa[b] = (uint32_t)auto_words_a(cost, L);
    sp.klen[b] = klen;
    sp.is3[b] = is3 ? 1u : 0u;
    sp.skip_table[b] = is3 && klen == 0 ? 1u : 0u;
    in_off[b] = (unsigned long long)(uintptr_t)(is3 ? K : data);
    in_len[b] = is3 ? klen : L;
}

__global__ __launch_bounds__(256) void k_au_choose(CtEncFrame f, CtEncHuff0 h, CtEncSparse sp, CtEncAns an, CtEncAuto au, uint32_t nb,
                                                   uint32_t blk_len)
{
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nb) return;
    const bool is3 = sp.is3[b] != 0;
    const unsigned long long klen = sp.klen[b];
    unsigned long long wS = is3 ? sp_mask_words(blk_len) + (klen ? h.nun[b] : 0ull) : h.nun[b];
    if (ct_stored_raw(wS, blk_len)) wS = ct_raw_words(blk_len);
    const bool pick5 = auto_pick5(au.wa[b], wS);
    if (!pick5 && is3) {                                       // the block stays kind 3: its table counts are K's
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) f.hist[(size_t)b * 256 + 4 * lane + k] = au.hist_s[(size_t)b * 256 + 4 * lane + k];
    }
    if (lane) return;
    au.pick5[b] = pick5 ? 1u : 0u;
    an.skip_ans[b] = pick5 ? 0u : 1u;
    sp.skip_move[b] = !pick5 && is3 ? 0u : 1u;
}

hipError_t ct_enc_auto_candidates(hipStream_t st, const SpSegs &g, const CtEncSparse &sp, const CtEncAuto &au, const uint32_t *hist,
                                  const uint8_t *ans_tab, unsigned long long *in_off, unsigned long long *in_len)
{
    hipLaunchKernelGGL(k_au_cand, dim3((g.count + 3) / 4), dim3(256), 0, st, g, sp, au, hist, ans_tab, in_off, in_len);
    return hipGetLastError();
}

hipError_t ct_enc_auto_choose(hipStream_t st, const CtEncFrame &f, const CtEncHuff0 &h, const CtEncSparse &sp, const CtEncAns &an,
                              const CtEncAuto &au, uint32_t nb, uint32_t blk_len)
{
    hipLaunchKernelGGL(k_au_choose, dim3((nb + 3) / 4), dim3(256), 0, st, f, h, sp, an, au, nb, blk_len);
    return hipGetLastError();
}

} // namespace glc
