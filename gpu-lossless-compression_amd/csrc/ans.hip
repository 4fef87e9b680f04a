// ans.hip -- the rANS mode of the container's order-0 codec (record kind 5, format version 7).  gfx950 / wave64.
// A segment (a block of a frame) is cut into chunks of 32768 bytes; a chunk is coded by 64 interleaved 32-bit rANS states, lane
// l owning the symbols l, 64 + l, ... of the chunk, with 12-bit probabilities quantised from the segment's byte counts and
// 16-bit renormalisation units.  One wave codes one chunk; the four waves of a workgroup take four chunks of one segment and
// share its table in LDS.
//   k_ans_table   one wave per segment: counts -> q (four symbols a lane, the largest-q searches as wave reductions), cum, the
//                 divisor of every symbol and the 4096 slot -> symbol bytes
//   k_ans_encode  steps from the last down to 0.  The lanes that renormalise in a step come from a ballot, a lane's place among
//                 them from mbcnt; their units go downward into the chunk's scratch slot (2 bytes a symbol), so the slot's tail
//                 reads, upward, in the decoder's order.  Input comes through LDS in aligned 16-byte granules, 16 steps at a time
//   k_ans_place   behind the record offsets: counts, states and units of every chunk into its record
//   k_ans_decode  steps from 0 up: slot -> symbol, state update, then the lanes below 2^16 take the next units by ballot and
//                 mbcnt from a running position.  Symbols go through LDS and leave as aligned 16-byte granules, bytes at a
//                 segment's ragged ends.  There is no second pass.  The decoder is TOLERANT: whatever the record holds, a unit
//                 beyond the chunk's count (or the record's end) reads as 0, nothing is read outside the record's words and
//                 nothing written outside the segment.
// Any length up to 2^20, any byte alignment of the segments; records are word-aligned.  The container's own step (record sizes,
// the record rule) is k_ct_kind0 of container.hip.
#include "container_internal.h"
#include "glc_device.h"

namespace glc {

constexpr uint32_t ANS_THREADS = 256, ANS_WAVES = ANS_THREADS / WAVE, ANS_BATCH = 1024, ANS_STAGE = ANS_BATCH + 16;

__device__ __forceinline__ uint32_t ans_len(const AnsSegs &g, uint32_t i)
{
    const unsigned long long l = g.data_len[i];
    return l > g.max_len ? g.max_len : (uint32_t)l;
}
__device__ __forceinline__ uint8_t *ans_data(const AnsSegs &g, uint32_t i) { return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(g.data) + g.data_off[i]); }
__device__ __forceinline__ uint32_t *ans_tab_w(const AnsSegs &g, uint32_t i) { return reinterpret_cast<uint32_t *>(g.tab + (size_t)i * ANS_TAB_BYTES); }

// ---------------------------------------------------------------------------
// the table of a segment.  Whatever the counts hold the q come out summing to 4096 (counts that do not sum to the segment's
// length are the caller's mistake, not a hazard): q is clamped to 4096, the R < 0 loop ends within 256 rounds because every
// round brings the largest q down to 1 or R to 0, and all-zero counts give symbol 0 the whole range.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_ans_table(AnsSegs g)
{
    __shared__ uint32_t s_cum[257];
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (g.skip && g.skip[b]) return;
    const uint32_t n = ans_len(g, b);
    const uint32_t *h = g.hist + (size_t)b * 256;
    uint32_t q[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const unsigned long long c = h[4 * lane + k];
        const unsigned long long v = n ? c * ANS_M / n : 0ull;
        q[k] = c == 0 ? 0u : (uint32_t)(v < 1 ? 1ull : v > ANS_M ? (unsigned long long)ANS_M : v);
    }
    int R = (int)ANS_M - (int)wave_sum(q[0] + q[1] + q[2] + q[3]);
    // the largest q, the lowest symbol on a tie: the maximum of (q << 8 | 255 - symbol)
    auto largest = [&]() {
        uint32_t key = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) key = max(key, (q[k] << 8) | (255u - (4 * lane + k)));
        return wave_max(key);
    };
    if (R > 0) {
        const uint32_t s = 255u - (largest() & 255u);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (4 * lane + k == s) q[k] += (uint32_t)R;
    }
    for (uint32_t round = 0; round < 256 && R < 0; round++) {
        const uint32_t key = largest(), s = 255u - (key & 255u), top = key >> 8;
        const uint32_t t = min(top - 1u, (uint32_t)(-R));
        if (t == 0) break;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) if (4 * lane + k == s) q[k] -= t;
        R += (int)t;
    }
    const uint32_t mine = q[0] + q[1] + q[2] + q[3];
    uint32_t cum = wave_incl_add(mine) - mine;
    uint32_t *tw = ans_tab_w(g, b), *tm = tw + 256;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const AnsDiv d = ans_div_make(q[k] ? q[k] : 1u);
        const uint32_t c = min(cum, ANS_M - 1u);               // (cum = 4096 only behind the last symbol present)
        tw[4 * lane + k] = ans_pack(q[k], c, d.l);
        tm[4 * lane + k] = d.m;
        s_cum[4 * lane + k] = cum;
        cum += q[k];
    }
    if (lane == 63) s_cum[256] = cum;
    __builtin_amdgcn_wave_barrier();
    // slot k belongs to the last symbol whose cum is <= k (symbols without a slot share their cum with the next one)
    uint32_t *slots = reinterpret_cast<uint32_t *>(g.tab + (size_t)b * ANS_TAB_BYTES + 2048);
    for (uint32_t j = 0; j < 16; j++) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t slot = 64 * lane + 4 * j + k;
            uint32_t lo = 0, hi = 256;                         // cum[lo] <= slot < cum[hi]
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_cum[mid] <= slot) lo = mid; else hi = mid;
            }
            word |= lo << (8 * k);
        }
        slots[16 * lane + j] = word;
    }
}

// ---------------------------------------------------------------------------
// encoder.  Scratch of chunk slot (segment i, chunk c) = i * nch_max + c: ANS_CHUNK u16 of units (filled from the back), 64
// states, one count.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint16_t *ans_sc_units(const AnsScratch &s, size_t slot) { return s.units + slot * ANS_CHUNK; }

__global__ __launch_bounds__(ANS_THREADS) void k_ans_encode(AnsSegs g, AnsScratch sc)
{
    __shared__ uint32_t s_w[256], s_m[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[ANS_WAVES][ANS_STAGE];
    const uint32_t b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g.skip && g.skip[b]) return;
    const uint32_t L = ans_len(g, b), c = blockIdx.y * ANS_WAVES + wave;
    if (blockIdx.y * ANS_WAVES * ANS_CHUNK >= L) return;       // (the whole workgroup)
    const uint32_t *tw = ans_tab_w(g, b);
    s_w[threadIdx.x] = tw[threadIdx.x];
    s_m[threadIdx.x] = tw[256 + threadIdx.x];
    __syncthreads();
    if ((unsigned long long)c * ANS_CHUNK >= L) return;
    const uint32_t clen = min(ANS_CHUNK, L - c * ANS_CHUNK);
    const uint8_t *in = ans_data(g, b) + (size_t)c * ANS_CHUNK;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(in) & 15);
    uint8_t *stage = s_stage[wave];
    const size_t slot = (size_t)b * sc.nch_max + c;
    uint16_t *units = ans_sc_units(sc, slot);
    uint32_t x = ANS_L, ptr = ANS_CHUNK;
    const uint32_t nbatch = (clen + ANS_BATCH - 1) / ANS_BATCH;
    for (uint32_t bt = nbatch; bt-- > 0;) {
        const uint32_t B = bt * ANS_BATCH, bn = min(ANS_BATCH, clen - B);
        // the aligned granules that hold a byte of [in + B, + bn): stage[mis + k] = in[B + k]
        const uint8_t *a0 = in + B - mis;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t gr = lane; 16 * gr < mis + bn; gr += 64)
            reinterpret_cast<uint4 *>(stage)[gr] = *reinterpret_cast<const uint4 *>(a0 + 16 * gr);
        __builtin_amdgcn_wave_barrier();
        for (uint32_t t = (bn + 63) / 64; t-- > 0;) {
            const uint32_t k = t * 64 + lane;
            const bool active = k < bn;
            const uint32_t s = active ? stage[mis + k] : 0u;
            const uint32_t w = s_w[s], m = s_m[s];
            const bool emit = active && (x >> 20) >= ans_f(w);  // x >= f * 2^20 (never for f = 4096)
            const uint64_t bal = __ballot(emit);
            ptr -= (uint32_t)__popcll(bal);
            if (emit) { units[ptr + mbcnt(bal)] = (uint16_t)x; x >>= 16; }
            if (active) x = ans_put(x, w, m);
        }
    }
    sc.states[slot * ANS_LANES + lane] = x;
    if (lane == 0) sc.counts[slot] = ANS_CHUNK - ptr;
}

__global__ __launch_bounds__(256) void k_ans_words(AnsSegs g, AnsScratch sc, unsigned long long *words)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= g.count || (g.skip && g.skip[b])) return;
    words[b] = ans_words_of(sc.counts + (size_t)b * sc.nch_max, ans_chunks(ans_len(g, b)));
}

// one workgroup per chunk: the record's count word, its 64 states and its units, two to a word
__global__ __launch_bounds__(ANS_THREADS) void k_ans_place(AnsSegs g, AnsScratch sc, uint32_t *rec_base, const unsigned long long *rec_off,
                                                           unsigned long long cap_words)
{
    const uint32_t b = blockIdx.x, c = blockIdx.y;
    if (g.skip && g.skip[b]) return;
    const uint32_t nch = ans_chunks(ans_len(g, b));
    if (c >= nch) return;
    const uint32_t *counts = sc.counts + (size_t)b * sc.nch_max;
    const unsigned long long o = rec_off[b];
    if (o + ans_words_of(counts, nch) > cap_words) return;
    unsigned long long so = nch;
    for (uint32_t k = 0; k < c; k++) so += ANS_LANES + (min(counts[k], ANS_CHUNK) + 1) / 2;
    uint32_t *rec = rec_base + o;
    const size_t slot = (size_t)b * sc.nch_max + c;
    const uint32_t nu = min(counts[c], ANS_CHUNK);
    if (threadIdx.x == 0) rec[c] = nu;
    if (threadIdx.x < ANS_LANES) rec[so + threadIdx.x] = sc.states[slot * ANS_LANES + threadIdx.x];
    const uint16_t *u = ans_sc_units(sc, slot) + (ANS_CHUNK - nu);
    for (uint32_t j = threadIdx.x; j < (nu + 1) / 2; j += ANS_THREADS)
        rec[so + ANS_LANES + j] = (uint32_t)u[2 * j] | (2 * j + 1 < nu ? (uint32_t)u[2 * j + 1] << 16 : 0u);
}

// ---------------------------------------------------------------------------
// decoder.  rec = rec_base + rec_off[b], W = its words (rec_len[b], or rec_off[b + 1] - rec_off[b] without rec_len).  Every
// index into rec is tested against W first; counts are clamped to a chunk's symbols, so the offsets stay small.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(ANS_THREADS) void k_ans_decode(AnsSegs g, const uint32_t *rec_base, const unsigned long long *rec_off,
                                                            const unsigned long long *rec_len)
{
    __shared__ uint32_t s_w[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_slot[ANS_M];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[ANS_WAVES][ANS_STAGE];
    const uint32_t b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (g.skip && g.skip[b]) return;
    const uint32_t L = ans_len(g, b), c = blockIdx.y * ANS_WAVES + wave;
    if (blockIdx.y * ANS_WAVES * ANS_CHUNK >= L) return;       // (the whole workgroup)
    const uint32_t *tw = ans_tab_w(g, b);
    s_w[threadIdx.x] = tw[threadIdx.x];
    reinterpret_cast<uint4 *>(s_slot)[threadIdx.x] = reinterpret_cast<const uint4 *>(tw + 512)[threadIdx.x];
    __syncthreads();
    if ((unsigned long long)c * ANS_CHUNK >= L) return;
    const uint32_t clen = min(ANS_CHUNK, L - c * ANS_CHUNK), nch = ans_chunks(L);
    const unsigned long long lo = rec_off[b], hi = rec_len ? lo + rec_len[b] : rec_off[b + 1];
    const unsigned long long W = hi > lo ? hi - lo : 0ull;
    const uint32_t *rec = rec_base + lo;
    // where the chunk's states start: the counts of the chunks in front of it, one a lane (nch <= 32)
    const uint32_t before = lane < c && lane < W ? ANS_LANES + (min(rec[lane], ANS_CHUNK) + 1) / 2 : 0u;
    const unsigned long long so = nch + wave_sum(before);     // <= 32 + 32 * (64 + 16384)
    uint32_t x = so + lane < W ? rec[so + lane] : ANS_L;
    const unsigned long long uo = so + ANS_LANES;              // the chunk's units, two to a word
    const uint32_t stored = c < W ? min(rec[c], ANS_CHUNK) : 0u;
    const uint32_t avail = uo < W ? (uint32_t)min((unsigned long long)stored, 2 * (W - uo)) : 0u;
    const uint16_t *units = reinterpret_cast<const uint16_t *>(rec + (uo < W ? uo : 0ull));
    uint8_t *out = ans_data(g, b) + (size_t)c * ANS_CHUNK;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15);
    uint8_t *stage = s_stage[wave];
    uint32_t pos = 0;
    const uint32_t nbatch = (clen + ANS_BATCH - 1) / ANS_BATCH;
    for (uint32_t bt = 0; bt < nbatch; bt++) {
        const uint32_t B = bt * ANS_BATCH, bn = min(ANS_BATCH, clen - B);
        for (uint32_t t = 0; t < (bn + 63) / 64; t++) {
            const uint32_t k = t * 64 + lane;
            const bool active = k < bn;
            bool need = false;
            if (active) {
                const uint32_t slot = x & (ANS_M - 1u), s = s_slot[slot], w = s_w[s];
                stage[mis + k] = (uint8_t)s;
                x = ans_f(w) * (x >> ANS_PROB_BITS) + slot - ans_c(w);
                need = x < ANS_L;
            }
            const uint64_t bal = __ballot(need);
            if (need) {
                const uint32_t idx = pos + mbcnt(bal);
                x = (x << 16) | (idx < avail ? (uint32_t)units[idx] : 0u);
            }
            pos += (uint32_t)__popcll(bal);
        }
        __builtin_amdgcn_wave_barrier();
        // stage[0 .. mis) is the carry of the batch before (the chunk's first batch: not ours), stage[mis .. mis + bn) this
        // batch's.  Whole granules leave as 16 bytes; the last batch also flushes what would have been its carry.
        const bool last = bt + 1 == nbatch;
        const uint32_t from = bt == 0 ? mis : 0u, to = last ? mis + bn : ANS_BATCH;
        uint8_t *a0 = out + B - mis;                           // 16-byte aligned
        for (uint32_t gr = lane; 16 * gr < to; gr += 64) {
            const uint32_t glo = 16 * gr, ghi = glo + 16;
            if (glo >= from && ghi <= to) *reinterpret_cast<uint4 *>(a0 + glo) = reinterpret_cast<const uint4 *>(stage)[gr];
            else for (uint32_t k = max(glo, from); k < min(ghi, to); k++) a0[k] = stage[k];
        }
        if (!last) {
            __builtin_amdgcn_wave_barrier();
            const uint8_t carry = lane < mis ? stage[ANS_BATCH + lane] : (uint8_t)0;
            __builtin_amdgcn_wave_barrier();
            if (lane < mis) stage[lane] = carry;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

hipError_t ans_tables(hipStream_t st, const AnsSegs &g)
{
    if (g.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ans_table, dim3(g.count), dim3(WAVE), 0, st, g);
    return hipGetLastError();
}

static dim3 ans_grid(const AnsSegs &g) { return dim3(g.count, (ans_chunks(g.max_len) + ANS_WAVES - 1) / ANS_WAVES); }

hipError_t ans_encode(hipStream_t st, const AnsSegs &g, const AnsScratch &sc)
{
    if (g.count == 0 || g.max_len == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ans_encode, ans_grid(g), dim3(ANS_THREADS), 0, st, g, sc);
    return hipGetLastError();
}

hipError_t ans_words(hipStream_t st, const AnsSegs &g, const AnsScratch &sc, unsigned long long *words)
{
    if (g.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ans_words, dim3((g.count + 255) / 256), dim3(256), 0, st, g, sc, words);
    return hipGetLastError();
}

hipError_t ans_place(hipStream_t st, const AnsSegs &g, const AnsScratch &sc, uint32_t *rec_base, const unsigned long long *rec_off,
                     unsigned long long cap_words)
{
    if (g.count == 0 || g.max_len == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ans_place, dim3(g.count, ans_chunks(g.max_len)), dim3(ANS_THREADS), 0, st, g, sc, rec_base, rec_off, cap_words);
    return hipGetLastError();
}

hipError_t ans_decode(hipStream_t st, const AnsSegs &g, const uint32_t *rec_base, const unsigned long long *rec_off,
                      const unsigned long long *rec_len)
{
    if (g.count == 0 || g.max_len == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ans_decode, ans_grid(g), dim3(ANS_THREADS), 0, st, g, rec_base, rec_off, rec_len);
    return hipGetLastError();
}

} // namespace glc
