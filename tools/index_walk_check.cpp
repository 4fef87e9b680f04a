// index_walk_check.cpp -- a stand-alone host program around ct_walk() (csrc/container_internal.h), the walk over a container's
// headers that the decoder, the frame index of a host buffer or file and k_ct_index all run.  It is meant to be built with
// the host sanitizers and run on the CPU; it touches no GPU:
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/index_walk_check.cpp -o index_walk_check && ./index_walk_check
// Every container lives in a heap buffer of exactly its length and the fetch callback copies straight out of it, so a header
// fetched from a position the walk failed to test against `len` is a heap overflow the sanitizer reports.
//   1. valid streams of several shapes: the walk ends with CT_OK and names every frame where it lies;
//   2. each of them cut at every multiple of 32 bytes (and one byte either side): refused, never read past the cut;
//   3. header words replaced by random values (stream header, frame headers, trailer; with and without a repaired header
//      CRC, so that the walk goes on with absurd sizes): any verdict is fine, a read outside the buffer is not.
#include "../gpu-lossless-compression_amd/csrc/container_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>

using namespace glc;

static const CrcTables T = crc_make_tables();

struct Shape { uint32_t version, flags, elem, block_len; std::vector<std::pair<uint32_t, uint32_t>> frames; };   // (nb, bl)

static void put(std::vector<uint8_t> &c, const uint32_t *w, size_t n) { const uint8_t *p = reinterpret_cast<const uint8_t *>(w); c.insert(c.end(), p, p + 4 * n); }

// header, frames (real headers, junk tables and payloads: the walk never looks at them) and trailer
static std::vector<uint8_t> make(const Shape &s, std::mt19937 &rng, std::vector<CtFrameRef> *refs)
{
    std::vector<uint8_t> c;
    unsigned long long total = 0;
    for (auto &f : s.frames) total += (unsigned long long)f.first * f.second;
    uint32_t h[8] = {CT_MAGIC_STREAM, s.version | (s.flags << 16), s.block_len, s.elem, (uint32_t)total, (uint32_t)(total >> 32), 0, 0};
    h[6] = crc32_bytes(T, h, 24);
    put(c, h, 8);
    unsigned long long done = 0;
    for (auto &f : s.frames) {
        const unsigned long long pw = rng() % ((unsigned long long)f.first * ct_raw_words(f.second) + 1);
        const uint32_t fh[8] = {CT_MAGIC_FRAME, f.first, f.second, 0, (uint32_t)pw, (uint32_t)(pw >> 32), (uint32_t)rng(), 0};
        refs->push_back(CtFrameRef{c.size(), done, pw, f.first, f.second});
        put(c, fh, 8);
        const unsigned long long rest = frame_bytes(f.first, f.second, pw) - CT_FRAME_HDR;
        for (unsigned long long i = 0; i < rest; i++) c.push_back((uint8_t)rng());
        done += (unsigned long long)f.first * f.second;
    }
    uint32_t t[4] = {CT_MAGIC_END, (uint32_t)s.frames.size(), (uint32_t)rng(), 0};
    t[3] = crc32_bytes(T, t, 12);
    put(c, t, 4);
    return c;
}

struct Walked { CtWalkEnd end; std::vector<CtFrameRef> frames; unsigned long long fetched = 0; };

// the walk over exactly len bytes on the heap
static Walked walk(const uint8_t *bytes, unsigned long long len, uint32_t plan_n, bool sparse)
{
    uint8_t *heap = static_cast<uint8_t *>(malloc(len ? len : 1));
    memcpy(heap, bytes, len);
    Walked w;
    w.end = ct_walk(
        T, len, plan_n, sparse,
        [&](uint32_t *dst, unsigned long long pos, uint32_t n, unsigned long long) { memcpy(dst, heap + pos, n); w.fetched += n; return true; },
        [&](const uint32_t *, const CtFormat &, uint32_t, unsigned long long) { return true; },
        [&](uint32_t fi, const uint32_t *, const CtFrameRef &r) { if (fi != w.frames.size()) abort(); w.frames.push_back(r); return true; },
        [&](const uint32_t *, uint32_t) { return true; });
    free(heap);
    return w;
}

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "index_walk_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
    std::mt19937 rng(20250);
    const std::vector<Shape> shapes = {
        {1, 0, 0, 4096, {}},                                                      // the empty input
        {1, 0, 0, 4096, {{8, 4096}, {8, 4096}, {2, 4096}, {1, 777}}},
        {3, 0, 4, 4096, {{3, 4096}, {1, 1}}},
        {5, 1, 8, 70000, {{2, 70000}, {1, 69999}}},
        {4, 1, 2, 512, {{1, 512}, {1, 512}, {1, 512}, {1, 512}, {1, 512}, {1, 3}}}};
    unsigned long long walks = 0;
    for (const Shape &s : shapes) {
        std::vector<CtFrameRef> refs;
        const std::vector<uint8_t> c = make(s, rng, &refs);
        // 1. valid
        Walked w = walk(c.data(), c.size(), 1u << 20, true);
        CHECK(w.end.what == CT_OK && w.end.frame == ~0ull && w.frames.size() == refs.size());
        for (size_t i = 0; i < refs.size(); i++)
            CHECK(w.frames[i].pos == refs[i].pos && w.frames[i].out_off == refs[i].out_off && w.frames[i].pw == refs[i].pw &&
                  w.frames[i].nb == refs[i].nb && w.frames[i].bl == refs[i].bl);
        CHECK(w.fetched == CT_HDR + CT_FRAME_HDR * refs.size() + CT_TRAILER);       // 32 bytes per frame and nothing else
        CHECK(walk(c.data(), c.size(), s.block_len, true).end.what == CT_OK);
        if (!s.frames.empty()) CHECK(walk(c.data(), c.size(), s.block_len - 1, true).end.what == CT_WALK_CONFIG);
        CHECK(walk(c.data(), c.size(), 1u << 20, false).end.what == (s.version >= 5 ? (uint32_t)CT_STREAM_HEADER : (uint32_t)CT_OK));
        // stray bytes behind the trailer
        std::vector<uint8_t> stray = c;
        stray.insert(stray.end(), 8, 0);
        w = walk(stray.data(), stray.size(), 1u << 20, true);
        CHECK(w.end.what == CT_STREAM_HEADER && w.end.frame == refs.size());
        // 2. truncated at every 32-byte step, and a byte either side
        for (unsigned long long cut = 0; cut < c.size(); cut += 32)
            for (long long d = -1; d <= 1; d++) {
                const long long L = (long long)cut + d;
                if (L < 0 || (unsigned long long)L >= c.size()) continue;
                w = walk(c.data(), (unsigned long long)L, 1u << 20, true);
                walks++;
                // a cut behind the last frame header leaves a shorter prefix that cannot end in a valid trailer
                CHECK(w.end.what == CT_TRUNCATED || w.end.what == CT_STREAM_HEADER || w.end.what == CT_FRAME_TABLE);
                CHECK(w.end.what != CT_TRUNCATED || w.end.frame == ~0ull || w.end.frame <= refs.size());
            }
        // 3. random header words
        std::vector<unsigned long long> hdrs = {0};
        for (auto &r : refs) hdrs.push_back(r.pos);
        hdrs.push_back(c.size() - CT_TRAILER);
        for (int it = 0; it < 4000; it++) {
            std::vector<uint8_t> x = c;
            const size_t hi = rng() % hdrs.size();
            const unsigned long long at = hdrs[hi];
            const uint32_t words = hi + 1 == hdrs.size() ? 4 : 8;
            uint32_t *hw = reinterpret_cast<uint32_t *>(x.data() + at);
            const int n = 1 + rng() % 3;
            for (int k = 0; k < n; k++) {
                const uint32_t v = (rng() & 1) ? (uint32_t)rng() : (1u << (rng() % 32)) - (uint32_t)(rng() & 1);
                hw[rng() % words] = v;
            }
            if (rng() & 1) {                                                     // repair the CRC: the walk takes the words for real
                if (at == 0) hw[6] = crc32_bytes(T, hw, 24);
                else if (words == 4) hw[3] = crc32_bytes(T, hw, 12);
            }
            w = walk(x.data(), x.size(), 1u << 20, true);
            walks++;
            CHECK(w.end.what <= CT_CAPACITY || w.end.what == CT_WALK_CONFIG);
        }
    }
    // fewer than 48 bytes of anything
    for (unsigned long long L = 0; L < CT_HDR + CT_TRAILER; L++) {
        std::vector<uint8_t> z(L + 1, 0xFF);
        CHECK(walk(z.data(), L, 4096, true).end.what == CT_TRUNCATED);
    }
    printf("index_walk_check: ok (%llu damaged walks)\n", walks);
    return 0;
}
