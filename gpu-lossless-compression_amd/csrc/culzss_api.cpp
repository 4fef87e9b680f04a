// culzss_api.cpp -- the C ABI of include/culzss.h.
//
// Mirrors the wrapper layer of the reference (cuda-lzss-cluster/gpu_compress.cu:352-460,
// 569-670; gpu_decompress.cu:98-118,247-358): same symbols, argument meaning and
// return values, called from the reference's pthread pipeline (culzss.c:85-86,108,
// 133-134,170,176; deculzss.c:78-79,98,119-120) on different threads ("launch on
// thread A, wait on thread B"), so all shared state sits behind the locks tabulated above State.
//
// Differences, all deliberate: token selection/packing runs on the GPU inside the
// compression stream instead of on a CPU thread (aftercomp, gpu_compress.cu:462-566);
// device scratch is cached per ring slot instead of cudaMalloc/cudaFree per call
// (gpu_decompress.cu:306-349); HIP errors are reported by return value 0 rather
// than exit() (gpu_compress.cu:170-179).
#include "../../include/culzss.h"
#include "culzss_internal.h"
#include "glc_internal.h"

#include <algorithm>
#include <array>
#include <memory>
#include <mutex>
#include <new>
#include <stdio.h>
#include <string.h>

// host clock around the four phases of compression_kernel_wrapper: nothing without the switch
#ifdef GLC_LZ_HOSTTRACE
#include <time.h>
namespace {
struct HostTrace {
    double t[5];
    int n = 0;
    void mark() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); t[n++] = ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; }
    void print(int index) const { fprintf(stderr, "wrapper slot %d: H2D %.0f us, kernels %.0f us, D2H cand %.0f us, D2H size %.0f us\n", index, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3]); }
};
} // namespace
#else
namespace { struct HostTrace { void mark() {} void print(int) const {} }; }
#endif

using namespace glc;

namespace {

constexpr int NSLOTS = 4;                       // ring slots of the reference queue (culzss.c:273-346)

bool ok(hipError_t e, const char *what)
{
    if (e == hipSuccess) return true;
    fprintf(stderr, "culzss (hip): %s: %s\n", what, hipGetErrorString(e));
    return false;
}

// One row per buffer of a slot, a group or the decode scratch.  The owner's list is walked to allocate (rows of 0 bytes are
// left out) and walked again to release, so what is freed is what was allocated.
struct Mem { void **p; size_t bytes; bool pinned; const char *what; };

template <class List> void mem_release(const List &list)
{
    for (const Mem &m : list) {
        if (*m.p) (void)(m.pinned ? hipHostFree(*m.p) : hipFree(*m.p));
        *m.p = nullptr;
    }
}

template <class List> bool mem_alloc(const List &list)
{
    for (const Mem &m : list)
        if (m.bytes && !ok(m.pinned ? glc_host_alloc(m.p, m.bytes) : glc_dev_alloc(m.p, m.bytes), m.what)) return false;
    return true;
}

// grow-only scratch: `list` sized for `want`, `cap` what it holds now (0 after a failure: the next call starts over)
template <class List> bool mem_ensure(int &cap, int want, const List &list)
{
    if (cap >= want) return true;
    mem_release(list);
    cap = mem_alloc(list) ? want : 0;
    return cap != 0;
}

struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int cap = 0;                                // buf_length the scratch below was sized for
    uint8_t *d_packed = nullptr;
    uint8_t *d_in = nullptr, *d_cand = nullptr; // the slot's own input / candidate buffers (see compression_kernel_wrapper)
    int *d_size = nullptr;
    void *d_work = nullptr;
    uint8_t *h_packed = nullptr;                // pinned
    int *h_size = nullptr;                      // pinned
    const unsigned char *key = nullptr;         // host candidate buffer of the in-flight call
    int len = 0;
    bool valid = false;
    // One lock per ring slot: the reference's callers run a producer, a GPU thread and a CPU thread on DIFFERENT slots
    // at the same time (culzss.c:85-176); under one global lock the launch of slot k + 1 (a dozen HIP calls) waited for
    // the copy-out of slot k.
    std::mutex mu;
};

// the scratch of a slot sized for buf_length (the sizes do not matter to a release)
std::array<Mem, 7> slot_mem(Slot &s, int buf_length)
{
    const size_t stride = lzss_pack_stride(buf_length);
    return {{{(void **)&s.d_packed, stride, false, "slot packed"},
             {(void **)&s.d_in, (size_t)buf_length, false, "slot in"},
             {(void **)&s.d_cand, (size_t)2 * buf_length, false, "slot candidates"},
             {(void **)&s.d_size, 16, false, "slot size"},                      // (leaves as one 16-byte piece: lzss_copy_to_host)
             {&s.d_work, lzss_work_bytes(buf_length, 1), false, "slot work"},
             {(void **)&s.h_packed, stride, true, "slot pinned"},
             {(void **)&s.h_size, 16, true, "slot pinned size"}}};
}

// (the tracking entry {valid, key, len} is read and written under g.mu only: the teardown clears it, the wrapper drops it
//  before it reuses a slot)
void slot_release(Slot &s) { mem_release(slot_mem(s, 0)); s.cap = 0; }
bool slot_ensure(Slot &s, int buf_length) { return mem_ensure(s.cap, buf_length, slot_mem(s, buf_length)); }

bool slot_create(Slot &s)
{
    return ok(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking), "slot stream") &&
           ok(hipEventCreate(&s.e0), "slot event") && ok(hipEventCreate(&s.e1), "slot event");
}

void slot_destroy(Slot &s, bool wait)
{
    if (wait && s.stream) (void)hipStreamSynchronize(s.stream);
    slot_release(s);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    if (s.e0) (void)hipEventDestroy(s.e0);
    if (s.e1) (void)hipEventDestroy(s.e1);
    s.stream = nullptr; s.e0 = s.e1 = nullptr; s.key = nullptr; s.len = 0; s.valid = false;
}

// what decompression_kernel_wrapper decodes in: one packed buffer in, one buffer out, {size, error word}
struct LzDecodeScratch {
    uint8_t *in = nullptr, *out = nullptr;
    int *size = nullptr;
    int cap = 0;                                // the original length this was sized for

    std::array<Mem, 3> mem(int orig)
    {
        return {{{(void **)&in, lzss_pack_stride(orig), false, "decode in"},
                 {(void **)&out, (size_t)orig, false, "decode out"},
                 {(void **)&size, 2 * sizeof(int), false, "decode size"}}};
    }
    bool ensure(int orig) { return mem_ensure(cap, orig, mem(orig)); }
    void release() { mem_release(mem(0)); cap = 0; }
};

// Which lock an entry point holds while it does what.  g.mu guards `inited`, the choice of a slot and every slot's tracking
// entry {valid, key, len}; a slot's mu guards that slot's stream, events and scratch.  No cycle: a RING slot's mu is never
// taken under g.mu (the wrapper takes g.mu under it, to publish three words); the SCRATCH slot's mu is, and takes nothing.
//   compression_kernel_wrapper             g.mu for the slot lookup (init; drops the tracking entry) and again to publish the
//                                          new entry; the ring slot's mu across the work: wait, regrow, copies, kernels
//   onestream_finish_GPU                   g.mu for the slot lookup (init); waits on the stream under no lock
//   aftercompression_wrapper               g.mu for the lookup of the entry (init); then the tracked slot's mu (wait, copy
//                                          out) or, untracked, the scratch slot's mu (the whole packing) -- not g.mu
//   decompression_kernel_wrapper,          g.mu across the whole call, the scratch slot's mu inside it (culzss_decompress:
//   culzss_compress                        inside the wrapper it calls)
//   culzss_container_compress/_decompress  g.mu across the whole call; streams of their own, no slot
//   initGPU, glcLzssLastKernelMs           g.mu across the whole call
//   deleteGPUStreams, resetGPU             g.mu only: the caller must have quiesced every thread that uses a slot
struct State {
    std::mutex mu;
    bool inited = false;
    Slot slot[NSLOTS + 1];                      // +1: scratch slot for stand-alone packing / conveniences
    LzDecodeScratch dd;                           // runs on the scratch slot's stream
} g;

// All streams and events, or none: after a failed creation nothing is left behind and `inited` stays false, so every entry
// point fails (0) until a later call gets them all.
bool init_locked()
{
    if (g.inited) return true;
    // the reference pins device 0 (gpu_compress.cu:395); here the streams belong to whatever device is current
    // in the calling thread, so one process per GPU (rank r on device r) works without HIP_VISIBLE_DEVICES
    for (auto &s : g.slot)
        if (!slot_create(s)) {
            for (auto &t : g.slot) slot_destroy(t, false);
            return false;
        }
    g.inited = true;
    return true;
}

void teardown_locked(bool wait)
{
    for (auto &s : g.slot) slot_destroy(s, wait);
    g.dd.release();
    g.inited = false;
}

Slot &slot_at(int index) { return g.slot[((index % NSLOTS) + NSLOTS) % NSLOTS]; }

// is [p, p + bytes) pinned host memory the device can write (hipHostMalloc / initCPUmem) and 16-byte aligned?
bool host_mapped(const void *p, size_t bytes)
{
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    // the kernel is handed p itself: only memory whose device address IS its host address (hipHostMalloc on this platform) -- a
    // registered or otherwise mapped range with another device address takes the copy-engine path
    if (a.type != hipMemoryTypeHost || a.devicePointer != p) return false;
    hipPointerAttribute_t b;                                   // ... to its last byte
    const void *last = (const char *)p + bytes - 1;
    if (hipPointerGetAttributes(&b, last) != hipSuccess) { (void)hipGetLastError(); return false; }
    return b.type == hipMemoryTypeHost && b.devicePointer == last;
}

bool valid_len(int n) { return n > 0 && n % GLC_LZSS_PACKET == 0 && n <= GLC_LZSS_MAX_BUF; }

// The trailer of a packed buffer (gpu_decompress.cu:257-270): the original length, big-endian, in bytes -6..-3 and the
// padding in -2..-1.  Only the layout is read here; what lengths a caller accepts is the caller's rule.
bool parse_trailer(const unsigned char *p, size_t len, int *orig, int *pad)
{
    if (len < 6) return false;
    const unsigned char *t = p + len - 6;
    *orig = (int)(((unsigned)t[0] << 24) | ((unsigned)t[1] << 16) | ((unsigned)t[2] << 8) | (unsigned)t[3]);
    *pad = (int)(((unsigned)t[4] << 8) | (unsigned)t[5]);
    return true;
}

// Host bytes in -> lzss_encode (a buffer) or lzss_pack (its 2 B/B candidate stream) on the scratch slot -> packed bytes in
// dst and their count in *size.  0: a HIP call failed; 2: the packed form "took more", dst and *size are untouched and the
// caller stores the buffer raw; 1 otherwise.
int scratch_pack(const unsigned char *src, int buf_length, bool candidates, unsigned char *dst, int *size)
{
    Slot &s = g.slot[NSLOTS];
    std::lock_guard<std::mutex> lk(s.mu);
    if (!slot_ensure(s, buf_length)) return 0;
    const size_t bytes = candidates ? (size_t)2 * buf_length : (size_t)buf_length;
    uint8_t *d_src = nullptr;
    if (!ok(glc_dev_alloc((void **)&d_src, bytes), "scratch upload")) return 0;
    const bool good = ok(hipMemcpyAsync(d_src, src, bytes, hipMemcpyHostToDevice, s.stream), "H2D")
                   && (candidates ? ok(lzss_pack(s.stream, d_src, buf_length, 1, s.d_packed, s.d_size, s.d_work), "pack")
                                  : ok(lzss_encode(s.stream, d_src, buf_length, 1, nullptr, s.d_packed, s.d_size, s.d_work), "encode"))
                   && ok(hipMemcpyAsync(s.h_packed, s.d_packed, lzss_pack_stride(buf_length), hipMemcpyDeviceToHost, s.stream), "D2H")
                   && ok(hipMemcpyAsync(s.h_size, s.d_size, sizeof(int), hipMemcpyDeviceToHost, s.stream), "D2H size")
                   && ok(hipStreamSynchronize(s.stream), "sync");
    (void)hipFree(d_src);
    if (!good) return 0;
    if (*s.h_size <= 0) return 2;
    memcpy(dst, s.h_packed, (size_t)*s.h_size);
    *size = *s.h_size;
    return 1;
}

using Bytes = std::unique_ptr<unsigned char[]>;
Bytes bytes_new(size_t n) { return Bytes(new (std::nothrow) unsigned char[n ? n : 1]); }

} // namespace

extern "C" {

void initGPU(void)
{
    std::lock_guard<std::mutex> lk(g.mu);
    (void)init_locked();
}

void resetGPU(void)
{
    std::lock_guard<std::mutex> lk(g.mu);
    teardown_locked(false);
    (void)hipDeviceReset();
}

int streams_in_GPU(void) { return 1; }

void deleteGPUStreams(void)
{
    std::lock_guard<std::mutex> lk(g.mu);
    teardown_locked(true);
}

void signalExitThreads(void) {}

unsigned char *initGPUmem(int buf_length)
{
    void *p = nullptr;
    if (buf_length <= 0 || !ok(glc_dev_alloc(&p, (size_t)buf_length), "initGPUmem")) return nullptr;
    return (unsigned char *)p;
}

unsigned char *initCPUmem(int buf_length)
{
    void *p = nullptr;
    if (buf_length <= 0 || !ok(glc_host_alloc(&p, (size_t)buf_length), "initCPUmem")) return nullptr;
    return (unsigned char *)p;
}

void deleteGPUmem(unsigned char *mem_d) { if (mem_d) (void)hipFree(mem_d); }
void deleteCPUmem(unsigned char *mem_d) { if (mem_d) (void)hipHostFree(mem_d); }
unsigned char *deinitGPUmem(int buf_length) { return initGPUmem(buf_length); }
void dedeleteGPUmem(unsigned char *mem_d) { deleteGPUmem(mem_d); }
void deinitGPU(void) { (void)hipSetDevice(0); }

int compression_kernel_wrapper(unsigned char *buffer, int buf_length, unsigned char *compressed_buffer,
                               int /*compression_type*/, int /*wsize*/, int /*numthre*/, int /*nstreams*/,
                               int index, unsigned char *in_d, unsigned char *out_d)
{
    if (!buffer || !compressed_buffer || !in_d || !out_d || !valid_len(buf_length)) return 0;
    Slot *sp;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (!init_locked()) return 0;
        sp = &slot_at(index);
        sp->valid = false;                         // the slot is taken again: what it tracked is gone (written under g.mu, as it is read)
    }
    Slot &s = *sp;
    std::lock_guard<std::mutex> lk(s.mu);
    (void)hipStreamSynchronize(s.stream);          // slot reuse: previous call on this slot must be done
    if (!slot_ensure(s, buf_length)) return 0;
    hipStream_t st = s.stream;
    // The reference's pipeline hands EVERY ring slot the same in_d / out_d (culzss.c:85-86,108) and queues the slots
    // on different streams without waiting (gpu_compress.cu:426-460): slot s+1's copy-in can overwrite what slot
    // s's kernel is still reading.  The caller's device buffers are therefore accepted but not used: each slot
    // stages through buffers of its own.
    (void)in_d; (void)out_d;
    HostTrace trace;
    trace.mark();
    if (!ok(hipMemcpyAsync(s.d_in, buffer, (size_t)buf_length, hipMemcpyHostToDevice, st), "H2D")) return 0;
    trace.mark();
    (void)hipEventRecord(s.e0, st);
    if (!ok(lzss_encode(st, s.d_in, buf_length, 1, s.d_cand, s.d_packed, s.d_size, s.d_work), "encode")) return 0;
    (void)hipEventRecord(s.e1, st);
    trace.mark();
    // what leaves the device here: the candidate stream (the interface's compressed_buffer: 2 B per input byte) and the
    // packed size.  The packed bytes stay in the slot until aftercompression_wrapper knows how many there are and copies
    // exactly those, straight into the caller's buffer (a whole-slot copy into pinned staging + a host memcpy were
    // 1 MiB more over PCIe and ~60 us of the CPU thread per buffer).
    if (host_mapped(compressed_buffer, (size_t)2 * buf_length)) {
        // pinned (initCPUmem, as the reference's callers allocate it): written by a kernel -- see k_lzss_to_host
        if (!ok(lzss_copy_to_host(st, s.d_cand, compressed_buffer, (size_t)2 * buf_length), "candidates to host")) return 0;
    } else if (!ok(hipMemcpyAsync(compressed_buffer, s.d_cand, (size_t)2 * buf_length, hipMemcpyDeviceToHost, st), "D2H cand")) return 0;
    trace.mark();
    if (!ok(lzss_copy_to_host(st, s.d_size, s.h_size, 16), "size to host")) return 0;
    trace.mark();
    trace.print(index);
    {
        std::lock_guard<std::mutex> lg(g.mu);
        s.key = compressed_buffer; s.len = buf_length; s.valid = true;
    }
    return 1;
}

int onestream_finish_GPU(int index)
{
    hipStream_t st;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (!init_locked()) return 0;
        st = slot_at(index).stream;
    }
    return ok(hipStreamSynchronize(st), "stream sync") ? 1 : 0;
}

int aftercompression_wrapper(unsigned char *buffer, int buf_length, unsigned char *bufferout, int *comp_length)
{
    if (!buffer || !bufferout || !comp_length || !valid_len(buf_length)) return 0;
    Slot *hit = nullptr;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        if (!init_locked()) return 0;
        for (int i = 0; i < NSLOTS; i++)
            if (g.slot[i].valid && g.slot[i].key == bufferout && g.slot[i].len == buf_length) { hit = &g.slot[i]; hit->valid = false; }
    }
    // candidates that did not come from a tracked call: pack them on the GPU now ("took more": the caller stores the buffer raw)
    if (!hit) return scratch_pack(bufferout, buf_length, true, buffer, comp_length) == 1 ? 1 : 0;
    std::lock_guard<std::mutex> lk(hit->mu);
    if (!ok(hipStreamSynchronize(hit->stream), "sync")) return 0;
    const int size = *hit->h_size;
    if (size <= 0) return 0;                        // "compression took more": caller stores the buffer raw (untouched)
    if (!ok(hipMemcpyAsync(buffer, hit->d_packed, (size_t)size, hipMemcpyDeviceToHost, hit->stream), "D2H packed") ||
        !ok(hipStreamSynchronize(hit->stream), "sync")) return 0;
    *comp_length = size;
    return 1;
}

int decompression_kernel_wrapper(unsigned char *buffer, int buf_length, int *decomp_length,
                                 int /*compression_type*/, int /*wsize*/, int /*numthre*/)
{
    if (!buffer || !decomp_length || buf_length < 8) return 0;
    int orig, pad;
    if (!parse_trailer(buffer, (size_t)buf_length, &orig, &pad)) return 0;
    if (!valid_len(orig) || pad < 0 || pad > orig || buf_length < 2 * (orig / GLC_LZSS_PACKET) + 6) return 0;
    std::lock_guard<std::mutex> lk(g.mu);
    if (!init_locked()) return 0;
    std::lock_guard<std::mutex> ls(g.slot[NSLOTS].mu);        // (the scratch slot's stream: shared with the untracked packing path)
    LzDecodeScratch &dd = g.dd;
    if (!dd.ensure(orig)) return 0;
    if ((size_t)buf_length > lzss_pack_stride(orig)) return 0;
    hipStream_t st = g.slot[NSLOTS].stream;
    int hdr[2] = {buf_length, 0}, err = 0;                     // {size, error word}
    bool good = ok(hipMemcpyAsync(dd.in, buffer, (size_t)buf_length, hipMemcpyHostToDevice, st), "H2D")
             && ok(hipMemcpyAsync(dd.size, hdr, sizeof hdr, hipMemcpyHostToDevice, st), "H2D size")
             && ok(hipStreamSynchronize(st), "sync")       // hdr is a stack variable
             && ok(lzss_decode(st, dd.in, dd.size, orig, 1, dd.out, dd.size + 1), "decode")
             && ok(hipMemcpyAsync(&err, dd.size + 1, sizeof(int), hipMemcpyDeviceToHost, st), "D2H err")
             && ok(hipStreamSynchronize(st), "sync");
    if (!good || err) return 0;                             // malformed stream: nothing is written back
    good = ok(hipMemcpyAsync(buffer, dd.out, (size_t)(orig - pad), hipMemcpyDeviceToHost, st), "D2H")
        && ok(hipStreamSynchronize(st), "sync");
    if (!good) return 0;
    *decomp_length = orig - pad;
    return 1;
}

// --------------------------------------------------------------------------
// conveniences
// --------------------------------------------------------------------------
int culzss_compress(const unsigned char *in, int len, unsigned char *out, int *out_len)
{
    if (!in || !out || !out_len || !valid_len(len)) return 0;
    std::lock_guard<std::mutex> lk(g.mu);
    if (!init_locked()) return 0;
    const int rc = scratch_pack(in, len, false, out, out_len);
    if (rc == 2) { memcpy(out, in, (size_t)len); *out_len = len; }
    return rc;
}

int culzss_decompress(const unsigned char *in, int len, unsigned char *out, int *out_len)
{
    if (!in || !out || !out_len || len < 8) return 0;
    int orig, pad;
    if (!parse_trailer(in, (size_t)len, &orig, &pad)) return 0;
    if (!valid_len(orig) || (size_t)len > lzss_pack_stride(orig)) return 0;
    Bytes tmp = bytes_new(std::max(lzss_pack_stride(orig), (size_t)orig));   // the wrapper decodes in place
    if (!tmp) return 0;
    memcpy(tmp.get(), in, (size_t)len);
    int n = 0;
    const int rc = decompression_kernel_wrapper(tmp.get(), len, &n, 0, 1, 1);
    if (rc == 1) { memcpy(out, tmp.get(), (size_t)n); *out_len = n; }
    return rc;
}

// --------------------------------------------------------------------------
// device-resident batch API
// --------------------------------------------------------------------------
unsigned long long glcLzssPackStride(int buf_length)
{
    return valid_len(buf_length) ? (unsigned long long)lzss_pack_stride(buf_length) : 0ull;
}

unsigned long long glcLzssWorkBytes(int buf_length, int nbuf)
{
    if (!valid_len(buf_length) || nbuf <= 0) return 0;
    return (unsigned long long)lzss_work_bytes(buf_length, nbuf);
}

int glcLzssEncodeDevice(const unsigned char *d_in, int buf_length, int nbuf, unsigned char *d_cand,
                        unsigned char *d_packed, int *d_sizes, void *d_work, void *stream)
{
    if (!d_in || !d_packed || !d_sizes || !d_work || !valid_len(buf_length) || nbuf <= 0) return 0;
    return ok(lzss_encode((hipStream_t)stream, d_in, buf_length, nbuf, d_cand, d_packed, d_sizes, d_work), "encode") ? 1 : 0;
}

int glcLzssDecodeDevice(const unsigned char *d_packed, const int *d_sizes, int buf_length, int nbuf,
                        unsigned char *d_out, void *stream)
{
    if (!d_packed || !d_sizes || !d_out || !valid_len(buf_length) || nbuf <= 0) return 0;
    return ok(lzss_decode((hipStream_t)stream, d_packed, d_sizes, buf_length, nbuf, d_out), "decode") ? 1 : 0;
}

int glcLzssEnableProfile(int on)
{
    KernelProf &pr = lzss_prof();
    (void)hipDeviceSynchronize();
    pr.collect();
    pr.reset();
    return pr.enable(on != 0) ? 1 : 0;
}

int glcLzssKernelProfile(int index, char *name, size_t nameCap, double *out3)
{
    return global_prof_get(lzss_prof(), LZP_NSLOT, index, name, nameCap, out3);
}

float glcLzssLastKernelMs(void)
{
    std::lock_guard<std::mutex> lk(g.mu);
    float best = 0.f;
    for (int i = 0; i < NSLOTS; i++) {
        float ms = 0.f;
        if (g.slot[i].e0 && hipEventElapsedTime(&ms, g.slot[i].e0, g.slot[i].e1) == hipSuccess && ms > best) best = ms;
    }
    return best;
}

} // extern "C"

// ==========================================================================
// Container + pipeline: the file format written by the
// reference's pthread pipeline (cuda-lzss-cluster/main.c:236-245, culzss.c:204-269,
// decompression.c:66-173, deculzss.c:125-180):
//     u32 nbufs | u32 padding | u32 cumulative_size[nbufs] | payload_0 | payload_1 ...
// (host-endian u32, as fwrite'd by culzss.c:220,263-264).  payload_i is the packed
// form of 1 MiB buffer i, or the raw buffer when packing "took more"
// (size == BUFSIZE, culzss.c:241-242; recognised by deculzss.c:94-95).  `padding`
// = bytes missing from the last buffer.  One deliberate fix: the reference
// compresses the last partial buffer together with stale bytes of the ring slot
// (main.c:122-130), so its bytes are run-dependent; here the tail is zero-filled.
//
// The reference overlaps file I/O, PCIe and the GPU with four pthreads and a
// 4-slot ledger.  Here PCIe and the GPU overlap through two HIP streams working on
// alternating groups of buffers (copy-in / kernels / copy-out of group g+1 run
// while the host assembles group g) -- no thread ring, no busy-wait on
// cudaStreamQuery (gpu_compress.cu:415-424).  File I/O is NOT overlapped: the
// *_file functions read the whole input and hold the whole output in memory
// (inputs are bounded by the 4 GiB - 1 payload limit of the u32 offsets anyway).
// ==========================================================================
namespace {

constexpr int CBUF = 1 << 20;                   // BUFSIZE (main.c:62)
constexpr int GROUP = 16;                       // buffers per in-flight group

struct Group {
    hipStream_t st = nullptr;
    uint8_t *d_in = nullptr, *d_packed = nullptr, *h_in = nullptr, *h_packed = nullptr;
    int *d_sizes = nullptr, *h_sizes = nullptr; // GROUP sizes + one error word
    void *d_work = nullptr;
    uint8_t *d_out = nullptr, *h_out = nullptr;  // decode side
    int nbuf = 0;
    size_t first = 0;
};

// a group's buffers; the rows of the other direction have 0 bytes (the sizes do not matter to a release)
std::array<Mem, 9> group_mem(Group &G, bool decode)
{
    const size_t stride = lzss_pack_stride(CBUF), enc = decode ? 0 : 1, dec = decode ? 1 : 0;
    return {{{(void **)&G.d_packed, stride * GROUP, false, "group packed"},
             {(void **)&G.d_sizes, sizeof(int) * (GROUP + 1), false, "group sizes"},
             {(void **)&G.h_packed, stride * GROUP, true, "group h_packed"},
             {(void **)&G.h_sizes, sizeof(int) * (GROUP + 1), true, "group h_sizes"},
             {(void **)&G.d_in, enc * CBUF * GROUP, false, "group in"},
             {(void **)&G.h_in, enc * CBUF * GROUP, true, "group h_in"},
             {&G.d_work, enc * lzss_work_bytes(CBUF, GROUP), false, "group work"},
             {(void **)&G.d_out, dec * CBUF * GROUP, false, "group out"},
             {(void **)&G.h_out, dec * CBUF * GROUP, true, "group h_out"}}};
}

bool group_alloc(Group &G, bool decode)
{
    return ok(hipStreamCreateWithFlags(&G.st, hipStreamNonBlocking), "group stream") && mem_alloc(group_mem(G, decode));
}

void group_free(Group &G)
{
    if (G.st) { (void)hipStreamSynchronize(G.st); (void)hipStreamDestroy(G.st); }
    mem_release(group_mem(G, false));
    G.st = nullptr;
}

// The double-buffered loop of both container directions over nb buffers: group g + 1 is submitted (its copies and kernels
// queued on its own stream) before group g is collected, so the device works while the host assembles.  submit(G) and
// collect(G) return false to stop; the two groups are released on every way out.
template <class Submit, class Collect> bool run_groups(size_t nb, bool decode, Submit submit, Collect collect)
{
    Group grp[2];
    auto start = [&](Group &G, size_t first) {
        G.first = first; G.nbuf = (int)std::min((size_t)GROUP, nb - first);
        return submit(G);
    };
    bool good = group_alloc(grp[0], decode) && group_alloc(grp[1], decode) && start(grp[0], 0);
    size_t next = GROUP;
    int cur = 0;
    while (good) {
        const bool more = next < nb;
        if (more) { good = start(grp[cur ^ 1], next); next += GROUP; }
        good = good && collect(grp[cur]);
        if (!more) break;
        cur ^= 1;
    }
    group_free(grp[0]); group_free(grp[1]);
    return good;
}

// the whole file, or nothing (pipes, FIFOs, directories: not seekable)
Bytes slurp(const char *path, unsigned long long *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) return nullptr;
    Bytes p;
    long sz = -1;
    if (fseek(f, 0, SEEK_END) == 0 && (sz = ftell(f)) >= 0 && fseek(f, 0, SEEK_SET) == 0) p = bytes_new((size_t)sz);
    if (p && fread(p.get(), 1, (size_t)sz, f) != (size_t)sz) p.reset();
    fclose(f);
    *len = p ? (unsigned long long)sz : 0;
    return p;
}

bool spill(const char *path, const unsigned char *data, size_t len)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool all = fwrite(data, 1, len, f) == len;
    fclose(f);
    return all;
}

} // namespace

extern "C" {

unsigned long long culzss_container_bound(unsigned long long len)
{
    const unsigned long long nb = (len + CBUF - 1) / CBUF;
    return 8 + 4 * nb + nb * (unsigned long long)CBUF;       // every buffer stored raw is the worst case
}

int culzss_container_compress(const unsigned char *in, unsigned long long len, unsigned char *out,
                              unsigned long long out_cap, unsigned long long *out_len)
{
    if (!in || !out || !out_len) return 0;
    if (len < (unsigned long long)CBUF) return 0;            // "too small to benefit from GPU" (main.c:228-232)
    const size_t nb = (size_t)((len + CBUF - 1) / CBUF);
    if (nb > 0x3FFFFFFFu || out_cap < culzss_container_bound(len)) return 0;
    const uint32_t nb32 = (uint32_t)nb, padding = (uint32_t)(nb * (size_t)CBUF - len);
    memcpy(out, &nb32, 4); memcpy(out + 4, &padding, 4);
    size_t wpos = 8 + 4 * nb, cum = 0;
    std::lock_guard<std::mutex> lk(g.mu);
    if (!init_locked()) return 0;
    const size_t stride = lzss_pack_stride(CBUF);
    auto submit = [&](Group &G) {
        for (int i = 0; i < G.nbuf; i++) {
            const size_t off = (G.first + i) * (size_t)CBUF;
            const size_t take = std::min((size_t)CBUF, (size_t)len - off);
            memcpy(G.h_in + (size_t)i * CBUF, in + off, take);
            if (take < (size_t)CBUF) memset(G.h_in + (size_t)i * CBUF + take, 0, CBUF - take);   // zero-filled tail
        }
        return ok(hipMemcpyAsync(G.d_in, G.h_in, (size_t)G.nbuf * CBUF, hipMemcpyHostToDevice, G.st), "H2D")
            && ok(lzss_encode(G.st, G.d_in, CBUF, G.nbuf, nullptr, G.d_packed, G.d_sizes, G.d_work), "encode")
            && ok(hipMemcpyAsync(G.h_sizes, G.d_sizes, sizeof(int) * G.nbuf, hipMemcpyDeviceToHost, G.st), "D2H sizes")
            && ok(hipMemcpyAsync(G.h_packed, G.d_packed, stride * G.nbuf, hipMemcpyDeviceToHost, G.st), "D2H packed");
    };
    auto collect = [&](Group &G) {
        if (!ok(hipStreamSynchronize(G.st), "sync")) return false;
        for (int i = 0; i < G.nbuf; i++) {
            int sz = G.h_sizes[i];
            if (sz >= CBUF) sz = 0;                                           // never packed to >= BUFSIZE: a payload of exactly
                                                                              // BUFSIZE bytes MEANS raw (deculzss.c:94-95)
            const size_t bytes = sz > 0 ? (size_t)sz : (size_t)CBUF;          // 0 => stored raw (culzss.c:241-242)
            if (wpos + bytes > out_cap || cum + bytes > 0xFFFFFFFFull) return false;              // u32 offsets: format limit
            memcpy(out + wpos, sz > 0 ? G.h_packed + (size_t)i * stride : G.h_in + (size_t)i * CBUF, bytes);
            wpos += bytes; cum += bytes;
            const uint32_t c32 = (uint32_t)cum;
            memcpy(out + 8 + 4 * (G.first + i), &c32, 4);
        }
        return true;
    };
    if (!run_groups(nb, false, submit, collect)) return 0;
    *out_len = wpos;
    return 1;
}

int culzss_container_decompress(const unsigned char *in, unsigned long long len, unsigned char *out,
                                unsigned long long out_cap, unsigned long long *out_len)
{
    if (!in || !out || !out_len || len < 8) return 0;
    uint32_t nb32, padding;
    memcpy(&nb32, in, 4); memcpy(&padding, in + 4, 4);
    const size_t nb = nb32;
    if (nb == 0 || len < 8 + 4 * nb || padding >= (uint32_t)CBUF) return 0;
    const unsigned long long total = (unsigned long long)nb * CBUF - padding;
    if (out_cap < total) return 0;
    std::lock_guard<std::mutex> lk(g.mu);
    if (!init_locked()) return 0;
    const size_t stride = lzss_pack_stride(CBUF);
    const size_t payload = 8 + 4 * nb;
    auto cumat = [&](size_t i) -> size_t { if (i == 0) return 0; uint32_t c; memcpy(&c, in + 8 + 4 * (i - 1), 4); return c; };
    auto submit = [&](Group &G) {
        for (int i = 0; i < G.nbuf; i++) {
            const size_t a = cumat(G.first + i), b = cumat(G.first + i + 1);
            const size_t sz = b - a;
            // (a packed chunk may be LONGER than the buffer: the reference's packer only gives up when the bytes flushed
            //  before the last group outgrow it, so up to BUFSIZE + 535 bytes reach the file -- include/culzss.h -- and
            //  its decoder takes everything that is not exactly BUFSIZE as packed, deculzss.c:92-98)
            if (b < a || sz > stride || payload + b > len) return false;
            const uint8_t *src = in + payload + a;
            if (sz != (size_t)CBUF) {                                          // packed: must hold its trailer, and the trailer
                constexpr size_t TR = 2 * (CBUF / GLC_LZSS_PACKET) + 6;        // must describe a 1 MiB buffer without padding
                int orig, pad;
                if (sz < TR || !parse_trailer(src, sz, &orig, &pad) || orig != CBUF || pad != 0) return false;
            }
            memcpy(G.h_packed + (size_t)i * stride, src, sz);
            G.h_sizes[i] = (sz == (size_t)CBUF) ? 0 : (int)sz;             // raw buffers: deculzss.c:94-95
        }
        G.h_sizes[GROUP] = 0;                                              // error word
        return ok(hipMemcpyAsync(G.d_packed, G.h_packed, stride * G.nbuf, hipMemcpyHostToDevice, G.st), "H2D")
            && ok(hipMemcpyAsync(G.d_sizes, G.h_sizes, sizeof(int) * (GROUP + 1), hipMemcpyHostToDevice, G.st), "H2D sizes")
            && ok(lzss_decode(G.st, G.d_packed, G.d_sizes, CBUF, G.nbuf, G.d_out, G.d_sizes + GROUP), "decode")
            && ok(hipMemcpyAsync(G.h_sizes + GROUP, G.d_sizes + GROUP, sizeof(int), hipMemcpyDeviceToHost, G.st), "D2H err")
            && ok(hipMemcpyAsync(G.h_out, G.d_out, (size_t)G.nbuf * CBUF, hipMemcpyDeviceToHost, G.st), "D2H");
    };
    auto collect = [&](Group &G) {
        if (!ok(hipStreamSynchronize(G.st), "sync") || G.h_sizes[GROUP]) return false;   // (a packet table that does not add up)
        for (int i = 0; i < G.nbuf; i++) {
            const size_t off = (G.first + i) * (size_t)CBUF;
            const size_t take = std::min((size_t)CBUF, (size_t)total - off);  // last buffer loses the padding (deculzss.c:156-159)
            memcpy(out + off, G.h_out + (size_t)i * CBUF, take);
        }
        return true;
    };
    if (!run_groups(nb, true, submit, collect)) return 0;
    *out_len = total;
    return 1;
}

/* ./main -i in -o out   (main.c:160-186, compress branch) */
int culzss_compress_file(const char *in_path, const char *out_path)
{
    unsigned long long len = 0, olen = 0;
    if (!in_path || !out_path) return 0;
    const Bytes in = slurp(in_path, &len);
    if (!in) return 0;
    const Bytes out = bytes_new((size_t)culzss_container_bound(len) + 16);
    return out && culzss_container_compress(in.get(), len, out.get(), culzss_container_bound(len), &olen) &&
           spill(out_path, out.get(), (size_t)olen);
}

/* ./main -d 1 -i in -o out   (main.c:207-222) */
int culzss_decompress_file(const char *in_path, const char *out_path)
{
    unsigned long long len = 0, olen = 0;
    if (!in_path || !out_path) return 0;
    const Bytes in = slurp(in_path, &len);
    if (!in || len < 8) return 0;
    uint32_t nb; memcpy(&nb, in.get(), 4);
    const unsigned long long cap = (unsigned long long)nb * CBUF;
    const Bytes out = bytes_new((size_t)cap);
    return out && culzss_container_decompress(in.get(), len, out.get(), cap, &olen) && spill(out_path, out.get(), (size_t)olen);
}

} // extern "C"
