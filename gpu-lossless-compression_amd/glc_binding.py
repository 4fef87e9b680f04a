"""ctypes binding of libglc_amd.so -- the host-side mirror, in Python, of what a
C caller of include/cudpp.h / include/culzss.h does.  Device memory comes from
torch (plumbing only): every call passes raw device pointers and sizes.

There is no CPU fallback: if the library is missing or a call fails, this
raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLC_LIB") or os.path.join(HERE, "libglc_amd.so")    # GLC_LIB: A/B builds of the same library

# enum values of include/cudpp.h (identical to the reference header)
CUDPP_SUCCESS = 0
CUDPP_ERROR_INVALID_HANDLE = 1
CUDPP_ERROR_ILLEGAL_CONFIGURATION = 2
CUDPP_ERROR_INVALID_PLAN = 3
CUDPP_ERROR_INSUFFICIENT_RESOURCES = 4
CUDPP_ERROR_UNKNOWN = 9999
CUDPP_UCHAR = 1
CUDPP_UINT = 5
CUDPP_ADD = 0
CUDPP_SCAN = 0
CUDPP_COMPRESS = 10
CUDPP_BWT = 12
CUDPP_MTF = 13
CUDPP_SA = 14
CHAIN_ALL_ROUNDS = 0x7FFFFFFF                           # glcPlanSetChains: a chain attempt in every doubling round
CUDPP_INVALID_HANDLE = 0xC0DABAD1
CUDPP_OPTION_FORWARD = 0x1
CUDPP_OPTION_BACKWARD = 0x2

HUFF_BLOCK = 4096
HUFF_MAX_WORDS = 1536
GLC_HD_MAX_LEN = 11

CUDPP_SYMBOLS = [
    "cudppCreate", "cudppDestroy", "cudppPlan", "cudppDestroyPlan", "cudppCompress",
    "cudppBurrowsWheelerTransform", "cudppMoveToFrontTransform", "cudppSuffixArray",
    "glcCompressBatch", "glcBwtBatch", "glcMtfBatch", "glcDecompressBatch", "glcPlanSetStream",
    "glcPlanSynchronize", "glcPlanEnableTiming", "glcPlanLastTiming", "glcPlanKernelProfile",
    "glcCompactStreams", "glcPlanSetPipelining", "glcPlanSetSorter", "glcPlanLastSortStats", "glcPlanLastSortStatsEx", "glcPlanLastSortRetries", "glcPlanLastSortResumed", "glcPlanLastSortPeriodic", "glcPlanSetChains", "glcPlanLastSortChains", "glcPlanLastSortSkipped", "glcPlanDebugSortFlags", "glcPlanDebugBucketFill", "glcHuffmanEncodeBatch", "glcExpandStreams", "glcPlanKernelProfileEx", "glcProbeStreamRead", "glcGenZipfPhilox", "glcGenFloatPhilox", "glcPlanKernelProfileLost",
    "glcCompressBatchCompact", "glcDecompressBatchCompact",
    "glcHuffmanDecodeBatch", "glcMtfInverseBatch", "glcPlanSetHuffDecoder",
    "glcDebugSetScratchFill", "glcDebugScratchFillStats",
]
CULZSS_SYMBOLS = [
    "compression_kernel_wrapper", "aftercompression_wrapper", "decompression_kernel_wrapper",
    "onestream_finish_GPU", "initGPUmem", "initCPUmem", "deleteGPUmem", "deleteCPUmem", "initGPU",
    "resetGPU", "streams_in_GPU", "deleteGPUStreams", "signalExitThreads", "deinitGPUmem",
    "dedeleteGPUmem", "deinitGPU", "culzss_compress", "culzss_decompress",
    "glcLzssEncodeDevice", "glcLzssDecodeDevice", "glcLzssLastKernelMs", "glcLzssPackStride",
    "glcLzssWorkBytes", "culzss_container_bound", "culzss_container_compress", "culzss_container_decompress",
    "culzss_compress_file", "culzss_decompress_file", "glcLzssEnableProfile", "glcLzssKernelProfile",
]
EXCHANGE_SYMBOLS = ["glcCommGetUniqueId", "glcCommInitRank", "glcCommAdopt", "glcCommDestroy", "glcCommInfo", "glcPackRecords",
                    "glcUnpackRecords", "glcGatherCounts", "glcGatherCountsBegin", "glcGatherCountsReady", "glcGatherCountsEnd",
                    "glcGatherStreams", "glcScatterStreams"]
HD_SYMBOLS = ["glcHdBuildTable", "glcHdEncodeHost", "glcHdWorkBytes", "glcHdDecodeDevice", "glcHdDecodeDeviceTable", "glcHdDecodeDeviceTableOnDevice", "glcHdEnableProfile",
              "glcHdKernelProfile", "glcHdEncodeBound", "glcHdEncodeWorkBytes", "glcHdHistogramDevice", "glcHdBuildTableDevice",
              "glcHdEncodeDevice", "glcHdSegmentsWorkBytes", "glcHdSegmentsTablesDevice", "glcHdSegmentsEncodeDevice",
              "glcHdSegmentsDecodeDevice"]


class CUDPPConfiguration(C.Structure):
    _fields_ = [("algorithm", C.c_int), ("op", C.c_int), ("datatype", C.c_int),
                ("options", C.c_uint), ("bucket_mapper", C.c_int)]


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libglc_amd.so is not built: run `python __graft_entry__.py` "
                           "(there is no CPU fallback)")
    # torch bundles its own libamdhip64.so.7 (ROCm 7.0) while the library links the
    # system one (ROCm 7.2) under the same soname: whichever is loaded first serves
    # both.  A process that uses torch for device memory must load torch's first,
    # or the two HIP runtimes disagree (hipGetDevice fails).  Pure C callers have
    # no torch and are unaffected.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    L.cudppCreate.argtypes = [C.POINTER(sz)]
    L.cudppDestroy.argtypes = [sz]
    L.cudppPlan.argtypes = [sz, C.POINTER(sz), CUDPPConfiguration, sz, sz, sz]
    L.cudppDestroyPlan.argtypes = [sz]
    L.cudppCompress.argtypes = [sz, vp, vp, vp, vp, vp, vp, vp, sz]
    L.cudppBurrowsWheelerTransform.argtypes = [sz, vp, vp, vp, sz]
    L.cudppMoveToFrontTransform.argtypes = [sz, vp, vp, sz]
    L.cudppSuffixArray.argtypes = [sz, vp, vp, sz]
    L.glcCompressBatch.argtypes = [sz, vp, vp, vp, vp, sz, vp, vp, sz, sz, sz]
    L.glcBwtBatch.argtypes = [sz, vp, vp, vp, sz, sz]
    L.glcMtfBatch.argtypes = [sz, vp, vp, sz, sz]
    L.glcDecompressBatch.argtypes = [sz, vp, vp, vp, sz, vp, sz, vp, sz, sz]
    L.glcCompressBatchCompact.argtypes = [sz, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, sz]
    L.glcDecompressBatchCompact.argtypes = [sz, vp, vp, vp, sz, vp, sz, vp, vp, sz, sz]
    L.glcPlanSetStream.argtypes = [sz, vp]
    L.glcPlanSynchronize.argtypes = [sz]
    L.glcPlanSetPipelining.argtypes = [sz, C.c_int]
    L.glcHuffmanEncodeBatch.argtypes = [sz, vp, vp, vp, sz, vp, vp, sz, sz, sz]
    L.glcHuffmanDecodeBatch.argtypes = [sz, vp, vp, sz, vp, sz, vp, sz, sz]
    L.glcMtfInverseBatch.argtypes = [sz, vp, vp, sz, sz]
    L.glcPlanSetHuffDecoder.argtypes = [sz, C.c_int]
    L.glcPlanSetSorter.argtypes = [sz, C.c_int]
    L.glcPlanLastSortStats.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanLastSortStatsEx.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanLastSortRetries.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanLastSortResumed.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanLastSortPeriodic.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanSetChains.argtypes = [sz, C.c_long, C.c_uint]
    L.glcPlanLastSortChains.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanLastSortSkipped.argtypes = [sz, C.POINTER(C.c_uint)]
    L.glcPlanDebugSortFlags.argtypes = [sz, C.POINTER(C.c_uint), C.POINTER(C.c_uint), sz]
    L.glcPlanDebugBucketFill.argtypes = [sz, sz, C.POINTER(C.c_uint)]
    L.glcPlanEnableTiming.argtypes = [sz, C.c_int]
    L.glcPlanLastTiming.argtypes = [sz, C.POINTER(C.c_float)]
    L.glcPlanKernelProfile.argtypes = [sz, C.POINTER(C.c_double)]
    L.glcPlanKernelProfileEx.argtypes = [sz, C.c_int, C.c_char_p, sz, C.POINTER(C.c_double)]
    L.glcPlanKernelProfileLost.argtypes = [sz, C.POINTER(C.c_ulonglong)]
    L.glcCompactStreams.argtypes = [sz, vp, sz, vp, sz, vp, vp]
    L.glcExpandStreams.argtypes = [sz, vp, vp, sz, vp, sz, vp]
    for name in CUDPP_SYMBOLS:
        getattr(L, name).restype = C.c_int
    L.glcDebugSetScratchFill.argtypes = [C.c_uint, C.c_uint]
    L.glcDebugSetScratchFill.restype = None
    L.glcDebugScratchFillStats.argtypes = [C.POINTER(C.c_ulonglong)]
    L.glcDebugScratchFillStats.restype = None
    L.glcProbeStreamRead.argtypes = [vp, sz, C.c_int, C.POINTER(C.c_float), vp]
    L.glcProbeStreamRead.restype = C.c_int
    L.glcGenZipfPhilox.argtypes = [vp, sz, C.c_ulonglong, C.c_uint, vp, vp]
    L.glcGenZipfPhilox.restype = C.c_int
    L.glcGenFloatPhilox.argtypes = [vp, sz, C.c_ulonglong, C.c_uint, vp]
    L.glcGenFloatPhilox.restype = C.c_int
    # CULZSS
    if hasattr(L, "compression_kernel_wrapper"):
        L.compression_kernel_wrapper.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, vp, vp]
        L.compression_kernel_wrapper.restype = C.c_int
        L.aftercompression_wrapper.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int)]
        L.aftercompression_wrapper.restype = C.c_int
        L.decompression_kernel_wrapper.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]
        L.decompression_kernel_wrapper.restype = C.c_int
        L.onestream_finish_GPU.argtypes = [C.c_int]
        L.onestream_finish_GPU.restype = C.c_int
        for nm in ("initGPUmem", "initCPUmem", "deinitGPUmem"):
            getattr(L, nm).argtypes = [C.c_int]
            getattr(L, nm).restype = vp
        for nm in ("deleteGPUmem", "deleteCPUmem", "dedeleteGPUmem"):
            getattr(L, nm).argtypes = [vp]
            getattr(L, nm).restype = None
        for nm in ("initGPU", "resetGPU", "deleteGPUStreams", "signalExitThreads", "deinitGPU"):
            getattr(L, nm).argtypes = []
            getattr(L, nm).restype = None
        L.streams_in_GPU.restype = C.c_int
        L.culzss_compress.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int)]
        L.culzss_compress.restype = C.c_int
        L.culzss_decompress.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int)]
        L.culzss_decompress.restype = C.c_int
        L.glcLzssEncodeDevice.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
        L.glcLzssEncodeDevice.restype = C.c_int
        L.glcLzssDecodeDevice.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
        L.glcLzssDecodeDevice.restype = C.c_int
        L.glcLzssPackStride.argtypes = [C.c_int]
        L.glcLzssPackStride.restype = C.c_ulonglong
        L.glcLzssWorkBytes.argtypes = [C.c_int, C.c_int]
        L.glcLzssWorkBytes.restype = C.c_ulonglong
        ull = C.c_ulonglong
        L.culzss_container_bound.argtypes = [ull]
        L.culzss_container_bound.restype = ull
        L.culzss_container_compress.argtypes = [vp, ull, vp, ull, C.POINTER(ull)]
        L.culzss_container_compress.restype = C.c_int
        L.culzss_container_decompress.argtypes = [vp, ull, vp, ull, C.POINTER(ull)]
        L.culzss_container_decompress.restype = C.c_int
        L.culzss_compress_file.argtypes = [C.c_char_p, C.c_char_p]
        L.culzss_compress_file.restype = C.c_int
        L.culzss_decompress_file.argtypes = [C.c_char_p, C.c_char_p]
        L.culzss_decompress_file.restype = C.c_int
        L.glcLzssEnableProfile.argtypes = [C.c_int]
        L.glcLzssEnableProfile.restype = C.c_int
        L.glcLzssKernelProfile.argtypes = [C.c_int, C.c_char_p, sz, C.POINTER(C.c_double)]
        L.glcLzssKernelProfile.restype = C.c_int
        L.glcLzssLastKernelMs.argtypes = []
        L.glcLzssLastKernelMs.restype = C.c_float
    if hasattr(L, "glcHdDecodeDevice"):
        L.glcHdBuildTable.argtypes = [vp, vp, vp]
        L.glcHdBuildTable.restype = C.c_int
        L.glcHdEncodeHost.argtypes = [vp, sz, vp, vp, vp, sz]
        L.glcHdEncodeHost.restype = sz
        L.glcHdWorkBytes.argtypes = [sz]
        L.glcHdWorkBytes.restype = sz
        L.glcHdDecodeDevice.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp]
        L.glcHdDecodeDevice.restype = C.c_int
        L.glcHdDecodeDeviceTable.argtypes = [vp, sz, vp, vp, sz, vp, vp]
        L.glcHdDecodeDeviceTable.restype = C.c_int
        L.glcHdDecodeDeviceTableOnDevice.argtypes = [vp, sz, vp, vp, sz, vp, vp]
        L.glcHdDecodeDeviceTableOnDevice.restype = C.c_int
        L.glcHdEnableProfile.argtypes = [C.c_int]
        L.glcHdEnableProfile.restype = C.c_int
        L.glcHdKernelProfile.argtypes = [C.c_int, C.c_char_p, sz, C.POINTER(C.c_double)]
        L.glcHdKernelProfile.restype = C.c_int
    if hasattr(L, "glcHdEncodeDevice"):
        L.glcHdEncodeBound.argtypes = [sz]
        L.glcHdEncodeBound.restype = sz
        L.glcHdEncodeWorkBytes.argtypes = [sz]
        L.glcHdEncodeWorkBytes.restype = sz
        L.glcHdHistogramDevice.argtypes = [vp, sz, vp, vp]
        L.glcHdHistogramDevice.restype = C.c_int
        L.glcHdBuildTableDevice.argtypes = [vp, vp, vp, vp, vp]
        L.glcHdBuildTableDevice.restype = C.c_int
        L.glcHdEncodeDevice.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp]
        L.glcHdEncodeDevice.restype = C.c_int
    if hasattr(L, "glcHdSegmentsEncodeDevice"):
        ull = C.c_ulonglong
        L.glcHdSegmentsWorkBytes.argtypes = [sz, sz]
        L.glcHdSegmentsWorkBytes.restype = sz
        L.glcHdSegmentsTablesDevice.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
        L.glcHdSegmentsTablesDevice.restype = C.c_int
        L.glcHdSegmentsEncodeDevice.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, ull, vp, vp, vp]
        L.glcHdSegmentsEncodeDevice.restype = C.c_int
        L.glcHdSegmentsDecodeDevice.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, vp]
        L.glcHdSegmentsDecodeDevice.restype = C.c_int
    if hasattr(L, "glcGatherStreams"):                             # include/glc_exchange.h
        ullp = C.POINTER(C.c_ulonglong)
        L.glcCommGetUniqueId.argtypes = [vp]
        L.glcCommInitRank.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int]
        L.glcCommAdopt.argtypes = [C.POINTER(vp), vp]
        L.glcCommDestroy.argtypes = [vp]
        L.glcCommInfo.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.glcPackRecords.argtypes = [vp, vp, vp, sz, vp, sz, sz, vp, vp]
        L.glcUnpackRecords.argtypes = [vp, sz, sz, vp, vp, vp, sz, vp, vp]
        L.glcGatherCounts.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, vp, ullp, vp]
        L.glcGatherCountsBegin.argtypes = [vp, C.c_ulonglong, C.c_ulonglong, vp, C.POINTER(C.c_int), vp]
        L.glcGatherCountsReady.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
        L.glcGatherCountsEnd.argtypes = [vp, C.c_int, ullp]
        L.glcGatherStreams.argtypes = [vp, C.c_int, vp, vp, sz, ullp, vp, vp, vp]
        L.glcScatterStreams.argtypes = [vp, C.c_int, vp, vp, sz, ullp, vp, vp, vp]
        for name in EXCHANGE_SYMBOLS:
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


class HdError(RuntimeError):
    pass


class CudppError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__("%s returned CUDPPResult %d" % (fn, code))
        self.code = code


def _chk(fn, code):
    if code != CUDPP_SUCCESS:
        raise CudppError(fn, code)


def debug_set_scratch_fill(word):
    """Process-wide test seam: while `word` is a 32-bit value, every block of device or pinned memory the library allocates
    for itself is filled with it before use; None switches the fill off again (the default).  Either way the counters of
    debug_scratch_fill_stats() start over."""
    if word is None:
        lib().glcDebugSetScratchFill(0, 0)
    else:
        if not 0 <= int(word) <= 0xFFFFFFFF:
            raise ValueError("the fill is a 32-bit word")
        lib().glcDebugSetScratchFill(1, int(word))


def debug_scratch_fill_stats():
    """(blocks, bytes) filled since the last debug_set_scratch_fill"""
    a = (C.c_ulonglong * 2)()
    lib().glcDebugScratchFillStats(a)
    return int(a[0]), int(a[1])


def config(algorithm, datatype=CUDPP_UCHAR, options=0, op=CUDPP_ADD):
    return CUDPPConfiguration(algorithm, op, datatype, options, 0)


class Cudpp:
    """cudppCreate/cudppDestroy pair."""

    def __init__(self):
        h = C.c_size_t(0)
        _chk("cudppCreate", lib().cudppCreate(C.byref(h)))
        self.handle = h.value

    def close(self):
        if self.handle:
            lib().cudppDestroy(self.handle)
            self.handle = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Plan:
    """cudppPlan/cudppDestroyPlan pair (rows = blocks per batched call)."""

    def __init__(self, cudpp, algorithm, n, rows=1, datatype=CUDPP_UCHAR, options=0):
        self.algorithm, self.n, self.rows = algorithm, n, rows
        h = C.c_size_t(0)
        rc = lib().cudppPlan(cudpp.handle, C.byref(h), config(algorithm, datatype, options), n, rows, 0)
        _chk("cudppPlan", rc)
        self.handle = h.value

    def close(self):
        if self.handle:
            lib().cudppDestroyPlan(self.handle)
            self.handle = 0

    def set_stream(self, stream_ptr):
        _chk("glcPlanSetStream", lib().glcPlanSetStream(self.handle, stream_ptr))

    def synchronize(self):
        _chk("glcPlanSynchronize", lib().glcPlanSynchronize(self.handle))

    def set_pipelining(self, on=True):
        """overlap the suffix sort of a batch with the MTF + Huffman stages of the previous one"""
        _chk("glcPlanSetPipelining", lib().glcPlanSetPipelining(self.handle, 1 if on else 0))

    def set_sorter(self, mode):
        """0 bucket sorter + general sorter for flagged blocks (default), 1 general only, 2 general, prefix doubling only"""
        _chk("glcPlanSetSorter", lib().glcPlanSetSorter(self.handle, int(mode)))

    def set_huff_decoder(self, mode):
        """the decoder's Huffman kernel: 0 by the call's size (default), 1 always k_dec_huff, 2 always k_dec_huff_lanes"""
        _chk("glcPlanSetHuffDecoder", lib().glcPlanSetHuffDecoder(self.handle, int(mode)))

    def last_flagged_blocks(self):
        a = C.c_uint(0)
        _chk("glcPlanLastSortStats", lib().glcPlanLastSortStats(self.handle, C.byref(a)))
        return a.value

    def last_sort_stats(self):
        """(blocks the bucket sorter gave up on, blocks the sample sorter gave up on too) of the last call"""
        a = (C.c_uint * 2)()
        _chk("glcPlanLastSortStatsEx", lib().glcPlanLastSortStatsEx(self.handle, a))
        return a[0], a[1]

    def last_sort_retries(self):
        """blocks of the last call the sample sorter finished in its second attempt (other samples)"""
        a = (C.c_uint * 1)()
        _chk("glcPlanLastSortRetries", lib().glcPlanLastSortRetries(self.handle, a))
        return a[0]

    def last_sort_resumed(self):
        """blocks of the last call whose prefix doubling resumed from the sample sorter's order (deep repeats inside them)"""
        a = (C.c_uint * 1)()
        _chk("glcPlanLastSortResumed", lib().glcPlanLastSortResumed(self.handle, a))
        return a[0]

    def last_sort_periodic(self):
        """blocks of the last call finished by the periodic tier (one periodic stretch: closed form over the sorted rotations)"""
        a = (C.c_uint * 1)()
        _chk("glcPlanLastSortPeriodic", lib().glcPlanLastSortPeriodic(self.handle, a))
        return a[0]

    def set_chains(self, min_live=None, round_mask=None):
        """chain groups of the doubling rounds: attempted in doubling round r where bit r of round_mask is set and at least
        min_live suffixes of the call are live (0: never); None restores the default (GLC_CHAIN_MIN / GLC_CHAIN_ROUNDS, else
        16384 / 0x15).  round_mask=CHAIN_ALL_ROUNDS: every round"""
        m = -1 if min_live is None else int(min_live)
        r = 0xFFFFFFFF if round_mask is None else int(round_mask)
        if not 0 <= r <= 0xFFFFFFFF:
            raise ValueError("round_mask is a 32-bit mask")
        _chk("glcPlanSetChains", lib().glcPlanSetChains(self.handle, m, r))

    def last_sort_chains(self):
        """(chain groups ordered by the rule, candidates refused) of the last call, summed over rounds and blocks"""
        a = (C.c_uint * 2)()
        _chk("glcPlanLastSortChains", lib().glcPlanLastSortChains(self.handle, a))
        return int(a[0]), int(a[1])

    def last_sort_skipped(self):
        """(skipped, streak): did the plan's last call go straight to the sample sorter, and the streak of all-text-like calls"""
        a = (C.c_uint * 2)()
        _chk("glcPlanLastSortSkipped", lib().glcPlanLastSortSkipped(self.handle, a))
        return bool(a[0]), int(a[1])

    def enable_timing(self, mode=1):
        """0 off, 1 stage events, 3 stage events + dominant-kernel events"""
        _chk("glcPlanEnableTiming", lib().glcPlanEnableTiming(self.handle, int(mode)))

    def kernel_profile(self):
        """dominant kernel {ms, launches, units}; resets the accumulators"""
        a = (C.c_double * 3)()
        _chk("glcPlanKernelProfile", lib().glcPlanKernelProfile(self.handle, a))
        return dict(ms=a[0], launches=int(a[1]), units=a[2])

    def kernel_profiles(self):
        """{kernel name: dict(ms, launches, units)} of every profiled kernel (call after synchronize())"""
        out, i = {}, 0
        name = C.create_string_buffer(96)
        a = (C.c_double * 3)()
        while lib().glcPlanKernelProfileEx(self.handle, i, name, 96, a) == CUDPP_SUCCESS:
            if a[1] > 0:
                out[name.value.decode()] = dict(ms=a[0], launches=int(a[1]), units=a[2])
            i += 1
        return out

    def last_timing(self):
        a = (C.c_float * 4)()
        _chk("glcPlanLastTiming", lib().glcPlanLastTiming(self.handle, a))
        return list(a)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def compressed_stride_words(n):
    return (HUFF_MAX_WORDS + 1) * ((n + HUFF_BLOCK - 1) // HUFF_BLOCK)


# ---------------------------------------------------------------------------
# torch-tensor conveniences (device pointers in, device tensors out)
# ---------------------------------------------------------------------------
def compress_batch(plan, d_in, n, nblk):
    """d_in: uint8 cuda tensor of nblk*n bytes.  Returns dict of cuda tensors."""
    import torch
    dev = d_in.device
    nsub = (n + HUFF_BLOCK - 1) // HUFF_BLOCK
    stride = compressed_stride_words(n)
    out = dict(
        bwt_index=torch.empty(nblk, dtype=torch.int32, device=dev),
        hist=torch.empty(nblk * 256, dtype=torch.int32, device=dev),
        offsets=torch.empty(nblk * nsub, dtype=torch.int32, device=dev),
        size=torch.empty(nblk, dtype=torch.int32, device=dev),
        words=torch.empty(nblk * stride, dtype=torch.int32, device=dev),
        stride=stride, nsub=nsub,
    )
    rc = lib().glcCompressBatch(plan.handle, d_in.data_ptr(), out["bwt_index"].data_ptr(),
                                out["hist"].data_ptr(), out["offsets"].data_ptr(), nsub,
                                out["size"].data_ptr(), out["words"].data_ptr(), stride, n, nblk)
    _chk("glcCompressBatch", rc)
    return out


def huffman_encode_batch(plan, d_sym, n, nblk):
    """stand-alone Huffman stage on symbols (uint8 cuda tensor of nblk*n bytes); same outputs as compress_batch"""
    import torch
    dev = d_sym.device
    nsub = (n + HUFF_BLOCK - 1) // HUFF_BLOCK
    stride = compressed_stride_words(n)
    out = dict(hist=torch.empty(nblk * 256, dtype=torch.int32, device=dev),
               offsets=torch.empty(nblk * nsub, dtype=torch.int32, device=dev),
               size=torch.empty(nblk, dtype=torch.int32, device=dev),
               words=torch.empty(nblk * stride, dtype=torch.int32, device=dev), stride=stride, nsub=nsub)
    rc = lib().glcHuffmanEncodeBatch(plan.handle, d_sym.data_ptr(), out["hist"].data_ptr(), out["offsets"].data_ptr(),
                                     nsub, out["size"].data_ptr(), out["words"].data_ptr(), stride, n, nblk)
    _chk("glcHuffmanEncodeBatch", rc)
    return out


def huffman_decode_batch(plan, comp, n, nblk, d_sym=None):
    """glcHuffmanDecodeBatch on a dict of hist / offsets / words (+ nsub, stride) as huffman_encode_batch returns it: the
    symbols, nblk rows of n bytes"""
    import torch
    if d_sym is None:
        d_sym = torch.empty(nblk * n, dtype=torch.uint8, device=comp["words"].device)
    rc = lib().glcHuffmanDecodeBatch(plan.handle, comp["hist"].data_ptr(), comp["offsets"].data_ptr(), comp["nsub"],
                                     comp["words"].data_ptr(), comp["stride"], d_sym.data_ptr(), n, nblk)
    _chk("glcHuffmanDecodeBatch", rc)
    return d_sym


def mtf_inverse_batch(plan, d_mtf, n, nblk, d_out=None):
    """glcMtfInverseBatch (a COMPRESS plan): nblk rows of n MTF bytes -> the bytes they stand for"""
    import torch
    if d_out is None:
        d_out = torch.empty(nblk * n, dtype=torch.uint8, device=d_mtf.device)
    _chk("glcMtfInverseBatch", lib().glcMtfInverseBatch(plan.handle, d_mtf.data_ptr(), d_out.data_ptr(), n, nblk))
    return d_out


def compress_batch_into(plan, d_in, n, nblk, out):
    rc = lib().glcCompressBatch(plan.handle, d_in.data_ptr(), out["bwt_index"].data_ptr(),
                                out["hist"].data_ptr(), out["offsets"].data_ptr(), out["nsub"],
                                out["size"].data_ptr(), out["words"].data_ptr(), out["stride"], n, nblk)
    _chk("glcCompressBatch", rc)


def compress_batch_compact(plan, d_in, n, nblk, words=None, block_off=None, start=None, meta=None, first=0):
    """glcCompressBatchCompact.  words: int32 cuda tensor that receives the streams back to back (default: room for the
    worst case); block_off: int64 tensor of >= first + nblk + 1 entries; start: data_ptr of a device u64 the first block
    begins at (None = 0); meta: dict with bwt_index / hist / offsets / size tensors for >= first + nblk blocks (default:
    new ones); first: index of this batch's first block in those arrays.  Returns the dict (+ words, block_off)."""
    import torch
    dev = d_in.device
    nsub = (n + HUFF_BLOCK - 1) // HUFF_BLOCK
    if meta is None:
        meta = dict(bwt_index=torch.empty(first + nblk, dtype=torch.int32, device=dev),
                    hist=torch.empty((first + nblk) * 256, dtype=torch.int32, device=dev),
                    offsets=torch.empty((first + nblk) * nsub, dtype=torch.int32, device=dev),
                    size=torch.empty(first + nblk, dtype=torch.int32, device=dev), nsub=nsub)
    if words is None:
        words = torch.empty(nblk * compressed_stride_words(n), dtype=torch.int32, device=dev)
    if block_off is None:
        block_off = torch.empty(first + nblk + 1, dtype=torch.int64, device=dev)
    rc = lib().glcCompressBatchCompact(plan.handle, d_in.data_ptr(), meta["bwt_index"].data_ptr() + 4 * first,
                                       meta["hist"].data_ptr() + 1024 * first, meta["offsets"].data_ptr() + 4 * nsub * first, nsub,
                                       meta["size"].data_ptr() + 4 * first, words.data_ptr(), words.numel(),
                                       block_off.data_ptr() + 8 * first, start, n, nblk)
    _chk("glcCompressBatchCompact", rc)
    out = dict(meta)
    out.update(words=words, block_off=block_off, nsub=nsub)
    return out


def decompress_batch_compact(plan, comp, n, nblk, first=0, d_out=None):
    """glcDecompressBatchCompact on the dict compress_batch_compact returns (blocks first .. first + nblk)"""
    import torch
    nsub = comp["nsub"]
    if d_out is None:
        d_out = torch.empty(nblk * n, dtype=torch.uint8, device=comp["words"].device)
    rc = lib().glcDecompressBatchCompact(plan.handle, comp["bwt_index"].data_ptr() + 4 * first, comp["hist"].data_ptr() + 1024 * first,
                                         comp["offsets"].data_ptr() + 4 * nsub * first, nsub, comp["words"].data_ptr(),
                                         comp["words"].numel(), comp["block_off"].data_ptr() + 8 * first, d_out.data_ptr(), n, nblk)
    _chk("glcDecompressBatchCompact", rc)
    return d_out


def decompress_batch(plan, comp, n, nblk, d_out=None):
    import torch
    if d_out is None:
        d_out = torch.empty(nblk * n, dtype=torch.uint8, device=comp["words"].device)
    rc = lib().glcDecompressBatch(plan.handle, comp["bwt_index"].data_ptr(), comp["hist"].data_ptr(),
                                  comp["offsets"].data_ptr(), comp["nsub"], comp["words"].data_ptr(),
                                  comp["stride"], d_out.data_ptr(), n, nblk)
    _chk("glcDecompressBatch", rc)
    return d_out


# ---------------------------------------------------------------------------
# CUHD-shaped stream (include/glc_hd.h)
# ---------------------------------------------------------------------------
def hd_build_table(hist256):
    """hist256: 256 counts.  Returns (lens u8[256], codes u16[256])."""
    import numpy as np
    h = np.ascontiguousarray(hist256, dtype=np.uint64)
    lens = np.zeros(256, dtype=np.uint8)
    codes = np.zeros(256, dtype=np.uint16)
    if lib().glcHdBuildTable(h.ctypes.data, lens.ctypes.data, codes.ctypes.data) == 0:
        raise HdError("glcHdBuildTable failed (empty histogram?)")
    return lens, codes


def hd_encode_host(data_u8, lens, codes):
    """Host encoder: returns the stream as uint32 units (incl. the zero pad unit)."""
    import numpy as np
    a = np.ascontiguousarray(data_u8, dtype=np.uint8)
    cap = (a.size * GLC_HD_MAX_LEN + 31) // 32 + 2
    out = np.zeros(cap, dtype=np.uint32)
    n = lib().glcHdEncodeHost(a.ctypes.data, a.size, lens.ctypes.data, codes.ctypes.data, out.ctypes.data, cap)
    if n == 0:
        raise HdError("glcHdEncodeHost failed (symbol without a code?)")
    return out[:n].copy()


def hd_decode_device(d_units, lens, codes, nsym, stream=None):
    """d_units: int32/uint32 cuda tensor.  Returns a uint8 cuda tensor of nsym bytes."""
    import torch
    nunits = d_units.numel()
    work = torch.empty(lib().glcHdWorkBytes(nunits), dtype=torch.uint8, device=d_units.device)
    out = torch.empty(max(1, nsym), dtype=torch.uint8, device=d_units.device)
    ok = lib().glcHdDecodeDevice(d_units.data_ptr(), nunits, lens.ctypes.data, codes.ctypes.data,
                                 out.data_ptr(), nsym, work.data_ptr(), _stream_ptr(stream))
    if not ok:
        raise HdError("glcHdDecodeDevice failed")
    return out[:nsym]


def _stream_ptr(stream):
    """None (the null stream), a raw hipStream_t value, or a torch.cuda.Stream"""
    return getattr(stream, "cuda_stream", stream)


def hd_histogram_device(d_in, stream=None, d_hist=None):
    """d_in: uint8 cuda tensor (any offset).  Returns an int64 cuda tensor of 256 byte counts; enqueued only."""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if d_hist is None:
        d_hist = torch.empty(256, dtype=torch.int64, device=x.device)
    if not lib().glcHdHistogramDevice(x.data_ptr() if x.numel() else None, x.numel(), d_hist.data_ptr(), _stream_ptr(stream)):
        raise HdError("glcHdHistogramDevice failed")
    return d_hist


def hd_build_table_device(d_hist, table=True, stream=None):
    """d_hist: 256 u64 counts in an int64 cuda tensor.  Returns (d_lens uint8[256], d_codes int16[256] holding the u16 codes,
    d_table uint8[4096] -- the reference's {num_bits, symbol}[2048] decoder table -- or None); enqueued only."""
    import torch
    dev = d_hist.device
    lens = torch.empty(256, dtype=torch.uint8, device=dev)
    codes = torch.empty(256, dtype=torch.int16, device=dev)
    tab = torch.empty(4096, dtype=torch.uint8, device=dev) if table else None
    if not lib().glcHdBuildTableDevice(d_hist.data_ptr(), lens.data_ptr(), codes.data_ptr(), tab.data_ptr() if table else None,
                                       _stream_ptr(stream)):
        raise HdError("glcHdBuildTableDevice failed")
    return lens, codes, tab


def hd_encode_device(d_in, d_lens, d_codes, cap_units=None, stream=None, work=None, d_units=None):
    """Device encode of the uint8 cuda tensor d_in with a device table.  Returns (d_units int32[cap_units], d_nunits int64[1]):
    the stream is d_units[:d_nunits] (0 units: a symbol without a usable code, or cap_units too small).  Enqueued only."""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    dev = x.device
    n = x.numel()
    if cap_units is None:
        cap_units = d_units.numel() if d_units is not None else int(lib().glcHdEncodeBound(n))
    if d_units is None:
        d_units = torch.empty(max(1, cap_units), dtype=torch.int32, device=dev)
    if work is None:
        work = torch.empty(int(lib().glcHdEncodeWorkBytes(n)), dtype=torch.uint8, device=dev)
    nunits = torch.empty(1, dtype=torch.int64, device=dev)
    if not lib().glcHdEncodeDevice(x.data_ptr() if n else None, n, d_lens.data_ptr(), d_codes.data_ptr(), d_units.data_ptr(),
                                   cap_units, nunits.data_ptr(), work.data_ptr(), _stream_ptr(stream)):
        raise HdError("glcHdEncodeDevice failed")
    if isinstance(stream, torch.cuda.Stream):                  # allocated on the current stream, used on `stream`
        for t in (work, d_units, nunits):
            t.record_stream(stream)
    return d_units, nunits


HD_SEGMENT_MAX = 1 << 20


def _i64(dev, values):
    import torch
    return torch.as_tensor(values, dtype=torch.int64).reshape(-1).to(dev)


def hd_segments_tables(d_base, d_offsets, d_lengths, max_len, stream=None):
    """The batched histogram + table builder: segments [d_offsets[i], + d_lengths[i]) of the uint8 cuda tensor d_base (offsets and
    lengths: int64 cuda tensors).  Returns (d_hist int32[count, 256], d_lens uint8[count, 256], d_codes int16[count, 256] holding the
    u16 codes, d_nunits int64[count]); enqueued only."""
    import torch
    dev, count = d_base.device, d_offsets.numel()
    hist = torch.empty((max(count, 1), 256), dtype=torch.int32, device=dev)
    lens = torch.empty((max(count, 1), 256), dtype=torch.uint8, device=dev)
    codes = torch.empty((max(count, 1), 256), dtype=torch.int16, device=dev)
    nunits = torch.empty(max(count, 1), dtype=torch.int64, device=dev)
    if not lib().glcHdSegmentsTablesDevice(d_base.data_ptr(), d_offsets.data_ptr(), d_lengths.data_ptr(), count, int(max_len),
                                           hist.data_ptr(), lens.data_ptr(), codes.data_ptr(), nunits.data_ptr(), _stream_ptr(stream)):
        raise HdError("glcHdSegmentsTablesDevice failed")
    if isinstance(stream, torch.cuda.Stream):
        for t in (hist, lens, codes, nunits):
            t.record_stream(stream)
    return hist[:count], lens[:count], codes[:count], nunits[:count]


def hd_segments_work(count, max_len, device):
    import torch
    return torch.empty(max(1, int(lib().glcHdSegmentsWorkBytes(int(count), int(max_len)))), dtype=torch.uint8, device=device)


def hd_segments_encode(d_base, d_offsets, d_lengths, max_len, d_lens, d_codes, d_nunits, d_units, d_unit_offsets, cap_units=None,
                       d_skip=None, work=None, stream=None):
    """Every segment's stream into the int32 cuda tensor d_units at d_unit_offsets[i] (int64, in units); enqueued only."""
    count = d_offsets.numel()
    if work is None:
        work = hd_segments_work(count, max_len, d_base.device)
    cap = d_units.numel() if cap_units is None else int(cap_units)
    if not lib().glcHdSegmentsEncodeDevice(d_base.data_ptr(), d_offsets.data_ptr(), d_lengths.data_ptr(), count, int(max_len),
                                           d_lens.data_ptr(), d_codes.data_ptr(), d_nunits.data_ptr(), d_units.data_ptr(),
                                           d_unit_offsets.data_ptr(), cap, d_skip.data_ptr() if d_skip is not None else None,
                                           work.data_ptr(), _stream_ptr(stream)):
        raise HdError("glcHdSegmentsEncodeDevice failed")
    return work


def hd_segments_decode(d_units, d_unit_offsets, d_nunits, d_hist, d_out, d_out_offsets, d_lengths, max_len, d_skip=None, work=None,
                       stream=None):
    """The inverse: d_lengths[i] symbols of every stream into the uint8 cuda tensor d_out at d_out_offsets[i]; enqueued only."""
    count = d_out_offsets.numel()
    if work is None:
        work = hd_segments_work(count, max_len, d_out.device)
    if not lib().glcHdSegmentsDecodeDevice(d_units.data_ptr(), d_unit_offsets.data_ptr(), d_nunits.data_ptr(), d_hist.data_ptr(),
                                           d_out.data_ptr(), d_out_offsets.data_ptr(), d_lengths.data_ptr(), count, int(max_len),
                                           d_skip.data_ptr() if d_skip is not None else None, work.data_ptr(), _stream_ptr(stream)):
        raise HdError("glcHdSegmentsDecodeDevice failed")
    return work


# --------------------------------------------------------------------------------------------------------------------------
# include/glc_container.h: the CRC-checked container of the BWT codec
# --------------------------------------------------------------------------------------------------------------------------
CONTAINER_SYMBOLS = ["glcContainerBound", "glcContainerCompressDevice", "glcContainerDecompressDevice", "glcContainerCompress",
                     "glcContainerDecompress", "glcContainerCompressFile", "glcContainerDecompressFile", "glcCrc32Segments",
                     "glcContainerLastError", "glcShuffleSegments", "glcUnshuffleSegments", "glcShuffleDevice", "glcUnshuffleDevice",
                     "glcPlanSetContainerShuffle", "glcPlanGetContainerShuffle", "glcPlanSetContainerCodec", "glcPlanGetContainerCodec",
                     "glcDeltaShuffleDevice", "glcUndeltaUnshuffleDevice", "glcPlanSetContainerDelta", "glcPlanGetContainerDelta",
                     "glcSparseSplitSegments", "glcSparseJoinSegments", "glcPlanSetContainerSparse", "glcPlanGetContainerSparse",
                     "glcZeroRunSplitSegments", "glcZeroRunJoinSegments", "glcPlanSetContainerRuns", "glcPlanGetContainerRuns",
                     "glcAnsEncodeSegments", "glcAnsDecodeSegments", "glcAnsSegmentsWorkBytes", "glcAnsBoundWords",
                     "glcPlanSetContainerAns", "glcPlanGetContainerAns",
                     "glcProbeSegments", "glcPlanSetContainerAuto", "glcPlanGetContainerAuto",
                     "glcBigramProbeSegments", "glcContainerLastChoice", "glcFilterProbeSegments",
                     "glcPlanSetContainerFilterAuto", "glcPlanGetContainerFilterAuto", "glcContainerLastFilters",
                     "glcDedupWorkBytes", "glcDedupMapSegments", "glcDedupFillSegments", "glcPlanSetContainerDedup", "glcPlanGetContainerDedup",
                     "glcLagDeltaShuffleDevice", "glcUnlagDeltaUnshuffleDevice", "glcUnlagDeltaUnshuffleRangeDevice",
                     "glcPlanSetContainerDeltaLag", "glcPlanGetContainerDeltaLag",
                     "glcGridDeltaShuffleDevice", "glcUngridDeltaUnshuffleDevice", "glcUngridDeltaUnshuffleRangeDevice",
                     "glcPlanSetContainerDeltaGrid", "glcPlanGetContainerDeltaGrid",
                     "glcLagProbeSegments", "glcLagPlanesSegments",
                     "glcPlanSetContainerFilterLag", "glcPlanGetContainerFilterLag", "glcContainerLastLagFilters",
                     "glcGridProbeSegments", "glcGridPlanesSegments",
                     "glcPlanSetContainerFilterGrid", "glcPlanGetContainerFilterGrid", "glcContainerLastGridFilters",
                     "glcByteDeltaDevice", "glcUnbyteDeltaDevice", "glcUnbyteDeltaRangeDevice",
                     "glcPlanSetContainerByteDelta", "glcPlanGetContainerByteDelta",
                     "glcByteProbeSegments", "glcBytePlanesSegments",
                     "glcPlanSetContainerFilterByte", "glcPlanGetContainerFilterByte", "glcContainerLastByteFilters",
                     "glcPlanSetContainerChooseFilters", "glcPlanGetContainerChooseFilters",
                     "glcVolDeltaShuffleDevice", "glcUnvolDeltaUnshuffleDevice", "glcUnvolDeltaUnshuffleRangeDevice",
                     "glcPlanSetContainerDeltaVolume", "glcPlanGetContainerDeltaVolume", "glcContainerIndexPlane",
                     "glcContainerIndexDevice", "glcContainerIndex", "glcContainerIndexFile", "glcContainerIndexInfo",
                     "glcContainerReadRangeDevice", "glcContainerReadRange", "glcContainerReadRangeFile", "glcContainerLastRangeStats",
                     "glcUnshuffleRangeDevice", "glcUndeltaUnshuffleRangeDevice", "glcContainerIndexFree"]
RANGE_SYMBOLS = CONTAINER_SYMBOLS[-11:]                         # the frame index and the range reads
CONTAINER_CODEC_BWT, CONTAINER_CODEC_HUFF0, CONTAINER_CODEC_CHOOSE = 0, 1, 4
CONTAINER_WHAT = {0: "ok", 1: "stream header", 2: "frame table", 3: "record crc", 4: "decoded crc", 5: "truncated", 6: "capacity"}
CONTAINER_HEADER_BYTES = 32


def _ct():
    L = lib()
    if not getattr(L, "_ct_ready", False):
        vp, sz, ull = C.c_void_p, C.c_size_t, C.c_ulonglong
        ullp = C.POINTER(ull)
        L.glcContainerBound.argtypes = [ull, sz]
        L.glcContainerBound.restype = ull
        for nm in ("glcContainerCompressDevice", "glcContainerDecompressDevice"):
            getattr(L, nm).argtypes = [sz, vp, ull, vp, ull, vp]
        for nm in ("glcContainerCompress", "glcContainerDecompress"):
            getattr(L, nm).argtypes = [sz, vp, ull, vp, ull, ullp]
        for nm in ("glcContainerCompressFile", "glcContainerDecompressFile"):
            getattr(L, nm).argtypes = [sz, C.c_char_p, C.c_char_p]
        L.glcCrc32Segments.argtypes = [vp, vp, vp, sz, vp, vp]
        L.glcContainerLastError.argtypes = [sz, ullp]
        for nm in ("glcShuffleSegments", "glcUnshuffleSegments"):
            getattr(L, nm).argtypes = [vp, vp, vp, vp, sz, C.c_uint, vp]
        for nm in ("glcShuffleDevice", "glcUnshuffleDevice", "glcDeltaShuffleDevice", "glcUndeltaUnshuffleDevice"):
            getattr(L, nm).argtypes = [vp, vp, ull, C.c_uint, vp]
        L.glcSparseSplitSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
        L.glcSparseJoinSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.glcZeroRunSplitSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp]
        L.glcZeroRunJoinSegments.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp]
        for nm in ("glcContainerIndexDevice", "glcContainerIndex"):
            getattr(L, nm).argtypes = [sz, vp, ull, C.POINTER(vp)]
        L.glcContainerIndexFile.argtypes = [sz, C.c_char_p, C.POINTER(vp)]
        L.glcContainerIndexFree.argtypes = [vp]
        L.glcContainerIndexInfo.argtypes = [vp, ullp]
        for nm in ("glcContainerReadRangeDevice", "glcContainerReadRange"):
            getattr(L, nm).argtypes = [sz, vp, vp, ull, ull, ull, vp]
        L.glcContainerReadRangeFile.argtypes = [sz, vp, C.c_char_p, ull, ull, vp]
        L.glcContainerLastRangeStats.argtypes = [sz, ullp]
        for nm in ("glcUnshuffleRangeDevice", "glcUndeltaUnshuffleRangeDevice"):
            getattr(L, nm).argtypes = [vp, vp, ull, C.c_uint, ull, ull, vp]
        for nm in CONTAINER_SYMBOLS:                              # the plan's settings: Set takes the value, Get a pointer to it
            if nm.startswith("glcPlanSetContainer"):
                getattr(L, nm).argtypes = [sz, C.c_uint]
            elif nm.startswith("glcPlanGetContainer"):
                getattr(L, nm).argtypes = [sz, C.POINTER(C.c_uint)]
        L.glcPlanSetContainerDeltaLag.argtypes = [sz, C.c_uint, C.c_uint]
        L.glcPlanGetContainerDeltaLag.argtypes = [sz, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        for nm in ("glcLagDeltaShuffleDevice", "glcUnlagDeltaUnshuffleDevice"):
            getattr(L, nm).argtypes = [vp, vp, ull, C.c_uint, C.c_uint, C.c_uint, vp]
        L.glcUnlagDeltaUnshuffleRangeDevice.argtypes = [vp, vp, ull, C.c_uint, C.c_uint, C.c_uint, ull, ull, vp]
        L.glcPlanSetContainerDeltaGrid.argtypes = [sz, C.c_uint, C.c_uint]
        L.glcPlanGetContainerDeltaGrid.argtypes = [sz, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        for nm in ("glcGridDeltaShuffleDevice", "glcUngridDeltaUnshuffleDevice"):
            getattr(L, nm).argtypes = [vp, vp, ull, C.c_uint, C.c_uint, C.c_uint, vp]
        L.glcUngridDeltaUnshuffleRangeDevice.argtypes = [vp, vp, ull, C.c_uint, C.c_uint, C.c_uint, ull, ull, vp]
        L.glcPlanSetContainerDeltaVolume.argtypes = [sz, C.c_uint]
        L.glcPlanGetContainerDeltaVolume.argtypes = [sz, C.POINTER(C.c_uint)]
        for nm in ("glcVolDeltaShuffleDevice", "glcUnvolDeltaUnshuffleDevice"):
            getattr(L, nm).argtypes = [vp, vp, ull, C.c_uint, C.c_uint, C.c_uint, C.c_uint, vp]
        L.glcUnvolDeltaUnshuffleRangeDevice.argtypes = [vp, vp, ull, C.c_uint, C.c_uint, C.c_uint, C.c_uint, ull, ull, vp]
        L.glcContainerIndexPlane.argtypes = [vp, C.POINTER(C.c_uint)]
        L.glcPlanSetContainerByteDelta.argtypes = [sz, C.c_uint, C.c_uint]
        L.glcPlanGetContainerByteDelta.argtypes = [sz, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        for nm in ("glcByteDeltaDevice", "glcUnbyteDeltaDevice"):
            getattr(L, nm).argtypes = [vp, vp, ull, C.c_uint, C.c_uint, vp]
        L.glcUnbyteDeltaRangeDevice.argtypes = [vp, vp, ull, C.c_uint, C.c_uint, ull, ull, vp]
        for nm in CONTAINER_SYMBOLS[1:-1]:
            getattr(L, nm).restype = C.c_int
        L.glcContainerIndexFree.restype = None
        L.glcAnsEncodeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]
        L.glcAnsDecodeSegments.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, vp, vp, sz, vp]
        L.glcAnsSegmentsWorkBytes.argtypes = [sz, sz]
        L.glcAnsSegmentsWorkBytes.restype = sz
        L.glcAnsBoundWords.argtypes = [sz]
        L.glcAnsBoundWords.restype = sz
        L.glcProbeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.glcBigramProbeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp]
        L.glcContainerLastChoice.argtypes = [sz, ullp]
        L.glcFilterProbeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.glcContainerLastFilters.argtypes = [sz, ullp]
        L.glcContainerLastLagFilters.argtypes = [sz, ullp]
        L.glcLagProbeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.glcLagPlanesSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.glcContainerLastGridFilters.argtypes = [sz, ullp]
        L.glcGridProbeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.glcGridPlanesSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.glcContainerLastByteFilters.argtypes = [sz, ullp]
        L.glcByteProbeSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.glcBytePlanesSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.glcDedupWorkBytes.argtypes = [sz, sz]
        L.glcDedupWorkBytes.restype = sz
        L.glcDedupMapSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp, sz, vp]
        L.glcDedupFillSegments.argtypes = [vp, vp, vp, sz, sz, vp, vp]
        L._ct_ready = True
    return L


def container_bound(length, block_len):
    """worst-case container bytes for `length` input bytes in blocks of `block_len`"""
    return int(_ct().glcContainerBound(int(length), int(block_len)))


def container_compress(plan, d_in, cap=None):
    """device uint8 tensor -> device uint8 tensor holding the container (a view of a buffer of `cap` bytes, default the bound)"""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    cap = container_bound(x.numel(), plan.n) if cap is None else int(cap)
    out = torch.empty(max(cap, 8), dtype=torch.uint8, device=x.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=x.device)
    _chk("glcContainerCompressDevice", _ct().glcContainerCompressDevice(plan.handle, x.data_ptr() if x.numel() else None,
                                                                         x.numel(), out.data_ptr(), cap, d_len.data_ptr()))
    return out[:int(d_len.item())]


def container_total_len(header):
    """the input length a container's stream header records (bytes 16..23)"""
    import numpy as np
    h = np.frombuffer(bytes(header[:CONTAINER_HEADER_BYTES]), dtype=np.uint8)
    return int(h[16:24].view(np.uint64)[0])


def container_decompress(plan, d_cont, cap=None):
    """device container (uint8 tensor, 8-byte aligned) -> device uint8 tensor of the decoded bytes"""
    import torch
    c = d_cont.reshape(-1)
    if cap is None:
        cap = container_total_len(c[:CONTAINER_HEADER_BYTES].cpu().numpy().tobytes()) if c.numel() >= CONTAINER_HEADER_BYTES else 0
    out = torch.empty(int(cap), dtype=torch.uint8, device=c.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=c.device)
    _chk("glcContainerDecompressDevice", _ct().glcContainerDecompressDevice(
        plan.handle, c.data_ptr(), c.numel(), out.data_ptr() if out.numel() else None, int(cap), d_len.data_ptr()))
    return out[:int(d_len.item())]


def container_compress_host(plan, data, cap=None):
    """host bytes / uint8 array -> numpy uint8 container"""
    import numpy as np
    a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                             dtype=np.uint8)
    cap = container_bound(a.size, plan.n) if cap is None else int(cap)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_ulonglong(0)
    _chk("glcContainerCompress", _ct().glcContainerCompress(plan.handle, a.ctypes.data if a.size else None, a.size,
                                                            out.ctypes.data, cap, C.byref(n)))
    return out[:n.value]


def container_decompress_host(plan, data, cap=None):
    """host container -> numpy uint8 array of the decoded bytes"""
    import numpy as np
    a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                             dtype=np.uint8)
    if cap is None:
        cap = container_total_len(a) if a.size >= CONTAINER_HEADER_BYTES else 0
    out = np.zeros(max(int(cap), 1), dtype=np.uint8)
    n = C.c_ulonglong(0)
    _chk("glcContainerDecompress", _ct().glcContainerDecompress(plan.handle, a.ctypes.data if a.size else None, a.size,
                                                                out.ctypes.data, int(cap), C.byref(n)))
    return out[:n.value]


def container_compress_file(plan, src, dst):
    _chk("glcContainerCompressFile", _ct().glcContainerCompressFile(plan.handle, os.fsencode(src), os.fsencode(dst)))


def container_decompress_file(plan, src, dst):
    _chk("glcContainerDecompressFile", _ct().glcContainerDecompressFile(plan.handle, os.fsencode(src), os.fsencode(dst)))


def _get_uint(name, plan):
    """a glcPlanGetContainer* entry: the setting as an int"""
    v = C.c_uint(0)
    _chk(name, getattr(_ct(), name)(plan.handle, C.byref(v)))
    return int(v.value)


def container_set_shuffle(plan, elem):
    """the byte-plane shuffle filter of the plan's container ENCODER: elem 2, 4 or 8 (format version 2), 0 or 1 = off (the
    default: version 1).  The decoder reads the element size from the stream and ignores this setting."""
    _chk("glcPlanSetContainerShuffle", _ct().glcPlanSetContainerShuffle(plan.handle, int(elem)))


def container_get_shuffle(plan):
    return _get_uint("glcPlanGetContainerShuffle", plan)


def container_set_codec(plan, codec):
    """the codec of the plan's container ENCODER: CONTAINER_CODEC_BWT (the default: format version 1 / 2) or CONTAINER_CODEC_HUFF0
    (order-0 Huffman records, format version 3), or CONTAINER_CODEC_CHOOSE (one of the two per block, from the bigram probe; format
    version 3 as well, frames cut where the choice changes; needs the filter off and takes no mode).  The decoder reads what was
    done from the stream and ignores this setting."""
    _chk("glcPlanSetContainerCodec", _ct().glcPlanSetContainerCodec(plan.handle, int(codec)))


def container_get_codec(plan):
    return _get_uint("glcPlanGetContainerCodec", plan)


def container_set_delta(plan, on):
    """the delta mode of the plan's container ENCODER filter (format version 4): True / 1 needs the shuffle on (elem 2, 4 or 8);
    container_set_shuffle(plan, 0) also switches it off.  The decoder reads what was done from the stream."""
    _chk("glcPlanSetContainerDelta", _ct().glcPlanSetContainerDelta(plan.handle, int(on)))


def container_get_delta(plan):
    return _get_uint("glcPlanGetContainerDelta", plan)


def container_set_sparse(plan, on):
    """the sparse mode of the plan's container ENCODER (format version 5): True / 1 needs the order-0 codec;
    container_set_codec(plan, CONTAINER_CODEC_BWT) also switches it off.  It is also the version the plan reads: on, versions 1
    to 5; off, versions 1 to 4, and a version-5 stream is a stream-header failure as it always was."""
    _chk("glcPlanSetContainerSparse", _ct().glcPlanSetContainerSparse(plan.handle, int(on)))


def container_get_sparse(plan):
    return _get_uint("glcPlanGetContainerSparse", plan)


def container_set_runs(plan, on):
    """the runs mode of the plan's container ENCODER (format version 6): True / 1 needs the BWT codec;
    container_set_codec(plan, CONTAINER_CODEC_HUFF0) also switches it off.  It is also the version the plan reads: on, versions 1
    to 4 and 6; off, a version-6 stream is a stream-header failure as it always was."""
    _chk("glcPlanSetContainerRuns", _ct().glcPlanSetContainerRuns(plan.handle, int(on)))


def container_get_runs(plan):
    return _get_uint("glcPlanGetContainerRuns", plan)


def container_set_ans(plan, on):
    """the rANS mode of the plan's container ENCODER (format version 7): True / 1 needs the order-0 codec and the sparse mode off;
    container_set_codec(plan, CONTAINER_CODEC_BWT) also switches it off.  It is also the version the plan reads: on, versions 1
    to 4 and 7; off, a version-7 stream is a stream-header failure as it always was."""
    _chk("glcPlanSetContainerAns", _ct().glcPlanSetContainerAns(plan.handle, int(on)))


def container_get_ans(plan):
    return _get_uint("glcPlanGetContainerAns", plan)


def container_set_auto(plan, on):
    """the auto mode of the plan's container ENCODER (format version 8: a kind per block out of 2, 3 and 5, from one probe pass):
    True / 1 needs the order-0 codec and the sparse and rANS modes off; container_set_codec(plan, CONTAINER_CODEC_BWT) also
    switches it off.  It is also the version the plan reads: on, versions 1 to 5, 7 and 8; off, a version-8 stream is a
    stream-header failure as it always was."""
    _chk("glcPlanSetContainerAuto", _ct().glcPlanSetContainerAuto(plan.handle, int(on)))


def container_get_auto(plan):
    return _get_uint("glcPlanGetContainerAuto", plan)


def container_set_filter_auto(plan, on):
    """filter-auto of the plan's container ENCODER (format version 10: every frame's filter picked from the filter probe and
    named in its frame header): True / 1 needs the order-0 codec, the auto mode on and the plan's shuffle off; while it is on
    container_set_shuffle(plan, 2, 4 or 8) is refused, and container_set_auto(plan, 0) or a codec change switch it off.  It is also
    the version the plan reads: on, versions 1 to 5, 7, 8 and 10; off, a version-10 stream is a stream-header failure."""
    _chk("glcPlanSetContainerFilterAuto", _ct().glcPlanSetContainerFilterAuto(plan.handle, int(on)))


def container_get_filter_auto(plan):
    return _get_uint("glcPlanGetContainerFilterAuto", plan)


def container_set_filter_lag(plan, on):
    """filter-lag of the plan's container ENCODER (format version 13: filter-auto also weighs the lagged, folded delta at the lag
    the lag probe finds per frame): True / 1 needs filter-auto on, and whatever switches filter-auto off switches it off.  It is
    also the version the plan reads: on, versions 1 to 5, 7, 8, 10 and 13; off, a version-13 stream is a stream-header failure."""
    _chk("glcPlanSetContainerFilterLag", _ct().glcPlanSetContainerFilterLag(plan.handle, int(on)))


def container_get_filter_lag(plan):
    return _get_uint("glcPlanGetContainerFilterLag", plan)


def container_last_lag_filters(plan):
    """(frames that took the lag candidate of elem 2, of elem 4, of elem 8, their sum) of the plan's last successful compress"""
    a = (C.c_ulonglong * 4)()
    _chk("glcContainerLastLagFilters", _ct().glcContainerLastLagFilters(plan.handle, a))
    return tuple(int(v) for v in a)


def container_set_filter_grid(plan, on):
    """filter-grid of the plan's container ENCODER (format version 14: filter-lag also weighs the 2-D predictor at the row width
    the grid probe finds per frame): True / 1 needs filter-lag on, and whatever switches filter-lag off switches it off.  It is
    also the version the plan reads: on, versions 1 to 5, 7, 8, 10, 13 and 14; off, a version-14 stream is a stream-header failure."""
    _chk("glcPlanSetContainerFilterGrid", _ct().glcPlanSetContainerFilterGrid(plan.handle, int(on)))


def container_get_filter_grid(plan):
    return _get_uint("glcPlanGetContainerFilterGrid", plan)


def container_last_grid_filters(plan):
    """(frames that took the grid candidate of elem 2, of elem 4, of elem 8, their sum) of the plan's last successful compress"""
    a = (C.c_ulonglong * 4)()
    _chk("glcContainerLastGridFilters", _ct().glcContainerLastGridFilters(plan.handle, a))
    return tuple(int(v) for v in a)


def container_set_filter_byte(plan, on):
    """filter-byte of the plan's container ENCODER (format version 16: filter-grid also weighs the byte predictor at the lag and the
    row stride the byte probe finds per frame): True / 1 needs filter-grid on, and whatever switches filter-grid off switches it
    off.  It is also the version the plan reads: on, versions 1 to 5, 7, 8, 10, 13, 14 and 16; off, a version-16 stream is a
    stream-header failure."""
    _chk("glcPlanSetContainerFilterByte", _ct().glcPlanSetContainerFilterByte(plan.handle, int(on)))


def container_get_filter_byte(plan):
    return _get_uint("glcPlanGetContainerFilterByte", plan)


def container_set_choose_filters(plan, level):
    """glcPlanSetContainerChooseFilters: what the CHOOSE codec's order-0 frames take -- 0 (the default) today's CHOOSE, version 3;
    1 the auto mode, version 8; 2 to 5 filter-auto, filter-lag, filter-grid and filter-byte on top, versions 10, 13, 14 and 16, the
    frames cut by class (typed with an element size, BWT, order-0).  Legal only while the codec is CHOOSE; every
    container_set_codec call puts it back to 0.  It is also what the plan reads: the level's version and what an order-0 plan
    with the same settings reads."""
    _chk("glcPlanSetContainerChooseFilters", _ct().glcPlanSetContainerChooseFilters(plan.handle, int(level)))


def container_get_choose_filters(plan):
    return _get_uint("glcPlanGetContainerChooseFilters", plan)


def container_last_byte_filters(plan):
    """(frames that took the byte candidate at (lag, 0), at (lag, stride), their sum) of the plan's last successful compress"""
    a = (C.c_ulonglong * 3)()
    _chk("glcContainerLastByteFilters", _ct().glcContainerLastByteFilters(plan.handle, a))
    return tuple(int(v) for v in a)


def container_set_delta_lag(plan, lag, fold):
    """the lag and fold of the delta of the plan's container ENCODER (format version 11: the predecessor `lag` elements back, the
    sign folded into bit 0 where fold is 1); (1, 0) is off.  Anything else needs the order-0 codec, the auto mode, the shuffle
    and the delta on and filter-auto off, and whatever ends one of them puts it back to (1, 0).  It is also the version the plan
    reads: on, versions 1 to 5, 7, 8 and 11; off, a version-11 stream is a stream-header failure."""
    _chk("glcPlanSetContainerDeltaLag", _ct().glcPlanSetContainerDeltaLag(plan.handle, int(lag), int(fold)))


def container_get_delta_lag(plan):
    lag, fold = C.c_uint(0), C.c_uint(0)
    _chk("glcPlanGetContainerDeltaLag", _ct().glcPlanGetContainerDeltaLag(plan.handle, C.byref(lag), C.byref(fold)))
    return int(lag.value), int(fold.value)


def container_set_delta_grid(plan, width, fold):
    """the row width and fold of the 2-D predictor of the plan's container ENCODER (format version 12: the delta over the
    differences to the element `width` places back, the row above; the sign folded into bit 0 where fold is 1); width 0 is off.
    Any other width (2 to 65536) needs the order-0 codec, the auto mode, the shuffle and the delta on, filter-auto off and the
    delta-lag setting at (1, 0), and whatever ends one of them puts it back to off.  It is also the version the plan reads: on,
    versions 1 to 5, 7, 8 and 12; off, a version-12 stream is a stream-header failure."""
    _chk("glcPlanSetContainerDeltaGrid", _ct().glcPlanSetContainerDeltaGrid(plan.handle, int(width), int(fold)))


def container_get_delta_grid(plan):
    width, fold = C.c_uint(0), C.c_uint(0)
    _chk("glcPlanGetContainerDeltaGrid", _ct().glcPlanGetContainerDeltaGrid(plan.handle, C.byref(width), C.byref(fold)))
    return int(width.value), int(fold.value)


def container_set_byte_delta(plan, lag, stride):
    """the lag and row stride of the byte predictor of the plan's container ENCODER (format version 15, for 8-bit sample data: the
    predecessor `lag` bytes back, 1 to 16, the channel count, over the differences to the byte `stride` back, 0 for none or 2 to
    65536, the row length in bytes); lag 0 is off.  On needs the order-0 codec, the auto mode on, the shuffle off and filter-auto
    off; while it is on the shuffle and filter-auto are refused, and a codec change or the auto mode going off switches it off.  It
    is also the version the plan reads: on, versions 1 to 5, 7, 8 and 15; off, a version-15 stream is a stream-header failure."""
    _chk("glcPlanSetContainerByteDelta", _ct().glcPlanSetContainerByteDelta(plan.handle, int(lag), int(stride)))


def container_get_byte_delta(plan):
    lag, stride = C.c_uint(0), C.c_uint(0)
    _chk("glcPlanGetContainerByteDelta", _ct().glcPlanGetContainerByteDelta(plan.handle, C.byref(lag), C.byref(stride)))
    return int(lag.value), int(stride.value)


def container_set_delta_volume(plan, plane):
    """the plane stride of the 3-D predictor of the plan's container ENCODER (format version 17: the 2-D predictor over the
    differences to the element `plane` places back, the plane behind); 0 is off.  Any other plane (up to 2^24) needs the grid
    setting on at a width below it; whatever switches that off switches this off, and while it is on a grid width >= plane is
    refused.  It is also the version the plan reads: on, versions 1 to 5, 7, 8, 12 and 17; off, a version-17 stream is a
    stream-header failure."""
    _chk("glcPlanSetContainerDeltaVolume", _ct().glcPlanSetContainerDeltaVolume(plan.handle, int(plane)))


def container_get_delta_volume(plan):
    plane = C.c_uint(0)
    _chk("glcPlanGetContainerDeltaVolume", _ct().glcPlanGetContainerDeltaVolume(plan.handle, C.byref(plane)))
    return int(plane.value)


def container_last_filters(plan):
    """(frames per candidate of FILTER_CANDS ..., frames) of the plan's last successful container compress: eight integers"""
    a = (C.c_ulonglong * 8)()
    _chk("glcContainerLastFilters", _ct().glcContainerLastFilters(plan.handle, a))
    return tuple(int(v) for v in a)


def container_set_dedup(plan, on):
    """the dedup mode of the plan's container ENCODER (format version 9: 512-byte chunks that repeat an earlier chunk of their frame
    are elided, kind 6): True / 1 needs the order-0 codec and the sparse, rANS and auto modes off; a codec change also switches it
    off.  It is also the version the plan reads: on, versions 1 to 4 and 9; off, a version-9 stream is a stream-header failure as it
    always was."""
    _chk("glcPlanSetContainerDedup", _ct().glcPlanSetContainerDedup(plan.handle, int(on)))


def container_get_dedup(plan):
    return _get_uint("glcPlanGetContainerDedup", plan)


# --- the segment helpers ------------------------------------------------------------------------------------------------------
# The *Segments entries only enqueue on `stream` (None, a raw hipStream_t or a torch.cuda.Stream).  The helpers below upload the
# segment lists and allocate work memory per call, so by default each ends with a wait for the whole device, behind which those
# temporaries may die.  A caller that wants the entry's own behaviour -- nothing but the enqueue, on its stream -- passes
# keep=[...]: the helper then does not wait and appends its temporaries to the list, which the caller holds until it has
# synchronised; and it passes offsets / lengths / fills as SegmentList, uploaded ahead of the call, so that the helper copies
# nothing either (a copy from pageable memory waits for the stream it is queued on).
class SegmentList(list):
    """a list of segment offsets, lengths or fill bytes together with its device copy (`tensor`), made here"""

    def __init__(self, values, device, dtype=None):
        import torch
        super().__init__(int(v) for v in values)
        self.tensor = torch.as_tensor(list(self), dtype=torch.int64 if dtype is None else dtype).to(device)


def _seg_tensor(values, dtype, dev):
    import torch
    t = getattr(values, "tensor", None)
    if t is None:
        return torch.as_tensor(values, dtype=dtype).to(dev)
    assert t.dtype == dtype and t.device == torch.device(dev), "a SegmentList of another type or device"
    return t


def _seg_done(dev, keep, *temps):
    import torch
    if keep is None:
        torch.cuda.synchronize(dev)                            # (the temporaries of the call die behind it)
    else:
        keep.extend(temps)


def probe_segments(d_in, offsets, lengths, max_len=None, hist=None, uniform=None, stream=None, keep=None):
    """the probe of the auto mode over the segments [offsets[i], + min(lengths[i], max_len)) of the device uint8 tensor d_in:
    (hist, uniform), int32 tensors [count, 256] -- the byte counts, and per byte value the 64-byte chunks (cut from the segment's
    start) made of that byte alone.  hist / uniform: tensors to write into (they need not be zeroed)."""
    import torch
    dev = d_in.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    n = off.numel()
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    hist = torch.empty((max(1, n), 256), dtype=torch.int32, device=dev) if hist is None else hist
    uniform = torch.empty((max(1, n), 256), dtype=torch.int32, device=dev) if uniform is None else uniform
    assert hist.is_contiguous() and uniform.is_contiguous() and hist.numel() >= 256 * n and uniform.numel() >= 256 * n
    _chk("glcProbeSegments", _ct().glcProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len, hist.data_ptr(),
                                                     uniform.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return hist[:n], uniform[:n]


def bigram_probe_segments(d_in, offsets, lengths, max_len=None, stats=None, stream=None, keep=None):
    """the bigram probe of CONTAINER_CODEC_CHOOSE over the segments [offsets[i], + min(lengths[i], max_len)) of the device uint8
    tensor d_in: an int64 tensor [count, 4] of rows {S2, SR, SC, M} (csrc/choose_rule.h).  stats: a tensor to write into."""
    import torch
    dev = d_in.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    n = off.numel()
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    stats = torch.empty((max(1, n), 4), dtype=torch.int64, device=dev) if stats is None else stats
    assert stats.is_contiguous() and stats.dtype == torch.int64 and stats.numel() >= 4 * n
    _chk("glcBigramProbeSegments", _ct().glcBigramProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len,
                                                                 stats.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return stats[:n]


FILTER_PROBE_ROWS, FILTER_CANDIDATES, FILTER_PROBE_MAX_LEN = 22, 7, 1 << 31
FILTER_CANDS = ((1, 0), (2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 1))     # (elem, delta) in the rule's order; (1, 0): no filter


def filter_probe_segments(d_in, offsets, lengths, max_len=None, planes=None, costs=None, stream=None, keep=None):
    """the filter probe over the segments [offsets[i], + min(lengths[i], max_len)) of the device uint8 tensor d_in: (planes,
    costs) -- an int32 tensor [count, 22, 256] of the histograms A_0..7, D_2, D_4 and D_8 of each segment's first L - L % 8 bytes,
    and an int64 tensor [count, 7] of the candidates' costs in the order of FILTER_CANDS (csrc/filter_rule.h).  planes / costs:
    tensors to write into (they need not be zeroed)."""
    import torch
    dev = d_in.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    n = off.numel()
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    planes = torch.empty((max(1, n), FILTER_PROBE_ROWS, 256), dtype=torch.int32, device=dev) if planes is None else planes
    costs = torch.empty((max(1, n), FILTER_CANDIDATES), dtype=torch.int64, device=dev) if costs is None else costs
    assert planes.is_contiguous() and costs.is_contiguous() and costs.dtype == torch.int64
    assert planes.numel() >= FILTER_PROBE_ROWS * 256 * n and costs.numel() >= FILTER_CANDIDATES * n
    _chk("glcFilterProbeSegments", _ct().glcFilterProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len,
                                                                 planes.data_ptr(), costs.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return planes[:n], costs[:n]


LAG_PROBE_SUMS, LAG_PROBE_ROWS, LAG_PROBE_MAX_LAG = 48, 14, 16


def _lag_probe_args(d_in, offsets, lengths, max_len):
    import torch
    dev = d_in.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    return dev, off, ln, off.numel(), int(max(lengths, default=0)) if max_len is None else int(max_len)


def lag_probe_segments(d_in, offsets, lengths, max_len=None, sums=None, lags=None, stream=None, keep=None):
    """the lag probe over the segments [offsets[i], + min(lengths[i], max_len)) of the device uint8 tensor d_in: (sums, lags) --
    an int64 tensor [count, 48] of the bit lengths S[e][l] of the folded differences at element size e = 2, 4, 8 and lag
    l = 1 .. 16 (row (log2 e - 1) * 16 + l - 1) over each segment's first L - L % 8 bytes, and an int32 tensor [count, 3] of the
    lag with the smallest sum per element size (csrc/lag_rule.h).  sums / lags: tensors to write into (they need not be zeroed)."""
    import torch
    dev, off, ln, n, max_len = _lag_probe_args(d_in, offsets, lengths, max_len)
    sums = torch.empty((max(1, n), LAG_PROBE_SUMS), dtype=torch.int64, device=dev) if sums is None else sums
    lags = torch.empty((max(1, n), 3), dtype=torch.int32, device=dev) if lags is None else lags
    assert sums.is_contiguous() and lags.is_contiguous() and sums.dtype == torch.int64 and lags.dtype == torch.int32
    assert sums.numel() >= LAG_PROBE_SUMS * n and lags.numel() >= 3 * n
    _chk("glcLagProbeSegments", _ct().glcLagProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len,
                                                           sums.data_ptr(), lags.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return sums[:n], lags[:n]


def lag_planes_segments(d_in, offsets, lengths, lags, max_len=None, planes=None, costs=None, stream=None, keep=None):
    """the plane probe of the lag rule over the same segments at the lags of the device int32 tensor `lags` [count, 3] (each word
    used as ((v - 1) & 15) + 1): (planes, costs) -- an int32 tensor [count, 14, 256] of the histograms E_2, E_4 and E_8 and an
    int64 tensor [count, 3] of their costs.  planes / costs: tensors to write into (they need not be zeroed)."""
    import torch
    dev, off, ln, n, max_len = _lag_probe_args(d_in, offsets, lengths, max_len)
    planes = torch.empty((max(1, n), LAG_PROBE_ROWS, 256), dtype=torch.int32, device=dev) if planes is None else planes
    costs = torch.empty((max(1, n), 3), dtype=torch.int64, device=dev) if costs is None else costs
    assert planes.is_contiguous() and costs.is_contiguous() and costs.dtype == torch.int64
    assert lags.is_contiguous() and lags.dtype == torch.int32 and lags.numel() >= 3 * n
    assert planes.numel() >= LAG_PROBE_ROWS * 256 * n and costs.numel() >= 3 * n
    _chk("glcLagPlanesSegments", _ct().glcLagPlanesSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len, lags.data_ptr(),
                                                             planes.data_ptr(), costs.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return planes[:n], costs[:n]


GRID_PROBE_ROW, GRID_PROBE_SUMS = 65537, 3 * 65537


def grid_probe_segments(d_in, offsets, lengths, max_len=None, sums=None, widths=None, stream=None, keep=None):
    """the grid probe over the segments [offsets[i], + min(lengths[i], max_len)) of the device uint8 tensor d_in: (sums, widths) --
    an int32 tensor [count, 3 * 65537] whose word k * 65537 + W is S_e[W] for e = 2 << k (the bit pattern 0xFFFFFFFF, so -1, where W
    is no candidate), and an int32 tensor [count, 3] of the width with the smallest sum per element size, 0 where there is none
    (csrc/grid_rule.h).  sums / widths: tensors to write into (they need not be zeroed)."""
    import torch
    dev, off, ln, n, max_len = _lag_probe_args(d_in, offsets, lengths, max_len)
    sums = torch.empty((max(1, n), GRID_PROBE_SUMS), dtype=torch.int32, device=dev) if sums is None else sums
    widths = torch.empty((max(1, n), 3), dtype=torch.int32, device=dev) if widths is None else widths
    assert sums.is_contiguous() and widths.is_contiguous() and sums.dtype == torch.int32 and widths.dtype == torch.int32
    assert sums.numel() >= GRID_PROBE_SUMS * n and widths.numel() >= 3 * n
    _chk("glcGridProbeSegments", _ct().glcGridProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len,
                                                             sums.data_ptr(), widths.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return sums[:n], widths[:n]


def grid_planes_segments(d_in, offsets, lengths, widths, max_len=None, planes=None, costs=None, stream=None, keep=None):
    """the plane probe of the grid rule over the same segments at the widths of the device int32 tensor `widths` [count, 3] (a
    word outside 2..65536 names no width: zero rows and the cost 2^56): (planes, costs) -- an int32 tensor [count, 14, 256] and an
    int64 tensor [count, 3].  planes / costs: tensors to write into (they need not be zeroed)."""
    import torch
    dev, off, ln, n, max_len = _lag_probe_args(d_in, offsets, lengths, max_len)
    planes = torch.empty((max(1, n), LAG_PROBE_ROWS, 256), dtype=torch.int32, device=dev) if planes is None else planes
    costs = torch.empty((max(1, n), 3), dtype=torch.int64, device=dev) if costs is None else costs
    assert planes.is_contiguous() and costs.is_contiguous() and costs.dtype == torch.int64
    assert widths.is_contiguous() and widths.dtype == torch.int32 and widths.numel() >= 3 * n
    assert planes.numel() >= LAG_PROBE_ROWS * 256 * n and costs.numel() >= 3 * n
    _chk("glcGridPlanesSegments", _ct().glcGridPlanesSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len, widths.data_ptr(),
                                                               planes.data_ptr(), costs.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return planes[:n], costs[:n]


BYTE_PROBE_LAGS, BYTE_PROBE_ROW, BYTE_PROBE_ROWS = 16, 65537, 2


def byte_probe_segments(d_in, offsets, lengths, max_len=None, lag_sums=None, stride_sums=None, winners=None, stream=None, keep=None):
    """the byte probe over the segments [offsets[i], + min(lengths[i], max_len)) of the device uint8 tensor d_in: (lag_sums,
    stride_sums, winners) -- an int64 tensor [count, 16] of the magnitudes A[l] of the byte differences at lag l = 1 .. 16 over each
    segment's first L - L % 8 bytes, an int32 tensor [count, 65537] whose word W is S[W] for the row strides 17 .. Wmax (the bit
    pattern 0xFFFFFFFF, so -1, where W is no candidate), and an int32 tensor [count, 2] of the lag and the stride with the smallest
    sums, the stride 0 where there is none (csrc/byte_rule.h).  The outputs need not be zeroed."""
    import torch
    dev, off, ln, n, max_len = _lag_probe_args(d_in, offsets, lengths, max_len)
    lag_sums = torch.empty((max(1, n), BYTE_PROBE_LAGS), dtype=torch.int64, device=dev) if lag_sums is None else lag_sums
    stride_sums = torch.empty((max(1, n), BYTE_PROBE_ROW), dtype=torch.int32, device=dev) if stride_sums is None else stride_sums
    winners = torch.empty((max(1, n), 2), dtype=torch.int32, device=dev) if winners is None else winners
    assert lag_sums.is_contiguous() and stride_sums.is_contiguous() and winners.is_contiguous()
    assert lag_sums.dtype == torch.int64 and stride_sums.dtype == torch.int32 and winners.dtype == torch.int32
    assert lag_sums.numel() >= BYTE_PROBE_LAGS * n and stride_sums.numel() >= BYTE_PROBE_ROW * n and winners.numel() >= 2 * n
    _chk("glcByteProbeSegments", _ct().glcByteProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len,
                                                             lag_sums.data_ptr(), stride_sums.data_ptr(), winners.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return lag_sums[:n], stride_sums[:n], winners[:n]


def byte_planes_segments(d_in, offsets, lengths, words, max_len=None, planes=None, costs=None, stream=None, keep=None):
    """the plane probe of the byte rule over the same segments at the {lag, stride} words of the device int32 tensor `words`
    [count, 2] (the lag used as ((v - 1) & 15) + 1; a stride outside 17..65536 names none: a zero row and the cost 2^56):
    (planes, costs) -- an int32 tensor [count, 2, 256], the histograms of the byte predictor's output at (lag, 0) and at (lag,
    stride), and an int64 tensor [count, 2].  planes / costs: tensors to write into (they need not be zeroed)."""
    import torch
    dev, off, ln, n, max_len = _lag_probe_args(d_in, offsets, lengths, max_len)
    planes = torch.empty((max(1, n), BYTE_PROBE_ROWS, 256), dtype=torch.int32, device=dev) if planes is None else planes
    costs = torch.empty((max(1, n), BYTE_PROBE_ROWS), dtype=torch.int64, device=dev) if costs is None else costs
    assert planes.is_contiguous() and costs.is_contiguous() and costs.dtype == torch.int64
    assert words.is_contiguous() and words.dtype == torch.int32 and words.numel() >= 2 * n
    assert planes.numel() >= BYTE_PROBE_ROWS * 256 * n and costs.numel() >= BYTE_PROBE_ROWS * n
    _chk("glcBytePlanesSegments", _ct().glcBytePlanesSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len, words.data_ptr(),
                                                               planes.data_ptr(), costs.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return planes[:n], costs[:n]


def ans_bound_words(length):
    """words of room the record of a segment of `length` bytes may need"""
    return int(_ct().glcAnsBoundWords(int(length)))


def ans_work_bytes(count, max_len):
    return int(_ct().glcAnsSegmentsWorkBytes(int(count), int(max_len)))


def _ans_args(d_base, offsets, lengths, max_len):
    import torch
    dev = d_base.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    work = torch.empty(max(16, ans_work_bytes(off.numel(), max_len)), dtype=torch.uint8, device=dev)
    return off, ln, max_len, work


def ans_encode_segments(d_in, offsets, lengths, max_len=None, stream=None, keep=None, rec_off=None):
    """the segments [offsets[i], + lengths[i]) of the device uint8 tensor d_in as rANS records (format version 7, kind 5).
    Returns (hist int32 tensor [count, 256], records int32 tensor, record word offsets (list), record words int64 tensor
    [count]); record i is records[rec_off[i] : rec_off[i] + words[i]]"""
    import torch
    off, ln, max_len, work = _ans_args(d_in, offsets, lengths, max_len)
    n = off.numel()
    offs, total = [], 0
    for l in lengths:
        offs.append(total)
        total += ans_bound_words(min(int(l), max_len))
    assert rec_off is None or list(rec_off) == offs            # (rec_off: these offsets as a SegmentList, uploaded ahead of the call)
    rec_off = offs if rec_off is None else rec_off
    ro = _seg_tensor(rec_off, torch.int64, d_in.device)
    hist = torch.zeros((max(1, n), 256), dtype=torch.int32, device=d_in.device)
    rec = torch.zeros(max(1, total), dtype=torch.int32, device=d_in.device)
    words = torch.zeros(max(1, n), dtype=torch.int64, device=d_in.device)
    _chk("glcAnsEncodeSegments", _ct().glcAnsEncodeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), n, max_len, hist.data_ptr(),
                                                             rec.data_ptr(), ro.data_ptr(), words.data_ptr(), work.data_ptr(),
                                                             work.numel(), _stream_ptr(stream)))
    _seg_done(d_in.device, keep, off, ln, ro, work)
    return hist[:n], rec, rec_off, words[:n]


def ans_decode_segments(rec, rec_off, words, hist, d_out, offsets, lengths, max_len=None, stream=None, keep=None):
    """the inverse of ans_encode_segments into the device uint8 tensor d_out; tolerant of whatever rec and words hold"""
    import torch
    off, ln, max_len, work = _ans_args(d_out, offsets, lengths, max_len)
    ro = _seg_tensor(rec_off, torch.int64, d_out.device)
    wd = _seg_tensor(words, torch.int64, d_out.device)
    h = hist.contiguous()
    assert ro.numel() == wd.numel() == off.numel() and h.numel() == 256 * off.numel()
    _chk("glcAnsDecodeSegments", _ct().glcAnsDecodeSegments(rec.data_ptr(), ro.data_ptr(), wd.data_ptr(), h.data_ptr(), off.data_ptr(),
                                                             ln.data_ptr(), off.numel(), max_len, d_out.data_ptr(), work.data_ptr(),
                                                             work.numel(), _stream_ptr(stream)))
    _seg_done(d_out.device, keep, off, ln, ro, wd, h, work)
    return d_out


def _zerorun_args(d_base, offsets, lengths):
    import torch
    off = _seg_tensor(offsets, torch.int64, d_base.device)
    ln = _seg_tensor(lengths, torch.int64, d_base.device)
    assert off.numel() == ln.numel()
    return off, ln


def zerorun_split_segments(d_in, d_a, d_b, offsets, lengths, max_len=None, stream=None, keep=None):
    """the segments [offsets[i], + lengths[i]) of the device uint8 tensor d_in split into A (non-zero bytes and one zero per run
    of zeros, a run ending at a 256-byte tile edge) at d_a + offsets[i] and B (run lengths minus one) at d_b + offsets[i].
    Returns (A lengths, B lengths), int64 tensors [count]"""
    import torch
    off, ln = _zerorun_args(d_in, offsets, lengths)
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    alen = torch.zeros(max(1, off.numel()), dtype=torch.int64, device=d_in.device)
    blen = torch.zeros(max(1, off.numel()), dtype=torch.int64, device=d_in.device)
    _chk("glcZeroRunSplitSegments", _ct().glcZeroRunSplitSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), max_len,
                                                                   d_a.data_ptr(), d_b.data_ptr(), alen.data_ptr(), blen.data_ptr(), _stream_ptr(stream)))
    _seg_done(d_in.device, keep, off, ln)
    return alen[:off.numel()], blen[:off.numel()]


def zerorun_join_segments(d_a, d_b, d_out, offsets, a_lengths, b_lengths, lengths, max_len=None, stream=None, keep=None):
    """the inverse of zerorun_split_segments; tolerant of streams that do not fit each other (see include/glc_container.h)"""
    import torch
    off, ln = _zerorun_args(d_out, offsets, lengths)
    al = _seg_tensor(a_lengths, torch.int64, d_out.device)
    bl = _seg_tensor(b_lengths, torch.int64, d_out.device)
    assert al.numel() == bl.numel() == off.numel()
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    _chk("glcZeroRunJoinSegments", _ct().glcZeroRunJoinSegments(d_a.data_ptr(), d_b.data_ptr(), off.data_ptr(), al.data_ptr(), bl.data_ptr(),
                                                                 ln.data_ptr(), off.numel(), max_len, d_out.data_ptr(), _stream_ptr(stream)))
    _seg_done(d_out.device, keep, off, ln, al, bl)
    return d_out


def sparse_mask_words(max_len):
    return ((int(max_len) + 63) // 64 + 31) // 32


def _sparse_args(d_base, offsets, lengths, fill):
    import torch
    dev = d_base.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    fl = _seg_tensor(fill, torch.int32, dev)
    assert off.numel() == ln.numel() == fl.numel()
    return off, ln, fl


def sparse_split_segments(d_in, d_kept, offsets, lengths, fill, max_len=None, stream=None, keep=None):
    """the segments [offsets[i], + lengths[i]) of the device uint8 tensor d_in, cut into 64-byte chunks: the chunks that are not
    all fill[i] go, in order, to d_kept at offsets[i].  Returns (mask int32 tensor [count, sparse_mask_words(max_len)], kept
    lengths int64 tensor [count])"""
    import torch
    off, ln, fl = _sparse_args(d_in, offsets, lengths, fill)
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    mask = torch.zeros((off.numel(), max(1, sparse_mask_words(max_len))), dtype=torch.int32, device=d_in.device)
    klen = torch.zeros(max(1, off.numel()), dtype=torch.int64, device=d_in.device)
    _chk("glcSparseSplitSegments", _ct().glcSparseSplitSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), max_len,
                                                                 fl.data_ptr(), mask.data_ptr(), d_kept.data_ptr(), klen.data_ptr(), _stream_ptr(stream)))
    _seg_done(d_in.device, keep, off, ln, fl)
    return mask[:, :sparse_mask_words(max_len)], klen[:off.numel()]


def sparse_join_segments(d_kept, d_out, offsets, lengths, fill, mask, max_len=None, stream=None, keep=None):
    """the inverse of sparse_split_segments: `mask` is its mask tensor (rows of sparse_mask_words(max_len) words)"""
    import torch
    off, ln, fl = _sparse_args(d_kept, offsets, lengths, fill)
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    m = mask.contiguous()
    assert m.numel() == off.numel() * sparse_mask_words(max_len) or sparse_mask_words(max_len) == 0
    _chk("glcSparseJoinSegments", _ct().glcSparseJoinSegments(d_kept.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), max_len,
                                                               fl.data_ptr(), m.data_ptr(), d_out.data_ptr(), _stream_ptr(stream)))
    _seg_done(d_kept.device, keep, off, ln, fl, m)
    return d_out


DEDUP_CHUNK = 512


def dedup_chunks(max_len):
    return (int(max_len) + DEDUP_CHUNK - 1) // DEDUP_CHUNK


def dedup_map_segments(d_base, offsets, lengths, max_len=None, stream=None, keep=None):
    """the segments [offsets[i], + lengths[i]) of the device uint8 tensor d_base as the blocks of one frame, cut into 512-byte
    chunks: an int32 tensor [count * dedup_chunks(max_len)] with, for chunk c of segment i at i * nch + c, the id of the earlier
    chunk it repeats under the writer's rule, or its own id"""
    import torch
    dev = d_base.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    L = _ct()
    src = torch.zeros(max(1, off.numel() * dedup_chunks(max_len)), dtype=torch.int32, device=dev)
    work = torch.empty(max(16, int(L.glcDedupWorkBytes(off.numel(), max_len))), dtype=torch.uint8, device=dev)
    _chk("glcDedupMapSegments", L.glcDedupMapSegments(d_base.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), max_len, src.data_ptr(),
                                                      work.data_ptr(), work.numel(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln, work)
    return src[:off.numel() * dedup_chunks(max_len)]


def dedup_fill_segments(d_out, offsets, lengths, src, max_len=None, stream=None, keep=None):
    """the inverse of dedup_map_segments, in place: every chunk whose entry of `src` is not its own id is copied from the chunk the
    entry names"""
    import torch
    dev = d_out.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    max_len = int(max(lengths, default=0)) if max_len is None else int(max_len)
    s = src.contiguous()
    assert s.numel() == off.numel() * dedup_chunks(max_len)
    _chk("glcDedupFillSegments", _ct().glcDedupFillSegments(d_out.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), max_len,
                                                             s.data_ptr() if s.numel() else None, _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln, s)
    return d_out


def _shuffle(fn, d_in, elem, out, stream):
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == x.numel()
    _chk(fn, getattr(_ct(), fn)(x.data_ptr() if x.numel() else None, out.data_ptr() if x.numel() else None, x.numel(), int(elem), _stream_ptr(stream)))
    return out


def shuffle(d_in, elem, out=None, stream=None):
    """byte-plane shuffle of a device uint8 tensor (elem 2, 4 or 8): byte j of every element gathered into plane j, the last
    numel % elem bytes in place; into `out` (same size, not overlapping) or a new tensor.  Queued on `stream` (None = default)."""
    return _shuffle("glcShuffleDevice", d_in, elem, out, stream)


def unshuffle(d_in, elem, out=None, stream=None):
    """the inverse of shuffle"""
    return _shuffle("glcUnshuffleDevice", d_in, elem, out, stream)


def delta_shuffle(d_in, elem, out=None, stream=None):
    """shuffle of the differences of neighbouring elements (little-endian unsigned, modulo 2^(8 elem), restarting every 2048
    elements) in one pass; the rules of shuffle"""
    return _shuffle("glcDeltaShuffleDevice", d_in, elem, out, stream)


def undelta_unshuffle(d_in, elem, out=None, stream=None):
    """the inverse of delta_shuffle"""
    return _shuffle("glcUndeltaUnshuffleDevice", d_in, elem, out, stream)


def _lag_shuffle(fn, d_in, elem, lag, fold, out, stream):
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == x.numel()
    _chk(fn, getattr(_ct(), fn)(x.data_ptr() if x.numel() else None, out.data_ptr() if x.numel() else None, x.numel(), int(elem), int(lag),
                                int(fold), _stream_ptr(stream)))
    return out


def lag_delta_shuffle(d_in, elem, lag, fold, out=None, stream=None):
    """delta_shuffle with the predecessor `lag` elements back (1 to 16: the channel count of interleaved data) and, where fold is
    1, the difference's sign folded into bit 0; (1, 0) is delta_shuffle.  The rules of shuffle"""
    return _lag_shuffle("glcLagDeltaShuffleDevice", d_in, elem, lag, fold, out, stream)


def unlag_delta_unshuffle(d_in, elem, lag, fold, out=None, stream=None):
    """the inverse of lag_delta_shuffle"""
    return _lag_shuffle("glcUnlagDeltaUnshuffleDevice", d_in, elem, lag, fold, out, stream)


def grid_delta_shuffle(d_in, elem, width, fold, out=None, stream=None):
    """delta_shuffle over the differences to the element `width` places back (the row above of row-major gridded data, 2 to 65536
    elements wide) within bands of 2048 * ceil(width / 64) elements, the sign folded into bit 0 where fold is 1.  The rules of
    shuffle"""
    return _lag_shuffle("glcGridDeltaShuffleDevice", d_in, elem, width, fold, out, stream)


def ungrid_delta_unshuffle(d_in, elem, width, fold, out=None, stream=None):
    """the inverse of grid_delta_shuffle"""
    return _lag_shuffle("glcUngridDeltaUnshuffleDevice", d_in, elem, width, fold, out, stream)


def _byte_delta(fn, d_in, lag, stride, out, stream):
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == x.numel()
    _chk(fn, getattr(_ct(), fn)(x.data_ptr() if x.numel() else None, out.data_ptr() if x.numel() else None, x.numel(), int(lag), int(stride),
                                _stream_ptr(stream)))
    return out


def _vol_shuffle(fn, d_in, elem, width, plane, fold, out, stream):
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == x.numel()
    _chk(fn, getattr(_ct(), fn)(x.data_ptr() if x.numel() else None, out.data_ptr() if x.numel() else None, x.numel(), int(elem), int(width),
                                int(plane), int(fold), _stream_ptr(stream)))
    return out


def vol_delta_shuffle(d_in, elem, width, plane, fold, out=None, stream=None):
    """grid_delta_shuffle over the differences to the element `plane` places back (the plane behind of a row-major volume,
    width < plane <= 2^24 elements) within slabs of about 16 planes, P * ceil(16 plane / P) elements with P the grid's period.
    The rules of shuffle"""
    return _vol_shuffle("glcVolDeltaShuffleDevice", d_in, elem, width, plane, fold, out, stream)


def unvol_delta_unshuffle(d_in, elem, width, plane, fold, out=None, stream=None):
    """the inverse of vol_delta_shuffle"""
    return _vol_shuffle("glcUnvolDeltaUnshuffleDevice", d_in, elem, width, plane, fold, out, stream)


def byte_delta(d_in, lag, stride, out=None, stream=None):
    """the byte predictor over a device uint8 tensor of 8-bit samples: every byte minus the byte `lag` back (1 to 16, the channel
    count; restarting every 2048 bytes), taken over the differences to the byte `stride` back (0 for none, or 2 to 65536, the row
    length in bytes) within bands of 2048 * ceil(stride / 64) bytes; modulo 256, same length and positions.  Into `out` (same
    size, not overlapping) or a new tensor"""
    return _byte_delta("glcByteDeltaDevice", d_in, lag, stride, out, stream)


def unbyte_delta(d_in, lag, stride, out=None, stream=None):
    """the inverse of byte_delta"""
    return _byte_delta("glcUnbyteDeltaDevice", d_in, lag, stride, out, stream)


def shuffle_segments(d_in, d_out, offsets, lengths, elem, inverse=False, stream=None, keep=None):
    """shuffle (or unshuffle) the segments [offsets[i], + lengths[i]) of the device uint8 tensor d_in into the same ranges of d_out"""
    import torch
    dev = d_in.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    fn = "glcUnshuffleSegments" if inverse else "glcShuffleSegments"
    _chk(fn, getattr(_ct(), fn)(d_in.data_ptr(), d_out.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(), int(elem), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return d_out


def crc32_segments_device(d_base, offsets, lengths, stream=None, keep=None):
    """CRC-32 (zlib.crc32) of segments [offsets[i], + lengths[i]) of the device uint8 tensor d_base: an int32 device tensor
    [count] (the sums' bit patterns)"""
    import torch
    dev = d_base.device
    off = _seg_tensor(offsets, torch.int64, dev)
    ln = _seg_tensor(lengths, torch.int64, dev)
    assert off.numel() == ln.numel()
    out = torch.zeros(max(1, off.numel()), dtype=torch.int32, device=dev)
    _chk("glcCrc32Segments", _ct().glcCrc32Segments(d_base.data_ptr(), off.data_ptr(), ln.data_ptr(), off.numel(),
                                                    out.data_ptr(), _stream_ptr(stream)))
    _seg_done(dev, keep, off, ln)
    return out[:off.numel()]


def crc32_segments(d_base, offsets, lengths, stream=None):
    """crc32_segments_device, waited for: a list of ints"""
    return [int(v) & 0xFFFFFFFF for v in crc32_segments_device(d_base, offsets, lengths, stream).cpu().tolist()]


def container_last_error(plan):
    """(what, frame, block) of the plan's last container failure; frame / block -1 where the failure is not tied to one"""
    a = (C.c_ulonglong * 3)()
    _chk("glcContainerLastError", _ct().glcContainerLastError(plan.handle, a))
    return tuple(-1 if v == (1 << 64) - 1 else int(v) for v in a)


# --- the frame index and range reads ------------------------------------------------------------------------------------
class ContainerIndex:
    """the frame index of one container (glcContainerIndex*): freed by close() or the with statement"""

    def __init__(self, ptr):
        self.ptr = ptr

    def info(self):
        """(total_len, block_len, frames, version, flags, elem); under version 12 the last is the header's word 3, elem | width << 8"""
        a = (C.c_ulonglong * 4)()
        _chk("glcContainerIndexInfo", _ct().glcContainerIndexInfo(self.ptr, a))
        return int(a[0]), int(a[1]), int(a[2]), int(a[3]) & 0xFFFF, (int(a[3]) >> 16) & 0xFFFF, int(a[3]) >> 32

    def plane(self):
        """the plane stride of a version-17 stream's header (word 7); 0 of every other stream"""
        p = C.c_uint(0)
        _chk("glcContainerIndexPlane", _ct().glcContainerIndexPlane(self.ptr, C.byref(p)))
        return int(p.value)

    def close(self):
        if self.ptr:
            _ct().glcContainerIndexFree(self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _host_u8(data):
    import numpy as np
    return np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)


def container_index(plan, d_cont):
    """the index of a container in device memory (uint8 tensor, 8-byte aligned): the walk runs on the GPU"""
    c = d_cont.reshape(-1)
    p = C.c_void_p(None)
    _chk("glcContainerIndexDevice", _ct().glcContainerIndexDevice(plan.handle, c.data_ptr(), c.numel(), C.byref(p)))
    return ContainerIndex(p)


def container_index_host(plan, data):
    a = _host_u8(data)
    p = C.c_void_p(None)
    _chk("glcContainerIndex", _ct().glcContainerIndex(plan.handle, a.ctypes.data, a.size, C.byref(p)))
    return ContainerIndex(p)


def container_index_file(plan, path):
    p = C.c_void_p(None)
    _chk("glcContainerIndexFile", _ct().glcContainerIndexFile(plan.handle, os.fsencode(path), C.byref(p)))
    return ContainerIndex(p)


def container_read_range(plan, index, d_cont, offset, count, out=None):
    """bytes [offset, offset + count) of the input of the device container d_cont, into `out` (a device uint8 tensor of at least
    `count` bytes, any alignment) or a new tensor"""
    import torch
    c = d_cont.reshape(-1)
    if out is None:
        out = torch.empty(int(count), dtype=torch.uint8, device=c.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= count
    _chk("glcContainerReadRangeDevice", _ct().glcContainerReadRangeDevice(
        plan.handle, index.ptr if index is not None else None, c.data_ptr(), c.numel(), int(offset), int(count),
        out.data_ptr() if out.numel() else None))
    return out[:int(count)]


def container_read_range_host(plan, index, data, offset, count, out=None):
    import numpy as np
    a = _host_u8(data)
    if out is None:
        out = np.zeros(max(int(count), 1), dtype=np.uint8)
    _chk("glcContainerReadRange", _ct().glcContainerReadRange(plan.handle, index.ptr if index is not None else None, a.ctypes.data, a.size,
                                                              int(offset), int(count), out.ctypes.data))
    return out[:int(count)]


def container_read_range_file(plan, index, path, offset, count, out=None):
    import numpy as np
    if out is None:
        out = np.zeros(max(int(count), 1), dtype=np.uint8)
    _chk("glcContainerReadRangeFile", _ct().glcContainerReadRangeFile(plan.handle, index.ptr if index is not None else None,
                                                                      os.fsencode(path), int(offset), int(count), out.ctypes.data))
    return out[:int(count)]


def container_last_range_stats(plan):
    """(frames fetched, blocks decoded, container bytes fetched) of the plan's last successful range read"""
    a = (C.c_ulonglong * 3)()
    _chk("glcContainerLastRangeStats", _ct().glcContainerLastRangeStats(plan.handle, a))
    return tuple(int(v) for v in a)


def container_last_choice(plan):
    """(blocks given to the BWT codec, blocks given to the order-0 codec, frames written) of the plan's last successful container
    compress; with CONTAINER_CODEC_CHOOSE the rule's choices, counted before the record rule"""
    a = (C.c_ulonglong * 3)()
    _chk("glcContainerLastChoice", _ct().glcContainerLastChoice(plan.handle, a))
    return tuple(int(v) for v in a)


def _unshuffle_range(fn, d_in, elem, first, count, out, stream):
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty(int(count) * int(elem), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= int(count) * int(elem)
    _chk(fn, getattr(_ct(), fn)(x.data_ptr(), out.data_ptr(), x.numel(), int(elem), int(first), int(count), _stream_ptr(stream)))
    return out


def unshuffle_range(d_in, elem, first, count, out=None, stream=None):
    """elements [first, first + count) of unshuffle(d_in, elem), reading only the plane runs they come from"""
    return _unshuffle_range("glcUnshuffleRangeDevice", d_in, elem, first, count, out, stream)


def undelta_unshuffle_range(d_in, elem, first, count, out=None, stream=None):
    """elements [first, first + count) of undelta_unshuffle(d_in, elem); first a multiple of 2048"""
    return _unshuffle_range("glcUndeltaUnshuffleRangeDevice", d_in, elem, first, count, out, stream)


def unlag_delta_unshuffle_range(d_in, elem, lag, fold, first, count, out=None, stream=None):
    """elements [first, first + count) of unlag_delta_unshuffle(d_in, elem, lag, fold); first a multiple of 2048"""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty(int(count) * int(elem), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= int(count) * int(elem)
    _chk("glcUnlagDeltaUnshuffleRangeDevice", _ct().glcUnlagDeltaUnshuffleRangeDevice(
        x.data_ptr(), out.data_ptr(), x.numel(), int(elem), int(lag), int(fold), int(first), int(count), _stream_ptr(stream)))
    return out


def ungrid_delta_unshuffle_range(d_in, elem, width, fold, first, count, out=None, stream=None):
    """elements [first, first + count) of ungrid_delta_unshuffle(d_in, elem, width, fold); first a multiple of the period,
    2048 * ceil(width / 64)"""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty(int(count) * int(elem), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= int(count) * int(elem)
    _chk("glcUngridDeltaUnshuffleRangeDevice", _ct().glcUngridDeltaUnshuffleRangeDevice(
        x.data_ptr(), out.data_ptr(), x.numel(), int(elem), int(width), int(fold), int(first), int(count), _stream_ptr(stream)))
    return out


def unvol_delta_unshuffle_range(d_in, elem, width, plane, fold, first, count, out=None, stream=None):
    """elements [first, first + count) of unvol_delta_unshuffle(d_in, elem, width, plane, fold); first a multiple of the slab,
    P * ceil(16 plane / P) with P = 2048 * ceil(width / 64)"""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty(int(count) * int(elem), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= int(count) * int(elem)
    _chk("glcUnvolDeltaUnshuffleRangeDevice", _ct().glcUnvolDeltaUnshuffleRangeDevice(
        x.data_ptr(), out.data_ptr(), x.numel(), int(elem), int(width), int(plane), int(fold), int(first), int(count), _stream_ptr(stream)))
    return out


def unbyte_delta_range(d_in, lag, stride, first, count, out=None, stream=None):
    """bytes [first, first + count) of unbyte_delta(d_in, lag, stride); first a multiple of 2048 at stride 0 and of the period,
    2048 * ceil(stride / 64), otherwise"""
    import torch
    x = d_in.reshape(-1)
    assert x.dtype == torch.uint8 and x.is_contiguous()
    if out is None:
        out = torch.empty(int(count), dtype=torch.uint8, device=x.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= int(count)
    _chk("glcUnbyteDeltaRangeDevice", _ct().glcUnbyteDeltaRangeDevice(
        x.data_ptr(), out.data_ptr(), x.numel(), int(lag), int(stride), int(first), int(count), _stream_ptr(stream)))
    return out
