"""The byte-plane shuffle kernels alone against a device-to-device copy of the same bytes, in one process and interleaved:

  copy       hipMemcpyAsync, device to device, of the buffer: one read and one write per byte, the yardstick
  shuffle N  glcShuffleDevice with element size N = 2, 4, 8 on the same buffers
  unshuf N   glcUnshuffleDevice
  delta-shuffle N / undelta-unshuffle N
             glcDeltaShuffleDevice / glcUndeltaUnshuffleDevice, the fused kernels of the filter's delta mode
  lag L[f] N / unlag L[f] N   (with --lag)
             glcLagDeltaShuffleDevice / glcUnlagDeltaUnshuffleDevice (csrc/lag.hip) with lag L = 2, 3, 8, 16, f = the fold on
  lag 1f N / unlag 1f N, grid Wf N / ungrid Wf N   (with --grid W, the fold on)
             glcGridDeltaShuffleDevice / glcUngridDeltaUnshuffleDevice (csrc/grid.hip) at row width W beside the lag kernels at
             (1, 1), which the grid's expectations are stated against; k_grid_vsum takes its 16-byte path when W * N and the
             destination's address (--offset) are multiples of 16, else its element path
  vol W,Sf N / unvol W,Sf N   (with --grid W --volume S, the fold on)
             glcVolDeltaShuffleDevice / glcUnvolDeltaUnshuffleDevice (csrc/vol.hip) at plane stride S beside the grid kernels at
             W, which the volume's expectations are stated against; the inverse is the grid's followed by k_grid_vsum up the
             slabs, whose rate alone is what "unvol" takes longer than "ungrid"
  byte L,S / unbyte L,S   (with --bytes)
             glcByteDeltaDevice / glcUnbyteDeltaDevice (csrc/byte_delta.hip) at (lag, stride) = (1, 0), (3, 0), (1, 4096) and (3, 1281),
             beside the kernels they are stated against on the same byte count: lag 3 2 / unlag 3 2 and grid 1281 2 / ungrid 1281 2
             (the lag and grid kernels at elem 2, no fold)

Every variant runs once per round, rounds repeat (--reps, after --warmup rounds); each run is bracketed by device events.  The
table gives the median, the fastest and the slowest run of every variant, as GB/s of input bytes (the traffic is twice that)
and relative to the copy's median.  The buffer (--gib, default 1) is larger than the 256 MiB Infinity Cache on purpose.
--offset A B misaligns source and destination by A and B bytes.  One JSON line on stdout, the table on stderr or in --md FILE.

python tools/bench_shuffle.py [--gib 1] [--reps 30] [--warmup 3] [--offset 0 0] [--lag] [--grid W [--volume S]] [--bytes] [--md FILE]"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's and the library's are one and the same object)"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in os.path.basename(path):
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime is loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--offset", type=int, nargs=2, default=[0, 0])
    ap.add_argument("--lag", action="store_true", help="the lagged, folded delta kernels beside the others")
    ap.add_argument("--grid", type=int, default=0, metavar="W", help="the 2-D predictor's kernels at row width W beside the lag kernels at (1, 1)")
    ap.add_argument("--volume", type=int, default=0, metavar="S", help="with --grid W: the 3-D predictor's kernels at plane stride S beside the grid kernels")
    ap.add_argument("--bytes", action="store_true", help="the byte predictor's kernels beside the lag and grid kernels at elem 2")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 timed repetitions"
    import torch

    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    L = glc._ct()
    dev = torch.device("cuda:0")
    n = int(args.gib * (1 << 30))
    so, do = args.offset
    src_buf = torch.randint(0, 256, (n + 256,), dtype=torch.uint8, device=dev)
    dst_buf = torch.empty(n + 256, dtype=torch.uint8, device=dev)
    src, dst = src_buf[so:so + n], dst_buf[do:do + n]
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3                                                    # hipMemcpyDeviceToDevice

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n, D2D, None) == 0

    def kernel(fn, elem):
        return lambda: glc._chk("shuffle", fn(src.data_ptr(), dst.data_ptr(), n, elem, None))

    variants = [("copy", copy)]
    for elem in (2, 4, 8):
        variants.append(("shuffle %d" % elem, kernel(L.glcShuffleDevice, elem)))
        variants.append(("unshuf %d" % elem, kernel(L.glcUnshuffleDevice, elem)))
        variants.append(("delta-shuffle %d" % elem, kernel(L.glcDeltaShuffleDevice, elem)))
        variants.append(("undelta-unshuffle %d" % elem, kernel(L.glcUndeltaUnshuffleDevice, elem)))
    def lagged(fn, elem, lag, fold):
        return lambda: glc._chk("lag", fn(src.data_ptr(), dst.data_ptr(), n, elem, lag, fold, None))

    if args.lag:
        for elem in (2, 4, 8):
            for lag in (2, 3, 8, 16):
                for fold in (0, 1):
                    tag = "%d%s %d" % (lag, "f" if fold else "", elem)
                    variants.append(("lag " + tag, lagged(L.glcLagDeltaShuffleDevice, elem, lag, fold)))
                    variants.append(("unlag " + tag, lagged(L.glcUnlagDeltaUnshuffleDevice, elem, lag, fold)))
            back = torch.empty_like(src)                       # what is timed inverts itself, once per lag, with the fold
            for lag in (2, 3, 8, 16):
                lagged(L.glcLagDeltaShuffleDevice, elem, lag, 1)()
                glc._chk("unlag", L.glcUnlagDeltaUnshuffleDevice(dst.data_ptr(), back.data_ptr(), n, elem, lag, 1, None))
                assert torch.equal(back, src), (elem, lag)
            del back
    if args.grid:
        back = torch.empty_like(src)                           # what is timed inverts itself
        for elem in (2, 4, 8):
            variants.append(("lag 1f %d" % elem, lagged(L.glcLagDeltaShuffleDevice, elem, 1, 1)))
            variants.append(("unlag 1f %d" % elem, lagged(L.glcUnlagDeltaUnshuffleDevice, elem, 1, 1)))
            variants.append(("grid %df %d" % (args.grid, elem), lagged(L.glcGridDeltaShuffleDevice, elem, args.grid, 1)))
            variants.append(("ungrid %df %d" % (args.grid, elem), lagged(L.glcUngridDeltaUnshuffleDevice, elem, args.grid, 1)))
            lagged(L.glcGridDeltaShuffleDevice, elem, args.grid, 1)()
            glc._chk("ungrid", L.glcUngridDeltaUnshuffleDevice(dst.data_ptr(), back.data_ptr(), n, elem, args.grid, 1, None))
            assert torch.equal(back, src), (elem, args.grid)
            if args.volume:
                def vol(fn, elem=elem):
                    return lambda: glc._chk("vol", fn(src.data_ptr(), dst.data_ptr(), n, elem, args.grid, args.volume, 1, None))

                variants.append(("vol %d,%df %d" % (args.grid, args.volume, elem), vol(L.glcVolDeltaShuffleDevice)))
                variants.append(("unvol %d,%df %d" % (args.grid, args.volume, elem), vol(L.glcUnvolDeltaUnshuffleDevice)))
                vol(L.glcVolDeltaShuffleDevice)()
                glc._chk("unvol", L.glcUnvolDeltaUnshuffleDevice(dst.data_ptr(), back.data_ptr(), n, elem, args.grid, args.volume, 1, None))
                assert torch.equal(back, src), (elem, args.grid, args.volume)
        del back
    if args.bytes:
        def byted(fn, lag, stride):
            return lambda: glc._chk("byte", fn(src.data_ptr(), dst.data_ptr(), n, lag, stride, None))

        back = torch.empty_like(src)                           # what is timed inverts itself
        variants.append(("lag 3 2", lagged(L.glcLagDeltaShuffleDevice, 2, 3, 0)))
        variants.append(("unlag 3 2", lagged(L.glcUnlagDeltaUnshuffleDevice, 2, 3, 0)))
        variants.append(("grid 1281 2", lagged(L.glcGridDeltaShuffleDevice, 2, 1281, 0)))
        variants.append(("ungrid 1281 2", lagged(L.glcUngridDeltaUnshuffleDevice, 2, 1281, 0)))
        for lag, stride in ((1, 0), (3, 0), (1, 4096), (3, 1281)):
            variants.append(("byte %d,%d" % (lag, stride), byted(L.glcByteDeltaDevice, lag, stride)))
            variants.append(("unbyte %d,%d" % (lag, stride), byted(L.glcUnbyteDeltaDevice, lag, stride)))
            byted(L.glcByteDeltaDevice, lag, stride)()
            glc._chk("unbyte", L.glcUnbyteDeltaDevice(dst.data_ptr(), back.data_ptr(), n, lag, stride, None))
            assert torch.equal(back, src), (lag, stride)
        del back
    # correctness of what is timed, once, at this size and alignment
    for elem in (2, 4, 8):
        kernel(L.glcShuffleDevice, elem)()
        q = n // elem
        want = src[:q * elem].view(q, elem).t().contiguous().view(-1)
        assert torch.equal(dst[:q * elem], want) and torch.equal(dst[q * elem:], src[q * elem:]), elem
        back = torch.empty_like(src)
        glc._chk("unshuffle", L.glcUnshuffleDevice(dst.data_ptr(), back.data_ptr(), n, elem, None))
        assert torch.equal(back, src), elem
        # delta + shuffle: the differences within runs of 2048 elements, then the same planes
        x = src[:q * elem].clone().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[elem])     # (a copy: aligned for the view)
        d = x.clone()
        d[1:] -= x[:-1]
        d[::2048] = x[::2048]
        want = d.view(torch.uint8).view(q, elem).t().contiguous().view(-1)
        kernel(L.glcDeltaShuffleDevice, elem)()
        assert torch.equal(dst[:q * elem], want) and torch.equal(dst[q * elem:], src[q * elem:]), elem
        glc._chk("undelta", L.glcUndeltaUnshuffleDevice(dst.data_ptr(), back.data_ptr(), n, elem, None))
        assert torch.equal(back, src), elem
        del back, want, d, x
    times = {name: [] for name, _ in variants}
    events = []
    for r in range(args.warmup + args.reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if r >= args.warmup:
                events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1) * 1e-3)
    base = statistics.median(times["copy"])
    res = {"bytes": n, "reps": args.reps, "offset": [so, do], "variants": {}}
    rows = ["| variant | median GB/s | fastest | slowest | time / copy |", "|---|---|---|---|---|"]
    for name, _ in variants:
        t = sorted(times[name])
        med = statistics.median(t)
        res["variants"][name] = {"median_ms": med * 1e3, "min_ms": t[0] * 1e3, "max_ms": t[-1] * 1e3,
                                 "median_GBps": n / med / 1e9, "vs_copy": med / base}
        rows.append("| %s | %.0f | %.0f | %.0f | %.2f |" % (name, n / med / 1e9, n / t[0] / 1e9, n / t[-1] / 1e9, med / base))
    table = "\n".join(rows) + "\n"
    if args.md:
        with open(args.md, "w") as f:
            f.write(table)
    else:
        sys.stderr.write(table)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
