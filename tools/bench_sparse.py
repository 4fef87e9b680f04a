"""The two passes of the container's sparse mode alone against a device-to-device copy of the same bytes, in one process and
interleaved:

  copy        hipMemcpyAsync, device to device, of the buffer: one read and one write per byte, the yardstick
  split D     glcSparseSplitSegments (mask pass, count, compaction) over the buffer as segments of 1 MiB, D percent of whose 64-byte
              chunks hold noise and the others the fill byte
  join D      glcSparseJoinSegments of what the split made

Every variant runs once per round, rounds repeat (--reps, after --warmup rounds); each run is bracketed by device events.  The
table gives the median, the fastest and the slowest run of every variant as GB/s of the segments' bytes (a split reads them once
and writes the kept part, a join writes them once and reads the kept part) and relative to the copy's median.  The buffer (--gib,
default 1) is larger than the 256 MiB Infinity Cache on purpose.  One JSON line on stdout, the table on stderr or in --md FILE.

python tools/bench_sparse.py [--gib 1] [--reps 30] [--warmup 3] [--density 0 25 100] [--md FILE]"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 1 << 20


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
    ap.add_argument("--density", type=int, nargs="+", default=[0, 25, 100], help="percent of the chunks that are kept")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 timed repetitions"
    import torch

    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    L = glc._ct()
    dev = torch.device("cuda:0")
    count = int(args.gib * 1024)
    n = count * SEG
    mw = glc.sparse_mask_words(SEG)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0020)
    off = torch.arange(count, dtype=torch.int64, device=dev) * SEG
    ln = torch.full((count,), SEG, dtype=torch.int64, device=dev)
    fill = torch.full((count,), 0x10, dtype=torch.int32, device=dev)
    kept = torch.empty(n, dtype=torch.uint8, device=dev)
    back = torch.empty(n, dtype=torch.uint8, device=dev)
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3                                                    # hipMemcpyDeviceToDevice
    inputs, masks, klens = {}, {}, {}
    for d in args.density:
        noise = torch.randint(0, 256, (n // 64, 64), dtype=torch.uint8, device=dev, generator=g)
        noise[:, 0] = 0x11                                     # (a kept chunk is never all fill)
        keep = torch.rand(n // 64, device=dev, generator=g) < d / 100.0
        x = torch.where(keep[:, None], noise, torch.full_like(noise, 0x10)).reshape(-1)
        inputs[d] = x
        masks[d] = torch.zeros((count, mw), dtype=torch.int32, device=dev)
        klens[d] = torch.zeros(count, dtype=torch.int64, device=dev)
        del noise

    def split(d):
        return lambda: glc._chk("split", L.glcSparseSplitSegments(inputs[d].data_ptr(), off.data_ptr(), ln.data_ptr(), count, SEG, fill.data_ptr(),
                                                                  masks[d].data_ptr(), kept.data_ptr(), klens[d].data_ptr(), None))

    def join(d):
        # (the kept bytes of density d are whatever the last split d left: the join's traffic does not depend on their values,
        # and its correctness is checked below right behind its own split)
        return lambda: glc._chk("join", L.glcSparseJoinSegments(kept.data_ptr(), off.data_ptr(), ln.data_ptr(), count, SEG, fill.data_ptr(),
                                                                masks[d].data_ptr(), back.data_ptr(), None))

    variants = [("copy", lambda: hip.hipMemcpyAsync(back.data_ptr(), inputs[args.density[0]].data_ptr(), n, D2D, None))]
    for d in args.density:                                     # correctness of what is timed, once, at this size
        split(d)()
        join(d)()
        torch.cuda.synchronize()
        assert torch.equal(back, inputs[d]), d
        bits = (inputs[d].view(-1, 64) != 0x10).any(dim=1)
        assert int(klens[d].sum().item()) == 64 * int(bits.sum().item()), d
        variants += [("split %d" % d, split(d)), ("join %d" % d, join(d))]
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
    res = {"bytes": n, "segment_bytes": SEG, "reps": args.reps, "variants": {}}
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
