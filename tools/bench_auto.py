"""The probe of the auto mode alone (csrc/auto.hip, glcProbeSegments) against the two passes it replaces and against a
device-to-device copy of the same bytes: --gib GiB as segments of 1 MiB of zeros, of scattered skew (90 % zeros, the rest uniform in
1 .. 15) and of noise; --rounds interleaved rounds after one warm-up, each call timed with device events; medians and spreads
(max - min) in one JSON line per input.  The calls:

  probe    glcProbeSegments: two memsets of the rows and k_au_probe
  tables   glcHdSegmentsTablesDevice: a memset, k_hdb_hist and k_hdb_table (what the sparse and rANS modes start a frame with)
  split    glcSparseSplitSegments with fill 0: k_sp_mask, k_sp_count and the compaction (nothing to move for zeros, everything for noise)
  copy     a device-to-device copy

k_hdb_hist and k_sp_mask have no call of their own; their own durations come from running this tool under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_auto.py), where every launch of the three kernels is listed.

python tools/bench_auto.py [--gib 1] [--rounds 5]"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    dev = torch.device("cuda:0")
    count = int(args.gib * 1024)
    total = count * MiB
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0010)
    off = torch.arange(count, dtype=torch.int64, device=dev) * MiB
    ln = torch.full((count,), MiB, dtype=torch.int64, device=dev)
    hist = torch.empty((count, 256), dtype=torch.int32, device=dev)
    uniform = torch.empty((count, 256), dtype=torch.int32, device=dev)
    hist2 = torch.empty((count, 256), dtype=torch.int32, device=dev)
    lens = torch.empty((count, 256), dtype=torch.uint8, device=dev)
    codes = torch.empty((count, 256), dtype=torch.int16, device=dev)
    nun = torch.empty(count, dtype=torch.int64, device=dev)
    fill = torch.zeros(count, dtype=torch.int32, device=dev)
    mask = torch.empty((count, MiB // 64 // 32), dtype=torch.int32, device=dev)
    klen = torch.empty(count, dtype=torch.int64, device=dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    L = glc._ct()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for name in ("zeros", "skew90", "noise"):
        if name == "zeros":
            d_in = torch.zeros(total, dtype=torch.uint8, device=dev)
        elif name == "skew90":
            d_in = torch.randint(1, 16, (total,), dtype=torch.uint8, device=dev, generator=g)
            d_in.mul_(torch.rand(total, dtype=torch.float32, device=dev, generator=g) >= 0.9)
        else:
            d_in = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)

        def probe():
            glc._chk("glcProbeSegments", L.glcProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), count, MiB, hist.data_ptr(),
                                                             uniform.data_ptr(), None))

        def tables():
            assert L.glcHdSegmentsTablesDevice(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), count, MiB, hist2.data_ptr(), lens.data_ptr(),
                                               codes.data_ptr(), nun.data_ptr(), None) == 1

        def split():
            glc._chk("glcSparseSplitSegments", L.glcSparseSplitSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), count, MiB,
                                                                         fill.data_ptr(), mask.data_ptr(), out.data_ptr(), klen.data_ptr(), None))

        def copy():
            out.copy_(d_in)

        res = {k: [] for k in ("probe_GBps", "tables_GBps", "split_GBps", "copy_GBps")}
        for r in range(args.rounds + 1):                        # round 0 is the warm-up
            for k, fn in (("probe_GBps", probe), ("tables_GBps", tables), ("split_GBps", split), ("copy_GBps", copy)):
                t = timed(fn)
                if r:
                    res[k].append(round(total / t / 1e9, 2))
        assert torch.equal(hist, hist2) and int(hist.sum(dtype=torch.int64).item()) == total
        assert int(uniform[:, 0].sum(dtype=torch.int64).item()) == (total - int(klen.sum().item())) // 64    # E against the mask pass
        rep = {"workload": "%d x 1 MiB segments of %s" % (count, name), "uniform_chunks": int(uniform.sum(dtype=torch.int64).item())}
        for k, v in res.items():
            s = sorted(v)
            rep[k], rep[k + "_median"], rep[k + "_spread"] = v, s[len(s) // 2], round(s[-1] - s[0], 2)
        print(json.dumps(rep))
        del d_in


if __name__ == "__main__":
    sys.exit(main())
