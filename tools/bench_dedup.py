"""The two passes of the dedup mode alone on one GPU (glcDedupMapSegments, glcDedupFillSegments; the mode itself is measured by
tools/bench_container.py --dedup and tools/bench_range.py --dedup): --gib GiB in segments of 1 MiB, frames of --rows segments,
--rounds interleaved rounds after one warm-up, every call timed with device events; medians and spreads (max - min), one JSON line.

  map    over random bytes (no two chunks alike), over `pages` of tests/dedup_inputs.py (about half the pages repeat) and over zeros
         (one slot takes every chunk: what the skip-insert is for)
  fill   with the map of the last frame of `pages`, the frame 16-byte aligned and one byte off (the stores of a lane are 16 bytes
         wide only at an aligned destination); GB/s count the frame's bytes, of which the elided chunks are moved
  copy   a device-to-device copy of the same bytes

python tools/bench_dedup.py [--gib 1] [--rows 512] [--rounds 5]"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    dev = torch.device("cuda:0")
    count = int(args.gib * 1024)
    total = count * MiB
    rows = min(args.rows, count)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0D0D)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    def summary(times):
        r = [total / t / 1e9 for t in times]
        return {"gbps": round(statistics.median(r), 1), "spread": round(max(r) - min(r), 1)}

    L = glc._ct()
    back = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    # the passes alone, frame by frame
    frames = count // rows
    off = torch.arange(rows, dtype=torch.int64, device=dev) * MiB
    ln = torch.full((rows,), MiB, dtype=torch.int64, device=dev)
    nch = MiB // 512
    src = torch.empty(rows * nch, dtype=torch.int32, device=dev)
    wb = int(L.glcDedupWorkBytes(rows, MiB))
    work = torch.empty(wb, dtype=torch.uint8, device=dev)

    def map_all(x):
        for f in range(frames):
            glc._chk("map", L.glcDedupMapSegments(x[f * rows * MiB:].data_ptr(), off.data_ptr(), ln.data_ptr(), rows, MiB, src.data_ptr(),
                                                   work.data_ptr(), wb, None))

    res = {"section": "passes", "gib": args.gib, "rows": rows}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import dedup_inputs
    paged = torch.empty(total + 16, dtype=torch.uint8, device=dev)     # the same bytes at an aligned address and one byte off
    host = torch.from_numpy(np.array(dedup_inputs.make("pages", total), copy=True))
    paged[:total] = host.to(dev)
    odd = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    odd[1:total + 1] = paged[:total]
    inputs = {"distinct": torch.randint(0, 256, (total,), generator=g, device=dev, dtype=torch.uint8), "pages": paged[:total],
              "zeros": torch.zeros(total, dtype=torch.uint8, device=dev)}
    times = {k: [] for k in list(inputs) + ["fill", "fill_unaligned", "copy"]}
    map_all(inputs["pages"])
    for _ in range(args.rounds):
        for k in ("distinct", "zeros", "pages"):                # (pages last: its map of the last frame feeds the fill)
            times[k].append(timed(lambda: map_all(inputs[k])))
        x = inputs["pages"]
        times["fill"].append(timed(lambda: [glc._chk("fill", L.glcDedupFillSegments(x[(frames - 1) * rows * MiB:].data_ptr(), off.data_ptr(),
                                                                                     ln.data_ptr(), rows, MiB, src.data_ptr(), None)) for _ in range(frames)]))
        y = odd[1:total + 1]
        times["fill_unaligned"].append(timed(lambda: [glc._chk("fill", L.glcDedupFillSegments(y[(frames - 1) * rows * MiB:].data_ptr(), off.data_ptr(),
                                                                                               ln.data_ptr(), rows, MiB, src.data_ptr(), None)) for _ in range(frames)]))
        times["copy"].append(timed(lambda: back[:total].copy_(x)))
    res.update({k: summary(v) for k, v in times.items()})
    res["elided_last_frame"] = int((src != torch.arange(rows * nch, dtype=torch.int32, device=dev)).sum().item())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
