"""The rANS kernels alone (csrc/ans.hip) against a device-to-device copy of the same bytes: glcAnsEncodeSegments and
glcAnsDecodeSegments over --gib GiB of scattered-skew bytes (90 % zeros, the rest uniform in 1 .. 15) as segments of 1 MiB,
--rounds interleaved rounds after one warm-up, each timed with device events; medians and spreads (max - min) in one JSON line.
The encode call includes the batched histogram, the table kernel and the placing of the records; the decode call the table kernel.

python tools/bench_ans.py [--gib 1] [--rounds 5]"""
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
    d_in = torch.randint(1, 16, (total,), dtype=torch.uint8, device=dev, generator=g)
    d_in.mul_(torch.rand(total, dtype=torch.float32, device=dev, generator=g) >= 0.9)
    out = torch.empty_like(d_in)
    off = torch.arange(count, dtype=torch.int64, device=dev) * MiB
    ln = torch.full((count,), MiB, dtype=torch.int64, device=dev)
    bound = glc.ans_bound_words(MiB)
    rec_off = torch.arange(count, dtype=torch.int64, device=dev) * bound
    rec = torch.empty(count * bound, dtype=torch.int32, device=dev)
    words = torch.zeros(count, dtype=torch.int64, device=dev)
    hist = torch.zeros((count, 256), dtype=torch.int32, device=dev)
    work = torch.empty(glc.ans_work_bytes(count, MiB), dtype=torch.uint8, device=dev)
    L = glc._ct()

    def encode():
        glc._chk("glcAnsEncodeSegments", L.glcAnsEncodeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), count, MiB, hist.data_ptr(),
                                                                 rec.data_ptr(), rec_off.data_ptr(), words.data_ptr(), work.data_ptr(),
                                                                 work.numel(), None))

    def decode():
        glc._chk("glcAnsDecodeSegments", L.glcAnsDecodeSegments(rec.data_ptr(), rec_off.data_ptr(), words.data_ptr(), hist.data_ptr(),
                                                                 off.data_ptr(), ln.data_ptr(), count, MiB, out.data_ptr(), work.data_ptr(),
                                                                 work.numel(), None))

    def copy():
        out.copy_(d_in)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    res = {k: [] for k in ("encode_GBps", "decode_GBps", "copy_GBps")}
    for r in range(args.rounds + 1):                            # round 0 is the warm-up
        for k, fn in (("encode_GBps", encode), ("decode_GBps", decode), ("copy_GBps", copy)):
            t = timed(fn)
            if k == "decode_GBps":
                assert torch.equal(out, d_in)
            if r:
                res[k].append(round(total / t / 1e9, 2))
    rep = {"workload": "%d x 1 MiB segments of scattered skew (90 %% zeros)" % count,
           "record_bytes": 4 * int(words.sum().item()), "ratio": total / (4 * int(words.sum().item())),
           "work_bytes": work.numel()}
    for k, v in res.items():
        s = sorted(v)
        rep[k], rep[k + "_median"], rep[k + "_spread"] = v, s[len(s) // 2], round(s[-1] - s[0], 2)
    print(json.dumps(rep))


if __name__ == "__main__":
    sys.exit(main())
