"""The container's two codecs, and the batched order-0 kernels against the single-stream ones, in one process (one JSON line
on stdout, also written to profiles/container_codec.json with --write):

  kernels    histogram -> table -> encode and decode of ONE stream of --gib GiB (glcHdHistogramDevice, glcHdBuildTableDevice,
             glcHdEncodeDevice, glcHdDecodeDeviceTableOnDevice) against the batched calls on the same bytes as 1 MiB segments
             (glcHdSegmentsTablesDevice / EncodeDevice / DecodeDevice; the decoder in chunks of --chunk segments): GB/s of
             input, and the ratio batched / single
  container  glcContainerCompressDevice / DecompressDevice with codec BWT and HUFF0 alternating on one plan and input: bytes,
             ratio (input / container bytes), GB/s, and the plan's per-kernel profile of one more HUFF0 round trip

--data: zipf (configs[1], the default), float32, quant16 (tools/bench_container.py's generators), text (tests/datagen.py's
text, --text-mib of it tiled); --shuffle ELEM sets the filter for the container section.  Every shape is warmed, timed
repetitions alternate the variants, and the device is synchronised inside every bracket.

The per-kernel table of a profiler comes from a run of its own, which slows the host and so is never the timed run:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_codec.py --gib 1 --iters 1 --sections container --write ''

python tools/bench_codec.py [--gib 4] [--rows 2048] [--iters 3] [--data KIND] [--shuffle ELEM] [--sections kernels,container]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MiB = 1 << 20


def make_input(torch, glc, L, dev, kind, total, text_mib):
    if kind == "zipf":
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        import datagen
        import numpy as np
        thr = torch.from_numpy(datagen.zipf_thresholds().view(np.int32)).to(dev)
        assert L.glcGenZipfPhilox(out.data_ptr(), total, 0, 0x5EED0002, thr.data_ptr(), None) == 1
        return out
    if kind == "text":
        import datagen
        import numpy as np
        t = torch.from_numpy(np.array(datagen.text_bytes_fast(text_mib * MiB, seed=1))).to(dev)
        return t.repeat((total + t.numel() - 1) // t.numel())[:total].contiguous()
    import bench_container
    return bench_container.typed_on_device(torch, L, dev, kind, total)[:total].contiguous()


def timed(torch, fns, iters):
    """seconds of each function, best of `iters`, the functions alternating"""
    best = [float("inf")] * len(fns)
    for _ in range(iters):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best[i] = min(best[i], time.perf_counter() - t0)
    return best


def kernels_section(torch, glc, L, d_in, iters, chunk):
    dev, total = d_in.device, d_in.numel()
    res = {}
    # single stream
    d_hist = torch.empty(256, dtype=torch.int64, device=dev)
    lens = torch.empty(256, dtype=torch.uint8, device=dev)
    codes = torch.empty(256, dtype=torch.int16, device=dev)
    tab = torch.empty(4096, dtype=torch.uint8, device=dev)
    cap = int(L.glcHdEncodeBound(total))
    glc.hd_histogram_device(d_in, d_hist=d_hist)
    L.glcHdBuildTableDevice(d_hist.data_ptr(), lens.data_ptr(), codes.data_ptr(), tab.data_ptr(), None)
    bits = int((d_hist * lens.to(torch.int64)).sum())
    cap = (bits + 31) // 32 + 1
    units = torch.empty(cap, dtype=torch.int32, device=dev)
    nun = torch.zeros(1, dtype=torch.int64, device=dev)
    ework = torch.empty(int(L.glcHdEncodeWorkBytes(total)), dtype=torch.uint8, device=dev)
    dwork = torch.empty(int(L.glcHdWorkBytes(cap)), dtype=torch.uint8, device=dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)

    def enc1():
        assert L.glcHdHistogramDevice(d_in.data_ptr(), total, d_hist.data_ptr(), None)
        assert L.glcHdBuildTableDevice(d_hist.data_ptr(), lens.data_ptr(), codes.data_ptr(), tab.data_ptr(), None)
        assert L.glcHdEncodeDevice(d_in.data_ptr(), total, lens.data_ptr(), codes.data_ptr(), units.data_ptr(), cap, nun.data_ptr(),
                                   ework.data_ptr(), None)

    def dec1():
        assert L.glcHdDecodeDeviceTableOnDevice(units.data_ptr(), cap, tab.data_ptr(), out.data_ptr(), total, dwork.data_ptr(), None)

    # batched: the same bytes as 1 MiB segments
    count = total // MiB
    d_off = torch.arange(count, dtype=torch.int64, device=dev) * MiB
    d_len = torch.full((count,), MiB, dtype=torch.int64, device=dev)
    bh = torch.empty((count, 256), dtype=torch.int32, device=dev)
    bl = torch.empty((count, 256), dtype=torch.uint8, device=dev)
    bc = torch.empty((count, 256), dtype=torch.int16, device=dev)
    bn = torch.empty(count, dtype=torch.int64, device=dev)
    assert L.glcHdSegmentsTablesDevice(d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), count, MiB, bh.data_ptr(), bl.data_ptr(),
                                       bc.data_ptr(), bn.data_ptr(), None)
    uoff = torch.cumsum(bn, 0) - bn
    bcap = int(bn.sum())
    bunits = torch.empty(bcap, dtype=torch.int32, device=dev)
    chunk = min(chunk, count)
    bwork = torch.empty(int(L.glcHdSegmentsWorkBytes(chunk, MiB)), dtype=torch.uint8, device=dev)
    ewk = torch.empty(int(L.glcHdSegmentsWorkBytes(count, MiB)), dtype=torch.uint8, device=dev)
    bout = torch.empty(total, dtype=torch.uint8, device=dev)

    def encb():
        assert L.glcHdSegmentsTablesDevice(d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), count, MiB, bh.data_ptr(),
                                           bl.data_ptr(), bc.data_ptr(), bn.data_ptr(), None)
        assert L.glcHdSegmentsEncodeDevice(d_in.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), count, MiB, bl.data_ptr(), bc.data_ptr(),
                                           bn.data_ptr(), bunits.data_ptr(), uoff.data_ptr(), bcap, None, ewk.data_ptr(), None)

    def decb():
        for a in range(0, count, chunk):
            m = min(chunk, count - a)
            assert L.glcHdSegmentsDecodeDevice(bunits.data_ptr(), uoff[a:].data_ptr(), bn[a:].data_ptr(), bh[a:].data_ptr(),
                                               bout.data_ptr(), d_off[a:].data_ptr(), d_len[a:].data_ptr(), m, MiB, None,
                                               bwork.data_ptr(), None)

    for fn in (enc1, dec1, encb, decb):
        fn()
    torch.cuda.synchronize()
    assert int(nun) == cap and torch.equal(out, d_in) and torch.equal(bout, d_in)
    te1, teb = timed(torch, [enc1, encb], iters)
    td1, tdb = timed(torch, [dec1, decb], iters)
    gb = total / 1e9
    res.update(single_encode_gbs=gb / te1, batched_encode_gbs=gb / teb, encode_ratio=te1 / teb,
               single_decode_gbs=gb / td1, batched_decode_gbs=gb / tdb, decode_ratio=td1 / tdb,
               single_units=cap, batched_units=bcap, segments=count, decode_chunk=chunk)
    return res


def container_section(torch, glc, plan, d_in, iters, elem):
    total, n = d_in.numel(), plan.n
    cap = glc.container_bound(total, n)
    dev = d_in.device
    conts = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    glc.container_set_shuffle(plan, elem)
    size = [0, 0]

    def enc(codec):
        def f():
            glc.container_set_codec(plan, codec)
            glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, conts[codec].data_ptr(), cap, d_len.data_ptr()))
            size[codec] = int(d_len.item())
        return f

    def dec(codec):
        def f():
            glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, conts[codec].data_ptr(), size[codec], out.data_ptr(), total, d_len.data_ptr()))
        return f

    for codec in (0, 1):
        enc(codec)()
        dec(codec)()
        torch.cuda.synchronize()
        assert torch.equal(out, d_in), codec
    te = timed(torch, [enc(0), enc(1)], iters)
    td = timed(torch, [dec(0), dec(1)], iters)
    plan.enable_timing(3)
    enc(1)()
    dec(1)()
    plan.synchronize()
    prof = {k: dict(ms=round(v["ms"], 3), launches=v["launches"]) for k, v in plan.kernel_profiles().items()}
    plan.enable_timing(0)
    gb = total / 1e9
    return dict(bytes_bwt=size[0], bytes_huff0=size[1], ratio_bwt=total / size[0], ratio_huff0=total / size[1],
                encode_gbs_bwt=gb / te[0], encode_gbs_huff0=gb / te[1], decode_gbs_bwt=gb / td[0], decode_gbs_huff0=gb / td[1],
                huff0_kernel_profile=prof)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--pipelining", type=int, default=1)
    ap.add_argument("--data", default="zipf", choices=["zipf", "float32", "quant16", "text"])
    ap.add_argument("--shuffle", type=int, default=0)
    ap.add_argument("--text-mib", type=int, default=8)
    ap.add_argument("--sections", default="kernels,container")
    ap.add_argument("--write", default=os.path.join(ROOT, "profiles", "container_codec.json"), help="the JSON line is appended here ('' = nowhere)")
    a = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.join(ROOT, "gpu-lossless-compression_amd"))
    import glc_binding as glc
    L = glc.lib()
    dev = torch.device("cuda:0")
    total = int(a.gib * 1024) * MiB
    d_in = make_input(torch, glc, L, dev, a.data, total, a.text_mib)
    res = dict(tool="bench_codec", data=a.data, shuffle=a.shuffle, gib=a.gib, rows=a.rows, iters=a.iters, pipelining=a.pipelining)
    sections = a.sections.split(",")
    if "kernels" in sections:
        res["kernels"] = kernels_section(torch, glc, L, d_in, a.iters, a.chunk)
    if "container" in sections:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, MiB, rows=a.rows) as plan:
            plan.set_pipelining(bool(a.pipelining))
            res["container"] = container_section(torch, glc, plan, d_in, a.iters, a.shuffle)
    line = json.dumps(res)
    print(line)
    if a.write:
        with open(a.write, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
