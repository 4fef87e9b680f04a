"""The BWT container against the codec it wraps, in one process and run (one JSON line on stdout):

  crc        glcCrc32Segments over one device buffer of --gib GiB, against glcProbeStreamRead on the same buffer
  encode     glcContainerCompressDevice of configs[1] (Philox Zipf(1.0) bytes, 1 MiB blocks, --rows-row plan, as bench.py
             generates it), against glcCompressBatchCompact batches chained into one array on the same plan
  decode     glcContainerDecompressDevice of that container, against glcDecompressBatchCompact of the compact array
  size       container bytes against the sum of the compact sizes
  filter     with --shuffle ELEM: glcContainerCompressDevice / glcContainerDecompressDevice with the byte-plane shuffle filter
             off and on (glcPlanSetContainerShuffle), alternating, on the same plan and input: ratio (input bytes / container
             bytes) and GB/s for both settings, the plan's per-kernel profile and the sorter tiers its last frame went through

--data picks the input: zipf (the default, configs[1]), or typed arrays generated on the device -- float32 (configs[3]: Philox
N(0,1), as bench.py generates it), smooth32 / smooth64 (a sine plus a random walk) and quant16 (uint16 Laplace codes around
512).  The comparison with the compact array needs input that shrinks: it runs for zipf only.

Integer series, also generated on the device, after tests/series_datagen.py: ts64 (int64 timestamps, steps uniform in [900, 1100)),
ids32 (sorted uint32 ids below 2^31), ctr32 (uint32 counters, Poisson(3) increments) and adc16 (12-bit sine plus N(0, 3) noise in
uint16).  --delta switches the filter's delta mode on for the filtered setting (glcPlanSetContainerDelta, format version 4), --codec 1
the order-0 codec for both settings.

--rounds R (typed data, --codec 1) replaces the filter section by the sparse section: the filter on (with --delta: in delta mode), the
order-0 codec, and R interleaved rounds of encode and decode timed with device events -- with --sparse each round runs the sparse
mode off and then on (glcPlanSetContainerSparse, format version 5), without it only off, which is also what a build without the
mode can run; with --ans each round also runs the rANS mode (glcPlanSetContainerAns, format version 7), so that one run interleaves
the settings off, sparse and ans; with --auto each round also runs the auto mode (glcPlanSetContainerAuto, format version 8),
interleaved with the others.  --data skew90 is the scattered-skew input (90 % zeros, the rest uniform in 1 .. 15, no filter).
Every round's rates are reported, with their median and spread (max - min) per setting.  With --dedup each round also runs the dedup
mode (glcPlanSetContainerDedup, format version 9), interleaved with the others; --data pages / pages_noise are the inputs of
tests/dedup_inputs.py (4 KiB pages of which about half repeat, compressible or not), made on the host by the generator the Python
model reads, so that container_bytes can be held against tests/dedup_model.py's size(); with --dedup, --data zipf (data without a
duplicate) runs through this section too.

--runs (with --data textlike or loglike, generated on the device; --rounds R, at least 1) is the runs section: the BWT codec with its
runs mode off and then on (glcPlanSetContainerRuns, format version 6), R interleaved rounds of encode and decode timed with device
events, their medians and spreads, the ratio of both settings, the plan's per-kernel profile of one encode and one decode per
setting, and the split and the join alone (glcZeroRunSplitSegments / glcZeroRunJoinSegments over the input's blocks) against a
device-to-device copy.  --runs-off-only runs the same section without ever touching the mode, which is also what a build without
it can run.

--codec 4 (with --data textlike, zipf or mix -- text-like and Zipf bytes half and half in runs of 64 blocks --; --rounds R, at least
1) is the choose section: the BWT codec, the order-0 codec and the CHOOSE codec on the same bytes in R interleaved rounds timed with
device events, ratio / encode / decode per codec and what glcContainerLastChoice reports, then the bigram probe alone against the
auto mode's probe and a device-to-device copy.

--filter-auto (any --data but zipf's compact comparison; --rounds R, at least 1) is the filter-auto section: the order-0 codec with
the auto mode on under no filter, under the filter named by --shuffle / --delta (default: the data's element size) and under
filter-auto (glcPlanSetContainerFilterAuto, format version 10), R interleaved rounds of encode and decode timed with device events,
ratio, the CRC-32 of the container and what glcContainerLastFilters reports per setting.  --filter-auto-off-only runs the first two
settings alone, which is also what a build without the setting can run.

--lag L [--fold] (with --data stereo16, adc16x8, xyz32, cplx64 or i32x4 of tests/lag_inputs.py -- 32 MiB generated on the host and
repeated to the size asked for --, or any typed kind; --rounds R, at least 1) is the lag section: the order-0 codec with the auto
mode on under the shuffle alone, the plain delta (both format version 8) and the delta with lag L and the fold (format version
11), interleaved, with the same output as the filter-auto section; --lag 1 without --fold runs the first two only.

--grid W [--fold] (with --data img16, field32 or walk32 of tests/grid_inputs.py at row width W -- about 32 MiB of whole rows
generated on the host and repeated --, or any typed kind; --rounds R, at least 1) is the grid section: the lag section's settings at
lag 1 -- the shuffle alone, the plain delta, with --fold the folded delta (format version 11) -- and the 2-D predictor of row width
W (glcPlanSetContainerDeltaGrid, format version 12), interleaved, with the same output.  --volume S (with --grid W, and --data
vol32, vol64, volr32, vol16 or vol16n -- smooth32, smooth64, round32, ct16 and ct16n of tests/vol_inputs.py at row width W and
plane stride S, about 32 MiB of whole planes generated on the host and repeated --, or any typed kind) adds the 3-D predictor of
plane stride S over it (glcPlanSetContainerDeltaVolume, format version 17) to the grid section's settings.

--filter-grid (with --grid W [--fold] and the data of the grid section; --rounds R, at least 1) is the filter-grid section: the
order-0 container under filter-lag, under filter-grid (format version 14) and with elem, W and the fold set by hand (version 12).
--filter-lag (with --lag L [--fold] and the data of the lag section; --rounds R, at least 1) is the filter-lag section: the order-0
codec with the auto mode on under filter-auto (format version 10), under filter-auto with lag (glcPlanSetContainerFilterLag, format
version 13: the lag probe per frame, the lag picked per frame) and under the plan set by hand to the data's element size, lag L and
the fold (format version 11), interleaved, with the filter-auto section's output and what glcContainerLastLagFilters reports.

--filter-byte (with --byte-delta LAG,STRIDE and --data grey8 or rgb8; --rounds R, at least 1) is the filter-byte section: the order-0
container under filter-grid (format version 14), under filter-byte (format version 16) and with LAG and STRIDE set by hand (version 15).
--byte-delta LAG,STRIDE (with --data grey8 or rgb8 of tests/byte_delta_inputs.py -- about 32 MiB of whole rows of STRIDE bytes
generated on the host and repeated; STRIDE 0: rows of 721 pixels --, or any other kind; --rounds R, at least 1) is the byte section:
the order-0 codec with the auto mode on and no filter (format version 8) and with the byte predictor at (LAG, STRIDE)
(glcPlanSetContainerByteDelta, format version 15), interleaved, with the same output as the lag section; LAG 0 runs the first only,
which is also what a build without the setting can run.
--choose-filters LEVEL [--block-kib K] (its own input: runs of 16 blocks of text-like bytes, float32 values, int64 timestamps, noise
and an 8-bit greyscale image in turn; --rounds R, at least 1) is the choose-filters section: the BWT codec, the CHOOSE codec alone, the
order-0 codec at the settings of every level up to LEVEL and the CHOOSE codec at every level up to it
(glcPlanSetContainerChooseFilters), interleaved, with the filter-auto section's output.  --bigram-kernels times the bigram probe's
one-pass kernel (segments of up to 64 KiB) against its two-pass kernel on the same blocks of 16 and 64 KiB.
python tools/bench_container.py [--gib 4] [--rows 2048] [--iters 2] [--pipelining 1|0] [--data KIND] [--shuffle ELEM] [--delta] [--codec 0|1|4]
                                [--rounds R] [--sparse] [--ans] [--auto] [--dedup] [--runs | --runs-off-only]
                                [--filter-auto | --filter-auto-off-only] [--lag L [--fold] [--filter-lag] | --grid W [--fold] [--volume S] [--filter-grid] |
                                 --byte-delta LAG,STRIDE [--filter-byte]]"""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
MiB = 1 << 20
DATA_ELEM = {"mix": 0, "textlike": 0, "loglike": 0, "zipf": 0, "float32": 4, "smooth32": 4, "smooth64": 8, "quant16": 2, "ts64": 8, "ids32": 4, "ctr32": 4, "adc16": 2, "skew90": 0, "pages": 0, "pages_noise": 0,
             "stereo16": 2, "adc16x8": 2, "xyz32": 4, "cplx64": 4, "i32x4": 4, "img16": 2, "field32": 4, "walk32": 4, "grey8": 0, "rgb8": 0,
             "vol32": 4, "vol64": 8, "volr32": 4, "vol16": 2, "vol16n": 2}
VOL_KINDS = {"vol32": "smooth32", "vol64": "smooth64", "volr32": "round32", "vol16": "ct16", "vol16n": "ct16n"}      # tests/vol_inputs.py's
LAG_PIECE = 32 * MiB                                           # what tests/lag_inputs.py generates on the host; repeated on the device


def typed_on_device(torch, L, dev, kind, total):
    """`total` bytes of typed data, generated on the device (seeded); the kinds of tests/typed_datagen.py at benchmark sizes"""
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0010)
    if kind == "float32":
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        assert L.glcGenFloatPhilox(out.data_ptr(), total, 0, 0x5EED0004, None) == 1
        return out
    if kind in ("smooth32", "smooth64"):
        elem = DATA_ELEM[kind]
        count = total // elem
        x = torch.randn(count, dtype=torch.float64, device=dev, generator=g).mul_(0.01).cumsum_(0)
        x.add_(torch.arange(count, dtype=torch.float64, device=dev).mul_(2.0 * 3.141592653589793 / 5000.0).sin_().mul_(100.0))
        return (x if elem == 8 else x.to(torch.float32)).view(torch.uint8)
    if kind == "skew90":                                       # scattered skew: 90 % zeros, the rest uniform in 1 .. 15
        v = torch.randint(1, 16, (total,), dtype=torch.uint8, device=dev, generator=g)
        return v.mul_(torch.rand(total, dtype=torch.float32, device=dev, generator=g) >= 0.9)
    if kind == "ts64":
        return torch.randint(900, 1100, (total // 8,), dtype=torch.int64, device=dev, generator=g).cumsum_(0).view(torch.uint8)
    if kind == "ids32":
        return torch.randint(0, 2 ** 31, (total // 4,), dtype=torch.int64, device=dev, generator=g).sort().values.to(torch.int32).view(torch.uint8)
    if kind == "ctr32":
        inc = torch.poisson(torch.full((total // 4,), 3.0, dtype=torch.float32, device=dev), generator=g).to(torch.int64)
        return inc.cumsum_(0).to(torch.int32).view(torch.uint8)
    if kind == "adc16":
        t = torch.arange(total // 2, dtype=torch.float64, device=dev).mul_(2.0 * 3.141592653589793 / 700.0).sin_().mul_(1500.0).add_(2048.0)
        t.add_(torch.randn(total // 2, dtype=torch.float64, device=dev, generator=g).mul_(3.0))
        return t.round_().clamp_(0, 4095).to(torch.int32).to(torch.int16).view(torch.uint8)
    u = torch.rand(total // 2, dtype=torch.float32, device=dev, generator=g).sub_(0.5)
    lap = u.sign() * torch.log1p(-2.0 * u.abs()).mul_(-6.0)
    return (512.0 + lap).round_().clamp_(0, 65535).to(torch.int32).to(torch.int16).view(torch.uint8)


def text_on_device(torch, dev, kind, total):
    """`total` bytes of text-like (words of a 4096-word vocabulary, Zipf-weighted, a third of them determined by the word in
    front) or log-like data (fixed-width lines: a rising timestamp, one of five levels, one of 64 sources and messages, three
    numeric fields), generated on the device (seeded)"""
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0020)
    if kind == "loglike":
        W = 96
        lines = (total + W - 1) // W
        tmpl = torch.full((64, W), 32, dtype=torch.uint8, device=dev)
        letters = torch.randint(97, 123, (64, W), dtype=torch.uint8, device=dev, generator=g)
        tmpl[:, 30:44] = letters[:, 30:44]                         # source
        tmpl[:, 45:80] = letters[:, 45:80]                         # message
        tmpl[:, 52] = 32; tmpl[:, 60] = 32; tmpl[:, 67] = 61
        out = tmpl[torch.randint(0, 64, (lines,), device=dev, generator=g)]
        levels = torch.tensor([list(b"INFO "), list(b"WARN "), list(b"DEBUG"), list(b"ERROR"), list(b"TRACE")], dtype=torch.uint8, device=dev)
        out[:, 24:29] = levels[torch.multinomial(torch.tensor([0.7, 0.1, 0.15, 0.03, 0.02], device=dev), lines, replacement=True, generator=g)]
        t = torch.randint(1, 40, (lines,), dtype=torch.int64, device=dev, generator=g).cumsum_(0).add_(1_700_000_000_000)
        for col in range(13):                                      # the timestamp, 13 decimal digits
            out[:, 12 - col] = (t % 10 + 48).to(torch.uint8)
            t //= 10
        for lo, width, top in ((14, 8, 10 ** 8), (80, 5, 3000), (88, 6, 10 ** 6)):
            v = torch.randint(0, top, (lines,), dtype=torch.int64, device=dev, generator=g)
            for col in range(width):
                out[:, lo + width - 1 - col] = (v % 10 + 48).to(torch.uint8)
                v //= 10
        out[:, W - 1] = 10
        return out.reshape(-1)[:total].contiguous()
    V, WMAX = 4096, 12
    wl = torch.randint(2, WMAX - 1, (V,), device=dev, generator=g)
    lw = torch.tensor([8.2, 1.5, 2.8, 4.3, 12.7, 2.2, 2.0, 6.1, 7.0, 0.2, 0.8, 4.0, 2.4, 6.7, 7.5, 1.9, 0.1, 6.0, 6.3, 9.1, 2.8, 1.0, 2.4, 0.2, 2.0, 0.1],
                      device=dev)
    vocab = (torch.multinomial(lw, V * WMAX, replacement=True, generator=g) + 97).to(torch.uint8).reshape(V, WMAX)
    col = torch.arange(WMAX, device=dev)
    vocab[col[None, :] == wl[:, None]] = 32                        # the space behind the word
    pw = 1.0 / torch.arange(1, V + 1, dtype=torch.float32, device=dev)
    parts, have = [], 0
    while have < total:                                            # 8 Mi words a piece
        w = torch.multinomial(pw, 1 << 23, replacement=True, generator=g)
        dep = torch.rand(w.numel(), device=dev, generator=g) < 0.35
        w[1:] = torch.where(dep[1:], (31 * w[:-1] + 7) % V, w[1:])
        keep = col[None, :] <= wl[w][:, None]
        parts.append(vocab[w][keep])
        have += parts[-1].numel()
    return torch.cat(parts)[:total].contiguous()


def runs_section(torch, glc, plan, d_in, total, rounds, with_runs):
    """the BWT container with the runs mode off and (with_runs) on, interleaved as sparse_section does it; then one profiled
    encode and decode per setting, and the two passes alone against a copy"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = ["off", "runs"] if with_runs else ["off"]
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    def enc():
        glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
            plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr()))

    def dec(clen):
        glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
            plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr()))

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            if with_runs:
                glc.container_set_runs(plan, 1 if s == "runs" else 0)
            t_enc = event_timed(enc)
            clen = int(d_len.item())
            t_dec = event_timed(lambda: dec(clen))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
        if with_runs:
            glc.container_set_runs(plan, 1 if s == "runs" else 0)
        plan.enable_timing(3)
        enc()
        plan.synchronize()
        prof_enc = plan.kernel_profiles()
        clen = int(d_len.item())
        plan.enable_timing(3)
        dec(clen)
        plan.synchronize()
        prof_dec = plan.kernel_profiles()
        plan.enable_timing(0)
        res[s]["encode_kernels_ms"] = {k: round(v["ms"], 3) for k, v in sorted(prof_enc.items(), key=lambda kv: -kv[1]["ms"])[:8]}
        res[s]["decode_kernels_ms"] = {k: round(v["ms"], 3) for k, v in sorted(prof_dec.items(), key=lambda kv: -kv[1]["ms"])[:8]}
    if with_runs:
        # the passes alone, on MTF-like bytes of the same zero density as a text block's: the input's bytes below 0x70 made zero
        nseg = min(total // n, 512)
        x = d_in[:nseg * n].clone()
        x[x < 0x70] = 0
        a, b = torch.empty_like(x), torch.empty_like(x)
        offs, lens = [i * n for i in range(nseg)], [n] * nseg
        off = torch.tensor(offs, dtype=torch.int64, device=x.device)
        ln = torch.tensor(lens, dtype=torch.int64, device=x.device)
        al, bl = torch.zeros_like(off), torch.zeros_like(off)
        L = glc._ct()
        split = lambda: glc._chk("glcZeroRunSplitSegments", L.glcZeroRunSplitSegments(x.data_ptr(), off.data_ptr(), ln.data_ptr(), nseg, n,
                                                                                       a.data_ptr(), b.data_ptr(), al.data_ptr(), bl.data_ptr(), None))
        y = torch.empty_like(x)
        join = lambda: glc._chk("glcZeroRunJoinSegments", L.glcZeroRunJoinSegments(a.data_ptr(), b.data_ptr(), off.data_ptr(), al.data_ptr(),
                                                                                    bl.data_ptr(), ln.data_ptr(), nseg, n, y.data_ptr(), None))
        split(); join()
        assert torch.equal(x, y)
        best = lambda fn: min(event_timed(fn) for _ in range(5))
        res["passes"] = {"bytes": x.numel(), "zero_fraction": float((x == 0).float().mean().item()),
                         "split_GBps": round(x.numel() / best(split) / 1e9, 1), "join_GBps": round(x.numel() / best(join) / 1e9, 1),
                         "copy_GBps": round(x.numel() / best(lambda: y.copy_(x)) / 1e9, 1)}
    return res


def choose_section(torch, glc, plan, d_in, total, rounds):
    """the container with the BWT codec, the order-0 codec and the CHOOSE codec, interleaved as sparse_section does it; then the
    bigram probe, the auto mode's probe and a copy over the same blocks"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = {"bwt": 0, "order0": 1, "choose": glc.CONTAINER_CODEC_CHOOSE}
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    def enc():
        glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
            plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr()))

    def dec(clen):
        glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
            plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr()))

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s, codec in settings.items():
            glc.container_set_codec(plan, codec)
            t_enc = event_timed(enc)
            clen = int(d_len.item())
            t_dec = event_timed(lambda: dec(clen))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                res[s]["last_choice"] = list(glc.container_last_choice(plan))
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    glc.container_set_codec(plan, 0)
    nseg = min(total // n, 512)
    x = d_in[:nseg * n]
    y = torch.empty_like(x)
    off = torch.arange(nseg, dtype=torch.int64, device=x.device) * n
    ln = torch.full((nseg,), n, dtype=torch.int64, device=x.device)
    stats = torch.empty((nseg, 4), dtype=torch.int64, device=x.device)
    hist, uni = (torch.empty((nseg, 256), dtype=torch.int32, device=x.device) for _ in range(2))
    L = glc._ct()
    bigram = lambda: glc._chk("glcBigramProbeSegments", L.glcBigramProbeSegments(x.data_ptr(), off.data_ptr(), ln.data_ptr(), nseg, n,
                                                                                   stats.data_ptr(), None))
    probe = lambda: glc._chk("glcProbeSegments", L.glcProbeSegments(x.data_ptr(), off.data_ptr(), ln.data_ptr(), nseg, n, hist.data_ptr(),
                                                                      uni.data_ptr(), None))
    bigram(); probe()
    med = lambda fn: sorted(event_timed(fn) for _ in range(5))[2]
    res["probe"] = {"bytes": x.numel(), "bigram_probe_GBps": round(x.numel() / med(bigram) / 1e9, 1),
                    "auto_probe_GBps": round(x.numel() / med(probe) / 1e9, 1), "copy_GBps": round(x.numel() / med(lambda: y.copy_(x)) / 1e9, 1)}
    return res


ARCHIVE_KINDS = ("textlike", "float32", "ts64", "noise", "grey8")


def archive_on_device(torch, L, dev, total, n, run_blocks=16):
    """`total` bytes (whole blocks of n) of the mixed input of the choose-filters section: runs of run_blocks blocks of text-like
    bytes, float32 values, int64 timestamps, noise and an 8-bit greyscale image 721 wide, in turn, each kind one stream cut into
    its runs"""
    import byte_delta_inputs
    import numpy as np
    run = run_blocks * n
    nruns = total // run
    assert nruns >= len(ARCHIVE_KINDS) and total % run == 0, "whole runs, at least one of each kind"
    out = torch.empty(total, dtype=torch.uint8, device=dev).view(nruns, run)
    for k, kind in enumerate(ARCHIVE_KINDS):
        mine = list(range(k, nruns, len(ARCHIVE_KINDS)))
        need = len(mine) * run
        if kind == "textlike":
            src = text_on_device(torch, dev, kind, need)
        elif kind == "noise":
            g = torch.Generator(device=dev)
            g.manual_seed(0x5EED0030)
            src = torch.randint(0, 256, (need,), dtype=torch.uint8, device=dev, generator=g)
        elif kind == "grey8":
            piece = torch.from_numpy(np.array(byte_delta_inputs.grey8(min(need, LAG_PIECE) // 721 * 721, 721), copy=True)).to(dev)
            src = piece.repeat((need + piece.numel() - 1) // piece.numel())[:need]
        else:
            src = typed_on_device(torch, L, dev, kind, need)[:need]
        out[mine] = src.contiguous().view(len(mine), run)
    return out.view(-1)


def choose_filters_section(torch, glc, plan, d_in, total, level, rounds):
    """the container of the mixed input under the CHOOSE codec alone, under the order-0 codec with the settings of every level up to
    `level` (the auto mode, filter-auto, filter-lag, filter-grid, filter-byte) and under the CHOOSE codec at every level up to it
    (glcPlanSetContainerChooseFilters), interleaved as sparse_section does it: ratio, encode and decode GB/s per setting, the CRC-32
    of the container, what glcContainerLastChoice and glcContainerLastFilters report"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    ladder = (glc.container_set_auto, glc.container_set_filter_auto, glc.container_set_filter_lag, glc.container_set_filter_grid,
              glc.container_set_filter_byte)

    def order0(k):
        def go():
            glc.container_set_codec(plan, 1)
            for setter in ladder[:k]:
                setter(plan, 1)
        return go

    def choose(k):
        def go():
            glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)      # (which puts the level back to 0)
            if k:
                glc.container_set_choose_filters(plan, k)
        return go

    settings = {"bwt": lambda: glc.container_set_codec(plan, 0), "order0": order0(0), "choose": choose(0)}
    for k in range(1, level + 1):
        settings["order0_level%d" % k] = order0(k)
        settings["choose_filters_level%d" % k] = choose(k)
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    def enc():
        glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
            plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr()))

    def dec(clen):
        glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
            plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr()))

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s, configure in settings.items():
            configure()
            t_enc = event_timed(enc)
            clen = int(d_len.item())
            t_dec = event_timed(lambda: dec(clen))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, round(total / clen, 4)
                res[s]["crc32"] = zlib.crc32(cont[:clen].cpu().numpy().tobytes())
                res[s]["last_choice"] = list(glc.container_last_choice(plan))
                res[s]["last_filters"] = list(glc.container_last_filters(plan))
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    glc.container_set_codec(plan, 0)
    return res


def bigram_kernels_section(torch, glc, L, dev, rounds, launches=20, span=64 * MiB):
    """k_ch_probe16 against k_ch_probe on the same segments: glcBigramProbeSegments picks the kernel by its maxLen, so the blocks of
    16 KiB and of 64 KiB of text-like bytes, Zipf bytes and zeros are probed with maxLen = the block (the one-pass kernel) and with
    maxLen = 65537 (the two-pass kernel, which the lengths keep to the same bytes), `rounds` interleaved rounds of `launches`
    launches each, timed with device events; the stats rows of the two must be equal"""
    import datagen
    import numpy as np
    data = {"textlike": text_on_device(torch, dev, "textlike", span), "zeros": torch.zeros(span, dtype=torch.uint8, device=dev)}
    z = torch.empty(span, dtype=torch.uint8, device=dev)
    thr = torch.from_numpy(datagen.zipf_thresholds().view(np.int32)).to(dev)
    assert L.glcGenZipfPhilox(z.data_ptr(), span, 0, 0x5EED0002, thr.data_ptr(), None) == 1
    data["zipf"] = z
    C = glc._ct()
    res = {}
    for blk in (16384, 65536):
        nseg = span // blk
        off = torch.arange(nseg, dtype=torch.int64, device=dev) * blk
        ln = torch.full((nseg,), blk, dtype=torch.int64, device=dev)
        for kind, x in data.items():
            stats = {k: torch.empty((nseg, 4), dtype=torch.int64, device=dev) for k in ("one_pass", "two_pass")}
            max_len = {"one_pass": blk, "two_pass": 65537}

            def run(k):
                for _ in range(launches):
                    glc._chk("glcBigramProbeSegments", C.glcBigramProbeSegments(x.data_ptr(), off.data_ptr(), ln.data_ptr(), nseg, max_len[k],
                                                                                 stats[k].data_ptr(), None))
            rates = {k: [] for k in stats}
            for r in range(rounds + 1):                            # round 0 is the warm-up
                for k in ("two_pass", "one_pass"):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    run(k)
                    b.record()
                    torch.cuda.synchronize()
                    if r:
                        rates[k].append(round(launches * span / (a.elapsed_time(b) * 1e-3) / 1e9, 1))
            assert torch.equal(stats["one_pass"], stats["two_pass"]), (blk, kind)
            row = {}
            for k, v in rates.items():
                s = sorted(v)
                row[k + "_GBps"], row[k + "_GBps_median"], row[k + "_GBps_spread"] = v, s[len(s) // 2], round(s[-1] - s[0], 1)
            row["one_pass_min_over_two_pass_max"] = round(min(rates["one_pass"]) / max(rates["two_pass"]), 3)
            res["%d KiB, %s" % (blk >> 10, kind)] = row
    return res


def filter_section(torch, glc, plan, d_in, total, elem, timed, delta=False):
    """the container with the shuffle filter off and on (with `delta`: in delta mode), on one plan: sizes, rates, kernel profile
    and sorter tiers"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    res = {}

    def enc():
        glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
            plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr()))

    for setting in (0, elem):
        glc.container_set_shuffle(plan, setting)
        if setting and delta:
            glc.container_set_delta(plan, 1)
        t_enc = timed(enc)
        clen = int(d_len.item())
        stats = dict(flagged_general=list(plan.last_sort_stats()), retries=plan.last_sort_retries(), resumed=plan.last_sort_resumed(),
                     periodic=plan.last_sort_periodic(), chains=list(plan.last_sort_chains()), skipped=plan.last_sort_skipped())
        out.zero_()
        t_dec = timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
            plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
        assert torch.equal(out, d_in) and int(d_len.item()) == total
        plan.enable_timing(3)                                  # one more pass of each for the per-kernel profile
        enc()
        plan.synchronize()
        prof_enc = plan.kernel_profiles()
        plan.enable_timing(3)
        glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
            plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr()))
        plan.synchronize()
        prof_dec = plan.kernel_profiles()
        plan.enable_timing(0)
        res["off" if not setting else ("delta%d" if delta else "elem%d") % setting] = {
            "container_bytes": clen, "ratio": total / clen, "encode_GBps": total / t_enc / 1e9, "decode_GBps": total / t_dec / 1e9,
            "last_frame_sort": stats,
            "encode_kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(prof_enc.items(), key=lambda kv: -kv[1]["ms"])},
            "decode_kernels_ms": {k: round(v["ms"], 3) for k, v in sorted(prof_dec.items(), key=lambda kv: -kv[1]["ms"])}}
    glc.container_set_shuffle(plan, 0)
    return res


def sparse_section(torch, glc, plan, d_in, total, elem, delta, rounds, with_sparse, with_ans=False, with_auto=False, with_dedup=False):
    """the order-0 container with its modes off, (with_sparse) the sparse mode on, (with_ans) the rANS mode on and (with_auto) the
    auto mode on, interleaved:
    `rounds` rounds of one encode and one decode per setting after one untimed round, each timed with device events on the plan's
    (the default) stream"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    glc.container_set_shuffle(plan, elem)
    if elem and delta:
        glc.container_set_delta(plan, 1)
    settings = ["off"] + (["sparse"] if with_sparse else []) + (["ans"] if with_ans else []) + (["auto"] if with_auto else []) + \
               (["dedup"] if with_dedup else [])
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            if with_dedup:
                glc.container_set_dedup(plan, 0)               # (the modes exclude each other: off before another goes on)
            if with_auto:
                glc.container_set_auto(plan, 0)
            if with_ans:
                glc.container_set_ans(plan, 0)
            if with_sparse:
                glc.container_set_sparse(plan, 1 if s == "sparse" else 0)
            if with_ans:
                glc.container_set_ans(plan, 1 if s == "ans" else 0)
            if with_auto:
                glc.container_set_auto(plan, 1 if s == "auto" else 0)
            if with_dedup:
                glc.container_set_dedup(plan, 1 if s == "dedup" else 0)
            t_enc = event_timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
            clen = int(d_len.item())
            t_dec = event_timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    res["working_set_bytes"] = {"input": total, "container_capacity": cap, "output": total}
    return res


def filter_auto_section(torch, glc, plan, d_in, total, elem, delta, rounds, with_filter_auto=True):
    """the order-0 container with the auto mode on under three filter settings, interleaved: "none" (no filter), "fixed" (the
    filter set by hand: elem, delta) and "filter_auto" (format version 10: a probe and a host wait per frame, the filter picked per
    frame; left out without with_filter_auto, which is what a build without it can run).  `rounds` rounds of one encode and one
    decode per setting after one untimed round, each timed with device events on the plan's (the default) stream"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = ["none", "fixed"] + (["filter_auto"] if with_filter_auto else [])
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}
    glc.container_set_auto(plan, 1)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            if with_filter_auto:
                glc.container_set_filter_auto(plan, 0)
            glc.container_set_shuffle(plan, elem if s == "fixed" else 0)
            if s == "fixed" and elem and delta:
                glc.container_set_delta(plan, 1)
            if s == "filter_auto":
                glc.container_set_filter_auto(plan, 1)
            t_enc = event_timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
            clen = int(d_len.item())
            t_dec = event_timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                res[s]["crc32"] = zlib.crc32(cont[:clen].cpu().numpy().tobytes())
                if with_filter_auto:
                    res[s]["frames_per_filter"] = list(glc.container_last_filters(plan))
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    res["working_set_bytes"] = {"input": total, "container_capacity": cap, "output": total}
    return res


def filter_lag_section(torch, glc, plan, d_in, total, elem, lag, fold, rounds, grid=0):
    """the order-0 container with the auto mode on under "filter_auto" (format version 10), "filter_lag" (format version 13: the
    filter probe and the lag probe per frame, one host wait, the filter and its lag picked per frame) and "hand" (format version 11:
    elem, lag and fold set by hand, no probe), interleaved: `rounds` rounds of one encode and one decode per setting after one
    untimed round, each timed with device events on the plan's (the default) stream.  With a row width `grid` the settings are
    "filter_lag", "filter_grid" (format version 14: the grid probe behind the two, the row width found per frame) and "hand"
    (format version 12: elem, `grid` and fold set by hand)"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = ["filter_lag", "filter_grid", "hand"] if grid else ["filter_auto", "filter_lag", "hand"]
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}
    glc.container_set_auto(plan, 1)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            glc.container_set_filter_auto(plan, 0)             # (filter-lag goes off with it)
            glc.container_set_shuffle(plan, 0)                 # (the delta and its lag go off with it)
            if s == "hand":
                glc.container_set_shuffle(plan, elem)
                glc.container_set_delta(plan, 1)
                if grid:
                    glc.container_set_delta_grid(plan, grid, fold)
                else:
                    glc.container_set_delta_lag(plan, lag, fold)
            else:
                glc.container_set_filter_auto(plan, 1)
                glc.container_set_filter_lag(plan, 0 if s == "filter_auto" else 1)
                glc.container_set_filter_grid(plan, 1 if s == "filter_grid" else 0)
            t_enc = event_timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
            clen = int(d_len.item())
            t_dec = event_timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                res[s]["version"] = int(cont[4].item()) | int(cont[5].item()) << 8
                res[s]["frames_per_filter"] = list(glc.container_last_filters(plan))
                res[s]["frames_per_lag_filter"] = list(glc.container_last_lag_filters(plan))
                res[s]["frames_per_grid_filter"] = list(glc.container_last_grid_filters(plan))
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    res["working_set_bytes"] = {"input": total, "container_capacity": cap, "output": total}
    return res


def lag_section(torch, glc, plan, d_in, total, elem, lag, fold, rounds, grid=0, volume=0):
    """the order-0 container with the auto mode on under "shuffle" (the shuffle alone), "delta" (the plain delta), "lag" (the
    delta with `lag` and `fold`, format version 11; left out at (1, 0)) and, with a row width `grid`, "grid" (the 2-D predictor
    with `fold`, format version 12) and, with a plane stride `volume` as well, "volume" (the 3-D predictor over it, format
    version 17), interleaved: `rounds` rounds of one encode and one decode per setting after one untimed round, each timed with
    device events on the plan's (the default) stream"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = ["shuffle", "delta"] + (["lag"] if (lag, fold) != (1, 0) else []) + (["grid"] if grid else []) + (["volume"] if grid and volume else [])
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}
    glc.container_set_auto(plan, 1)
    glc.container_set_shuffle(plan, elem)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            glc.container_set_delta(plan, 0 if s == "shuffle" else 1)      # (off: the lag goes back to (1, 0) with it)
            if s == "lag":
                glc.container_set_delta_lag(plan, lag, fold)
            if s in ("grid", "volume"):
                glc.container_set_delta_grid(plan, grid, fold)
            if s == "volume":
                glc.container_set_delta_volume(plan, volume)
            t_enc = event_timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
            clen = int(d_len.item())
            t_dec = event_timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
            if s == "lag":
                glc.container_set_delta_lag(plan, 1, 0)
            if s in ("grid", "volume"):
                glc.container_set_delta_grid(plan, 0, 0)       # (the volume goes off with it)
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                res[s]["version"] = int(cont[4].item()) | int(cont[5].item()) << 8
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    res["working_set_bytes"] = {"input": total, "container_capacity": cap, "output": total}
    return res


def byte_section(torch, glc, plan, d_in, total, lag, stride, rounds):
    """the order-0 container with the auto mode on under "off" (no filter, format version 8) and, unless lag is 0, "on" (the byte
    predictor at (lag, stride), format version 15), interleaved: `rounds` rounds of one encode and one decode per setting after one
    untimed round, each timed with device events on the plan's (the default) stream"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = ["off"] + (["on"] if lag else [])
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}
    glc.container_set_auto(plan, 1)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            if lag:
                glc.container_set_byte_delta(plan, lag if s == "on" else 0, stride)
            t_enc = event_timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
            clen = int(d_len.item())
            t_dec = event_timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                res[s]["version"] = int(cont[4].item()) | int(cont[5].item()) << 8
                res[s]["container_crc32"] = zlib.crc32(cont[:clen].cpu().numpy().tobytes())
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    res["working_set_bytes"] = {"input": total, "container_capacity": cap, "output": total}
    return res


def filter_byte_section(torch, glc, plan, d_in, total, lag, stride, rounds):
    """the order-0 container with the auto mode on under "filter_grid" (format version 14), "filter_byte" (format version 16: the
    byte probe behind the grid probe, the byte predictor's lag and row stride found per frame) and "hand" (format version 15: the
    byte predictor at (lag, stride) set by hand, no probe), interleaved: `rounds` rounds of one encode and one decode per setting
    after one untimed round, each timed with device events on the plan's (the default) stream"""
    n = plan.n
    cap = glc.container_bound(total, n)
    cont = torch.empty(cap, dtype=torch.uint8, device=d_in.device)
    out = torch.empty(total, dtype=torch.uint8, device=d_in.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d_in.device)
    settings = ["filter_grid", "filter_byte", "hand"]
    res = {s: {"encode_GBps": [], "decode_GBps": []} for s in settings}
    glc.container_set_auto(plan, 1)

    def event_timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for r in range(rounds + 1):                                # round 0 is the warm-up (scratch allocation, code load)
        for s in settings:
            glc.container_set_filter_auto(plan, 0)             # (filter-lag, filter-grid and filter-byte go off with it)
            glc.container_set_byte_delta(plan, 0, 0)
            if s == "hand":
                glc.container_set_byte_delta(plan, lag, stride)
            else:
                glc.container_set_filter_auto(plan, 1)
                glc.container_set_filter_lag(plan, 1)
                glc.container_set_filter_grid(plan, 1)
                glc.container_set_filter_byte(plan, 1 if s == "filter_byte" else 0)
            t_enc = event_timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
                plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
            clen = int(d_len.item())
            t_dec = event_timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
                plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
            if r == 0:
                assert torch.equal(out, d_in) and int(d_len.item()) == total
                res[s]["container_bytes"], res[s]["ratio"] = clen, total / clen
                res[s]["version"] = int(cont[4].item()) | int(cont[5].item()) << 8
                res[s]["frames_per_filter"] = list(glc.container_last_filters(plan))
                res[s]["frames_per_grid_filter"] = list(glc.container_last_grid_filters(plan))
                res[s]["frames_per_byte_filter"] = list(glc.container_last_byte_filters(plan))
                continue
            res[s]["encode_GBps"].append(round(total / t_enc / 1e9, 2))
            res[s]["decode_GBps"].append(round(total / t_dec / 1e9, 2))
    for s in settings:
        for k in ("encode_GBps", "decode_GBps"):
            v = sorted(res[s][k])
            res[s][k + "_median"], res[s][k + "_spread"] = v[len(v) // 2], round(v[-1] - v[0], 2)
    res["working_set_bytes"] = {"input": total, "container_capacity": cap, "output": total}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--pipelining", type=int, default=1)
    ap.add_argument("--data", choices=sorted(DATA_ELEM), default="zipf")
    ap.add_argument("--shuffle", type=int, default=0, choices=[0, 2, 4, 8], metavar="ELEM")
    ap.add_argument("--delta", action="store_true", help="the filtered setting uses the filter's delta mode (format version 4)")
    ap.add_argument("--codec", type=int, default=0, choices=[0, 1, 4],
                    help="the filter section's container codec: 0 BWT, 1 order-0; 4: the choose section (all three codecs, no filter)")
    ap.add_argument("--rounds", type=int, default=0, help="typed data: the sparse section, this many interleaved rounds timed with device events")
    ap.add_argument("--sparse", action="store_true", help="the sparse section also runs the order-0 codec's sparse mode (format version 5)")
    ap.add_argument("--ans", action="store_true", help="the sparse section also runs the order-0 codec's rANS mode (format version 7)")
    ap.add_argument("--auto", action="store_true", help="the sparse section also runs the order-0 codec's auto mode (format version 8)")
    ap.add_argument("--dedup", action="store_true", help="the sparse section also runs the order-0 codec's dedup mode (format version 9)")
    ap.add_argument("--runs", action="store_true", help="text-like data: the runs section, the BWT codec's runs mode off and on (format version 6)")
    ap.add_argument("--runs-off-only", action="store_true", help="the runs section without the mode (what a build without it can run)")
    ap.add_argument("--filter-auto", action="store_true",
                    help="the filter-auto section (format version 10): the auto mode with no filter, with --shuffle / --delta set by hand and with filter-auto")
    ap.add_argument("--filter-auto-off-only", action="store_true", help="the filter-auto section without the setting (what a build without it can run)")
    ap.add_argument("--lag", type=int, default=0, metavar="L", help="the lag section (format version 11): the delta's lag, 1 to 16")
    ap.add_argument("--filter-lag", action="store_true",
                    help="the filter-lag section (format version 13): filter-auto, filter-auto with lag, and elem / --lag / --fold set by hand")
    ap.add_argument("--filter-grid", action="store_true",
                    help="the filter-grid section (format version 14): filter-lag, filter-lag with grid, and elem / --grid / --fold set by hand")
    ap.add_argument("--fold", action="store_true", help="the lag or grid section's delta folds its sign")
    ap.add_argument("--grid", type=int, default=0, metavar="W", help="the grid section (format version 12): the 2-D predictor's row width, 2 to 65536")
    ap.add_argument("--volume", type=int, default=0, metavar="S", help="with --grid W: the 3-D predictor's plane stride (format version 17), above W, up to 2^24")
    ap.add_argument("--byte-delta", default=None, metavar="LAG,STRIDE",
                    help="the byte section (format version 15): the byte predictor's lag, 0 (off only) to 16, and row stride, 0 or 2 to 65536")
    ap.add_argument("--filter-byte", action="store_true",
                    help="the filter-byte section (format version 16): filter-grid, filter-grid with bytes, and --byte-delta set by hand")
    ap.add_argument("--choose-filters", type=int, default=None, choices=range(0, 6), metavar="LEVEL",
                    help="the choose-filters section: the mixed input under CHOOSE, the order-0 codec at every level's settings and CHOOSE at every level up to LEVEL")
    ap.add_argument("--block-kib", type=int, default=1024, help="the choose-filters section's block size in KiB (1 to 1024)")
    ap.add_argument("--bigram-kernels", action="store_true", help="the bigram probe's one-pass kernel against its two-pass kernel at 16 and 64 KiB blocks")
    args = ap.parse_args()
    byte_delta = tuple(int(v) for v in args.byte_delta.split(",")) if args.byte_delta else None
    assert byte_delta is None or len(byte_delta) == 2, "--byte-delta LAG,STRIDE"
    import importlib.util
    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    sys.modules["glc_binding"] = glc
    import datagen
    L = glc.lib()
    dev = torch.device("cuda:0")
    if args.bigram_kernels:
        print(json.dumps({"workload": "bigram probe kernels, 64 MiB a kind", "bigram_kernels": bigram_kernels_section(torch, glc, L, dev, max(1, args.rounds))}))
        return
    if args.choose_filters is not None:
        n = args.block_kib << 10
        total = int(args.gib * 1024 * MiB) // (16 * n) * (16 * n)
        d_in = archive_on_device(torch, L, dev, total, n)
        torch.cuda.synchronize()
        res = {"workload": "archive (runs of 16 blocks of %s): %d x %d KiB blocks, plan rows %d, pipelining %s"
                           % (", ".join(ARCHIVE_KINDS), total // n, args.block_kib, args.rows, bool(args.pipelining))}
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            res["choose_filters"] = choose_filters_section(torch, glc, plan, d_in, total, args.choose_filters, max(1, args.rounds))
        print(json.dumps(res))
        return
    n = MiB
    nblocks = int(args.gib * 1024)
    total = nblocks * n
    if args.data in ("pages", "pages_noise"):                 # the model's own generator, on the host
        import dedup_inputs
        d_in = torch.from_numpy(np.array(dedup_inputs.make(args.data, total), copy=True)).to(dev)
    elif args.data in ("stereo16", "adc16x8", "xyz32", "cplx64", "i32x4"):
        import lag_inputs
        assert args.lag, "the interleaved kinds are the lag section's"
        piece = torch.from_numpy(lag_inputs.lag_bytes(args.data, min(total, LAG_PIECE))).to(dev)
        d_in = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
    elif args.data in ("img16", "field32", "walk32"):
        import grid_inputs
        assert args.grid, "the grids are the grid section's"
        row = args.grid * grid_inputs.KINDS[args.data]
        piece = torch.from_numpy(grid_inputs.grid_bytes(args.data, max(row, min(total, LAG_PIECE) // row * row), args.grid)).to(dev)      # whole rows
        d_in = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
    elif args.data in VOL_KINDS:
        import vol_inputs
        assert args.grid and args.volume > args.grid, "the volumes are the grid section's with --volume"
        plane = args.volume * DATA_ELEM[args.data]
        piece = torch.from_numpy(vol_inputs.vol_bytes(VOL_KINDS[args.data], max(plane, min(total, LAG_PIECE) // plane * plane), args.grid, args.volume)).to(dev)   # whole planes
        d_in = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
    elif args.data in ("grey8", "rgb8"):
        import byte_delta_inputs
        assert byte_delta, "the 8-bit images are the byte section's"
        ch = 3 if args.data == "rgb8" else 1
        row = byte_delta[1] or 721 * ch
        assert row % ch == 0, "a row of whole pixels"
        gen = byte_delta_inputs.rgb8 if ch == 3 else byte_delta_inputs.grey8
        piece = torch.from_numpy(gen(max(row, min(total, LAG_PIECE) // row * row), row // ch)).to(dev)      # whole rows
        d_in = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
    elif args.data in ("zipf", "mix"):
        d_in = torch.empty(total, dtype=torch.uint8, device=dev)
        thr = torch.from_numpy(datagen.zipf_thresholds().view(np.int32)).to(dev)
        assert L.glcGenZipfPhilox(d_in.data_ptr(), total, 0, 0x5EED0002, thr.data_ptr(), None) == 1
        if args.data == "mix":                                 # every other run of 64 blocks is text-like
            assert args.codec == 4, "the mix is the choose section's"
            runs = d_in[:total // (128 * n) * 128 * n].view(-1, 2, 64 * n)
            runs[:, 1, :] = text_on_device(torch, dev, "textlike", runs.shape[0] * 64 * n).view(-1, 64 * n)
    elif args.data in ("textlike", "loglike"):
        assert args.runs or args.runs_off_only or args.codec == 4 or args.filter_auto or args.filter_auto_off_only, \
            "text-like data is the runs, the choose and the filter-auto section's"
        d_in = text_on_device(torch, dev, args.data, total)
    else:
        d_in = typed_on_device(torch, L, dev, args.data, total)
    torch.cuda.synchronize()

    def timed(fn):
        fn()                                                   # warm-up
        torch.cuda.synchronize()
        best = 1e30
        for _ in range(args.iters):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        return best

    res = {"workload": "%s: %d x 1 MiB blocks, plan rows %d, pipelining %s"
                       % ("configs[1] Philox Zipf(1.0)" if args.data == "zipf" else args.data, nblocks, args.rows, bool(args.pipelining))}
    if args.codec == 4:
        assert args.data in ("zipf", "mix", "textlike", "loglike") and not args.shuffle, "the choose section takes untyped data and no filter"
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            res["choose"] = choose_section(torch, glc, plan, d_in, total, max(1, args.rounds))
        print(json.dumps(res))
        return
    if args.runs or args.runs_off_only:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            res["runs"] = runs_section(torch, glc, plan, d_in, total, max(1, args.rounds), args.runs)
        print(json.dumps(res))
        return
    if args.filter_byte:
        assert byte_delta and byte_delta[0], "--filter-byte compares with the plan set by hand: give its --byte-delta LAG,STRIDE"
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["filter_byte"] = filter_byte_section(torch, glc, plan, d_in, total, byte_delta[0], byte_delta[1], max(1, args.rounds))
        print(json.dumps(res))
        return
    if byte_delta:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["byte_delta"] = byte_section(torch, glc, plan, d_in, total, byte_delta[0], byte_delta[1], max(1, args.rounds))
        print(json.dumps(res))
        return
    if args.filter_grid:
        assert args.grid, "--filter-grid compares with the plan set by hand: give its --grid (and --fold)"
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["filter_grid"] = filter_lag_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM[args.data], 1, int(args.fold),
                                                    max(1, args.rounds), args.grid)
        print(json.dumps(res))
        return
    if args.grid:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["grid"] = lag_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM[args.data], 1, int(args.fold), max(1, args.rounds), args.grid,
                                      args.volume)
        print(json.dumps(res))
        return
    if args.filter_lag:
        assert args.lag, "--filter-lag compares with the plan set by hand: give its --lag (and --fold)"
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["filter_lag"] = filter_lag_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM[args.data], args.lag, int(args.fold),
                                                   max(1, args.rounds))
        print(json.dumps(res))
        return
    if args.lag:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["lag"] = lag_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM[args.data], args.lag, int(args.fold), max(1, args.rounds))
        print(json.dumps(res))
        return
    if args.filter_auto or args.filter_auto_off_only:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, 1)
            res["filter_auto"] = filter_auto_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM.get(args.data, 0), args.delta,
                                                     max(1, args.rounds), args.filter_auto)
        print(json.dumps(res))
        return
    if args.data != "zipf" or args.dedup:
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
            plan.set_pipelining(bool(args.pipelining))
            glc.container_set_codec(plan, args.codec)
            res["codec"] = args.codec
            if args.rounds:
                assert args.codec == 1, "the sparse section is the order-0 codec's"
                res["sparse"] = sparse_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM[args.data], args.delta, args.rounds,
                                               args.sparse, args.ans, args.auto, args.dedup)
            else:
                res["filter"] = filter_section(torch, glc, plan, d_in, total, args.shuffle or DATA_ELEM[args.data], timed, args.delta)
        print(json.dumps(res))
        return
    # --- CRC against the read probe
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = torch.full((1,), total, dtype=torch.int64, device=dev)
    crc = torch.zeros(1, dtype=torch.int32, device=dev)
    t_crc = timed(lambda: glc._chk("glcCrc32Segments", glc._ct().glcCrc32Segments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), 1,
                                                                                 crc.data_ptr(), None)))
    import ctypes as C
    ms = C.c_float(0)
    assert L.glcProbeStreamRead(d_in.data_ptr(), total, 5, C.byref(ms), None) == 1
    res["crc_GBps"] = total / t_crc / 1e9
    res["probe_read_GBps"] = total / (ms.value * 1e-3) / 1e9
    res["crc_vs_probe"] = res["crc_GBps"] / res["probe_read_GBps"]

    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=args.rows) as plan:
        plan.set_pipelining(bool(args.pipelining))
        nsub = n // 4096
        bwt = torch.empty(nblocks, dtype=torch.int32, device=dev)
        hist = torch.empty(nblocks * 256, dtype=torch.int32, device=dev)
        offs = torch.empty(nblocks * nsub, dtype=torch.int32, device=dev)
        size = torch.empty(nblocks, dtype=torch.int32, device=dev)
        compact = torch.empty(nblocks * (n // 4 + nsub + 1), dtype=torch.int32, device=dev)   # (Zipf(1.0) bytes shrink: a word per 4 input bytes is room)
        coff = torch.empty(nblocks + 1, dtype=torch.int64, device=dev)

        def enc_compact():
            for b0 in range(0, nblocks, args.rows):
                nb = min(args.rows, nblocks - b0)
                rc = L.glcCompressBatchCompact(plan.handle, d_in.data_ptr() + b0 * n, bwt.data_ptr() + 4 * b0, hist.data_ptr() + 1024 * b0,
                                               offs.data_ptr() + 4 * nsub * b0, nsub, size.data_ptr() + 4 * b0, compact.data_ptr(),
                                               compact.numel(), coff.data_ptr() + 8 * b0, (coff.data_ptr() + 8 * b0) if b0 else None, n, nb)
                assert rc == 0, rc
            plan.synchronize()

        t_enc = timed(enc_compact)
        compact_bytes = 4 * int(coff[nblocks].item())
        cap = glc.container_bound(total, n)
        cont = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_len = torch.zeros(1, dtype=torch.int64, device=dev)
        t_cenc = timed(lambda: glc._chk("glcContainerCompressDevice", glc._ct().glcContainerCompressDevice(
            plan.handle, d_in.data_ptr(), total, cont.data_ptr(), cap, d_len.data_ptr())))
        clen = int(d_len.item())
        out = torch.empty(total, dtype=torch.uint8, device=dev)

        def dec_compact():
            for b0 in range(0, nblocks, args.rows):
                nb = min(args.rows, nblocks - b0)
                rc = L.glcDecompressBatchCompact(plan.handle, bwt.data_ptr() + 4 * b0, hist.data_ptr() + 1024 * b0,
                                                 offs.data_ptr() + 4 * nsub * b0, nsub, compact.data_ptr(), compact.numel(),
                                                 coff.data_ptr() + 8 * b0, out.data_ptr() + b0 * n, n, nb)
                assert rc == 0, rc
            plan.synchronize()

        t_dec = timed(dec_compact)
        assert torch.equal(out, d_in)
        out.zero_()
        t_cdec = timed(lambda: glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(
            plan.handle, cont.data_ptr(), clen, out.data_ptr(), total, d_len.data_ptr())))
        assert torch.equal(out, d_in) and int(d_len.item()) == total
        if args.shuffle:
            del compact, out
            glc.container_set_codec(plan, args.codec)
            res["codec"] = args.codec
            res["filter"] = filter_section(torch, glc, plan, d_in, total, args.shuffle, timed, args.delta)
            glc.container_set_codec(plan, 0)
    res.update({"compact_encode_GBps": total / t_enc / 1e9, "container_encode_GBps": total / t_cenc / 1e9,
                "encode_ratio": t_enc / t_cenc,
                "compact_decode_GBps": total / t_dec / 1e9, "container_decode_GBps": total / t_cdec / 1e9,
                "decode_ratio": t_dec / t_cdec,
                "compact_bytes": compact_bytes, "container_bytes": clen, "size_overhead": clen / compact_bytes - 1})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
