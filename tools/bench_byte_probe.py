"""The byte probe alone (csrc/byte_probe.hip) beside its siblings, each call over --gib GiB as ONE segment (a frame, as the
container's writer probes it) of the greyscale image 721 wide and the RGB image 427 wide of tests/byte_delta_inputs.py (32 MiB of
whole rows made on the host and repeated); --rounds interleaved rounds after one warm-up, each call timed with device events;
medians and spreads (max - min) in one JSON line per input.

  byte_sums    glcByteProbeSegments: a memset, k_bp_init, k_bp_lags, k_bp_strides, k_bp_argmin
  byte_sample  the same call over the first 132 KiB alone: the stride sample (k_bp_strides) is the same work at any length from
               there on and k_bp_lags has next to nothing to read, so this is the constant part of byte_sums
  byte_planes  glcBytePlanesSegments at the winners: a memset of the rows, k_bp_planes, k_bp_cost
  lag_sums     glcLagProbeSegments (k_lp_sums), lag_planes glcLagPlanesSegments (k_lp_planes)
  grid_sums    glcGridProbeSegments (the two instances of k_gw_sums), grid_planes glcGridPlanesSegments (k_gw_planes x 3)
  copy         a device-to-device copy

python tools/bench_byte_probe.py [--gib 1] [--rounds 5]"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import byte_delta_inputs as BI
    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    dev = torch.device("cuda:0")
    total = int(args.gib * 1024) * MiB
    assert total <= glc.FILTER_PROBE_MAX_LEN, "one segment holds at most 2 GiB"
    L = glc._ct()
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = torch.full((1,), total, dtype=torch.int64, device=dev)
    ln_small = torch.full((1,), 132 << 10, dtype=torch.int64, device=dev)
    lag_sums = torch.empty(48, dtype=torch.int64, device=dev)
    lags = torch.empty(4, dtype=torch.int32, device=dev)
    rows14 = torch.empty(14 * 256, dtype=torch.int32, device=dev)
    costs = torch.empty(3, dtype=torch.int64, device=dev)
    gsums = torch.empty(glc.GRID_PROBE_SUMS, dtype=torch.int32, device=dev)
    widths = torch.empty(4, dtype=torch.int32, device=dev)
    bl = torch.empty(16, dtype=torch.int64, device=dev)
    bs = torch.empty(glc.BYTE_PROBE_ROW, dtype=torch.int32, device=dev)
    bw = torch.empty(2, dtype=torch.int32, device=dev)
    rows2 = torch.empty(2 * 256, dtype=torch.int32, device=dev)

    def ok(r):
        assert r == glc.CUDPP_SUCCESS

    for name, gen, row in (("grey8 at 721", lambda n: BI.grey8(n, 721), 721), ("rgb8 at 427", lambda n: BI.rgb8(n, 427), 1281)):
        piece = torch.from_numpy(gen((32 * MiB) // row * row)).to(dev)
        d = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
        dst = torch.empty_like(d)
        p = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, total]
        small = [d.data_ptr(), off.data_ptr(), ln_small.data_ptr(), 1, 132 << 10]
        calls = {
            "byte_sums": lambda: ok(L.glcByteProbeSegments(*p, bl.data_ptr(), bs.data_ptr(), bw.data_ptr(), None)),
            "byte_sample": lambda: ok(L.glcByteProbeSegments(*small, bl.data_ptr(), bs.data_ptr(), bw.data_ptr(), None)),
            "byte_planes": lambda: ok(L.glcBytePlanesSegments(*p, bw.data_ptr(), rows2.data_ptr(), costs.data_ptr(), None)),
            "lag_sums": lambda: ok(L.glcLagProbeSegments(*p, lag_sums.data_ptr(), lags.data_ptr(), None)),
            "lag_planes": lambda: ok(L.glcLagPlanesSegments(*p, lags.data_ptr(), rows14.data_ptr(), costs.data_ptr(), None)),
            "grid_sums": lambda: ok(L.glcGridProbeSegments(*p, gsums.data_ptr(), widths.data_ptr(), None)),
            "grid_planes": lambda: ok(L.glcGridPlanesSegments(*p, widths.data_ptr(), rows14.data_ptr(), costs.data_ptr(), None)),
            "copy": lambda: dst.copy_(d),
        }
        ms = {k: [] for k in calls}
        for r in range(args.rounds + 1):                           # round 0 is the warm-up
            for k, fn in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if r:
                    ms[k].append(a.elapsed_time(b))
            if r == 0:
                ok(L.glcByteProbeSegments(*p, bl.data_ptr(), bs.data_ptr(), bw.data_ptr(), None))      # (byte_sample overwrote the winners)
                torch.cuda.synchronize()
                winners = bw.cpu().tolist()
        res = {"input": name, "bytes": total, "winners": winners}
        for k, v in ms.items():
            v = sorted(v)
            med = v[len(v) // 2]
            res[k] = {"ms_median": round(med, 3), "ms_spread": round(v[-1] - v[0], 3), "GBps_median": round(total / med / 1e6, 1)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
