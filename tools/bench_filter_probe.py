"""The filter probe alone (csrc/filter_probe.hip, glcFilterProbeSegments) against a device-to-device copy of the same bytes:
--gib GiB as ONE segment (a frame, as the container's writer probes it) and as segments of 1 MiB, of zeros, int64 timestamps
(the running sum of steps uniform in [900, 1100): tests/series_datagen.py's ts64, made on the device), float32 ~ N(0, 1) and noise;
--rounds interleaved rounds after one warm-up, each call timed with device events; medians and spreads (max - min) in one JSON line
per input, with the candidate the rule picks from the costs.

  frame    glcFilterProbeSegments over the whole buffer as one segment: a memset of the rows, k_fp_probe, k_fp_cost
  blocks   the same call over segments of 1 MiB
  copy     a device-to-device copy


--lag adds the lag probe (csrc/lag_probe.hip) over the same buffer as one segment, in the same interleaved rounds, and two
interleaved-channel inputs (adc16x8 and xyz32 of tests/lag_inputs.py, 32 MiB made on the host and repeated):
  lag_sums    glcLagProbeSegments: a memset of the sums, k_lp_sums, k_lp_argmin
  lag_planes  glcLagPlanesSegments at the winners: a memset of the rows, k_lp_planes, k_lp_cost
with the winners and the candidate the ten-cost walk picks.

--filter-grid (with --lag) adds the grid probe (csrc/grid_probe.hip) in the same way, and three gridded inputs (img16 at row width
1024, field32 at 1800 and walk32 at 721 of tests/grid_inputs.py, 32 MiB of whole rows made on the host and repeated):
  grid_sums    glcGridProbeSegments: k_gw_init, the two instances of k_gw_sums, k_gw_argmin
  grid_planes  glcGridPlanesSegments at the winners: a memset of the rows, the three instances of k_gw_planes, k_lp_cost
with the widths, the candidate the thirteen-cost walk picks and, because the first call costs the same for every length, both
calls' medians in milliseconds as well.

python tools/bench_filter_probe.py [--gib 1] [--rounds 5] [--lag [--filter-grid]]"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
MiB = 1 << 20

from filter_auto_model import CANDS, pick  # noqa: E402  (the rule and its margin are the model's)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lag", action="store_true", help="also the lag probe, and the interleaved-channel inputs")
    ap.add_argument("--filter-grid", action="store_true", help="also the grid probe, and the gridded inputs (needs --lag)")
    args = ap.parse_args()
    assert args.lag or not args.filter_grid, "--filter-grid adds to --lag"
    import torch
    spec = importlib.util.spec_from_file_location("glc_binding", os.path.join(ROOT, "gpu-lossless-compression_amd", "glc_binding.py"))
    glc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(glc)
    dev = torch.device("cuda:0")
    count = int(args.gib * 1024)
    total = count * MiB
    assert total <= glc.FILTER_PROBE_MAX_LEN, "one segment holds at most 2 GiB"
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0011)
    off = torch.arange(count, dtype=torch.int64, device=dev) * MiB
    ln = torch.full((count,), MiB, dtype=torch.int64, device=dev)
    off1 = torch.zeros(1, dtype=torch.int64, device=dev)
    ln1 = torch.full((1,), total, dtype=torch.int64, device=dev)
    planes = torch.empty((count, 22, 256), dtype=torch.int32, device=dev)
    costs = torch.empty((count, 7), dtype=torch.int64, device=dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    lp_sums = torch.empty((1, 48), dtype=torch.int64, device=dev)
    lp_lags = torch.empty((1, 3), dtype=torch.int32, device=dev)
    lp_planes = torch.empty((1, 14, 256), dtype=torch.int32, device=dev)
    lp_costs = torch.empty((1, 3), dtype=torch.int64, device=dev)
    gw_sums = torch.empty((1, glc.GRID_PROBE_SUMS), dtype=torch.int32, device=dev)
    gw_widths = torch.empty((1, 3), dtype=torch.int32, device=dev)
    gw_planes = torch.empty((1, 14, 256), dtype=torch.int32, device=dev)
    gw_costs = torch.empty((1, 3), dtype=torch.int64, device=dev)
    GRIDS = {"img16": 1024, "field32": 1800, "walk32": 721}
    L = glc._ct()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for name in ("zeros", "ts64", "float32", "noise") + (("adc16x8", "xyz32") if args.lag else ()) + (tuple(GRIDS) if args.filter_grid else ()):
        if name == "zeros":
            d_in = torch.zeros(total, dtype=torch.uint8, device=dev)
        elif name == "ts64":
            d_in = torch.cumsum(torch.randint(900, 1100, (total // 8,), dtype=torch.int64, device=dev, generator=g), 0).view(torch.uint8)
        elif name in ("adc16x8", "xyz32"):
            import lag_inputs
            import numpy as np
            piece = torch.from_numpy(np.array(lag_inputs.lag_bytes(name, min(total, 32 * MiB)), copy=True)).to(dev)
            d_in = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
        elif name in GRIDS:
            import grid_inputs
            import numpy as np
            row = GRIDS[name] * grid_inputs.KINDS[name]
            piece = torch.from_numpy(grid_inputs.grid_bytes(name, max(row, min(total, 32 * MiB) // row * row), GRIDS[name])).to(dev)
            d_in = piece.repeat((total + piece.numel() - 1) // piece.numel())[:total].contiguous()
        elif name == "float32":
            d_in = torch.randn(total // 4, dtype=torch.float32, device=dev, generator=g).view(torch.uint8)
        else:
            d_in = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)

        def frame():
            glc._chk("glcFilterProbeSegments", L.glcFilterProbeSegments(d_in.data_ptr(), off1.data_ptr(), ln1.data_ptr(), 1, total,
                                                                         planes.data_ptr(), costs.data_ptr(), None))

        def blocks():
            glc._chk("glcFilterProbeSegments", L.glcFilterProbeSegments(d_in.data_ptr(), off.data_ptr(), ln.data_ptr(), count, MiB,
                                                                         planes.data_ptr(), costs.data_ptr(), None))

        def copy():
            out.copy_(d_in)

        def lag_sums():
            glc._chk("glcLagProbeSegments", L.glcLagProbeSegments(d_in.data_ptr(), off1.data_ptr(), ln1.data_ptr(), 1, total,
                                                                   lp_sums.data_ptr(), lp_lags.data_ptr(), None))

        def lag_planes():
            glc._chk("glcLagPlanesSegments", L.glcLagPlanesSegments(d_in.data_ptr(), off1.data_ptr(), ln1.data_ptr(), 1, total, lp_lags.data_ptr(),
                                                                     lp_planes.data_ptr(), lp_costs.data_ptr(), None))

        def grid_sums():
            glc._chk("glcGridProbeSegments", L.glcGridProbeSegments(d_in.data_ptr(), off1.data_ptr(), ln1.data_ptr(), 1, total,
                                                                     gw_sums.data_ptr(), gw_widths.data_ptr(), None))

        def grid_planes():
            glc._chk("glcGridPlanesSegments", L.glcGridPlanesSegments(d_in.data_ptr(), off1.data_ptr(), ln1.data_ptr(), 1, total, gw_widths.data_ptr(),
                                                                       gw_planes.data_ptr(), gw_costs.data_ptr(), None))

        calls = (("frame_GBps", frame), ("blocks_GBps", blocks), ("copy_GBps", copy)) + \
                ((("lag_sums_GBps", lag_sums), ("lag_planes_GBps", lag_planes)) if args.lag else ()) + \
                ((("grid_sums_GBps", grid_sums), ("grid_planes_GBps", grid_planes)) if args.filter_grid else ())
        res = {k: [] for k, _ in calls}
        for r in range(args.rounds + 1):                        # round 0 is the warm-up
            for k, fn in calls:
                t = timed(fn)
                if r:
                    res[k].append(round(total / t / 1e9, 2))
        block_rows = planes.to(torch.int64).sum(dim=0)          # the segments of 1 MiB start on delta restarts: their rows add up
        frame()
        torch.cuda.synchronize()
        assert torch.equal(planes[0].to(torch.int64), block_rows) and int(planes[0, :8].sum(dtype=torch.int64).item()) == total
        c = [int(v) for v in costs[0].cpu().tolist()]
        rep = {"workload": "%d MiB of %s" % (count, name), "costs_bytes": [v // 2048 for v in c], "pick": list(CANDS[pick(c)])}
        if args.lag:
            import filter_lag_model as FL
            lags = [int(v) for v in lp_lags[0].cpu().tolist()]
            c10 = c + [int(v) for v in lp_costs[0].cpu().tolist()]
            assert int(lp_planes.sum(dtype=torch.int64).item()) == 3 * total
            rep.update({"lags": lags, "lag_costs_bytes": [v // 2048 for v in c10[7:]], "lag_pick": list(FL.cands(lags)[FL.pick(c10)])})
        if args.filter_grid:
            import filter_grid_model as Q
            widths = [int(v) for v in gw_widths[0].cpu().tolist()]
            c13 = c10 + [int(v) for v in gw_costs[0].cpu().tolist()]
            assert int(gw_planes.sum(dtype=torch.int64).item()) == sum(total // 8 * 8 for w in widths if w)
            rep.update({"widths": widths, "grid_costs_bytes": [v // 2048 for v in c13[10:]], "grid_pick": list(Q.cands(lags, widths)[Q.pick(c13)])})
        for k, v in res.items():
            s = sorted(v)
            rep[k], rep[k + "_median"], rep[k + "_spread"] = v, s[len(s) // 2], round(s[-1] - s[0], 2)
            if k.startswith("grid_"):
                rep[k[:-4] + "ms_median"] = round(total / (s[len(s) // 2] * 1e9) * 1e3, 4)
        print(json.dumps(rep))
        del d_in


if __name__ == "__main__":
    sys.exit(main())
