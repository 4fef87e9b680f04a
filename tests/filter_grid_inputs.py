"""Inputs of the filter-grid tests (tests/filter_grid_model.py, format version 14), shared by the CPU and the GPU tests and by
tests/golden/make_filter_grid_v14_gold.py."""
import numpy as np

import filter_lag_inputs
import grid_inputs
import lag_inputs

N, ROWS = 65536, 4
FRAME = N * ROWS
# the frames of the mixed stream -- (kind, row width or None) -- and the candidate (elem, delta, lag, fold, width) the rule gives
# each at 256 KiB: two grids of different widths, text, an interleaved ADC dump (a lag frame) and a 1-D series
FRAMES = ((("img16", 640), (2, 1, 1, 1, 640)), (("text", None), (1, 0, 1, 0, 0)), (("walk32", 300), (4, 1, 1, 1, 300)),
          (("adc16x8", None), (2, 1, 8, 1, 0)), (("ts64", None), (8, 1, 1, 1, 0)))
TAIL = 3001
TAIL_PICK = (4, 1, 4, 1, 0)
# the segment whose sums the golden fixture keeps for tests/test_gpu_grid_probe.py: kind, row width, bytes
PROBE_BIG = ("walk32", 721, 1 << 18)


def frame_bytes(kind, width=None, n=FRAME):
    if width:
        return grid_inputs.grid_bytes(kind, n, width)
    return filter_lag_inputs.frame_bytes(kind, n)


def mixed_stream():
    """five frames of 256 KiB at n = 65536, rows 4 -- a 12-bit image 640 wide, text, an int32 2-D walk 300 wide, an 8-channel ADC
    dump and int64 timestamps -- and a ragged tail of four interleaved int32 counters"""
    return np.concatenate([frame_bytes(k, w) for (k, w), _ in FRAMES] + [lag_inputs.lag_bytes("i32x4", TAIL + 7)[:TAIL]])
