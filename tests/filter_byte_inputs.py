"""Inputs of the filter-byte tests (tests/filter_byte_model.py, format version 16), shared by the CPU and the GPU tests and by
tests/golden/make_filter_byte_v16_gold.py."""
import numpy as np

import byte_delta_inputs as BI
import filter_grid_inputs as QI
import filter_lag_inputs

N, ROWS = 65536, 4
FRAME = N * ROWS
# the frames of the mixed stream -- (kind, row width in pixels or None) -- and the candidate (elem, delta, lag, fold, width) the rule
# gives each at 256 KiB; a byte candidate is (1, 1, lag, 0, stride)
FRAMES = ((("grey8", 721), (1, 1, 1, 0, 721)), (("text", None), (1, 0, 1, 0, 0)), (("rgb8", 427), (1, 1, 3, 0, 1281)),
          (("img16", 640), (2, 1, 1, 1, 640)), (("stereo8", None), (1, 1, 2, 0, 0)), (("ts64", None), (8, 1, 1, 1, 0)))
TAIL = 3001
# the segment whose sums and rows the golden fixture keeps for tests/test_gpu_byte_probe_kernels.py: kind, row width, bytes
PROBE_BIG = ("rgb8", 427, 1 << 18)


def frame_bytes(kind, width=None, n=FRAME):
    if kind == "grey8":
        return BI.grey8(n, width)
    if kind == "rgb8":
        return BI.rgb8(n, width)
    if kind == "stereo8":
        return BI.stereo8(n)
    if kind == "text":
        return BI.text(n)
    if kind == "noise":
        return BI.noise(n)
    if kind == "img16":
        return QI.frame_bytes(kind, width, n)
    return filter_lag_inputs.frame_bytes(kind, n)


def mixed_stream():
    """six frames of 256 KiB at n = 65536, rows 4 -- a greyscale image 721 wide, text, an RGB image 427 wide, a 12-bit image 640
    wide, 8-bit stereo audio and int64 timestamps -- and a ragged tail of 3001 bytes of a greyscale image 100 wide"""
    return np.concatenate([frame_bytes(k, w) for (k, w), _ in FRAMES] + [BI.grey8(TAIL, 100)])
