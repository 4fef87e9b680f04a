"""Inputs of the filter-lag tests (tests/filter_lag_model.py, format version 13), shared by the CPU and the GPU tests and by
tests/golden/make_filter_lag_v13_gold.py."""
import numpy as np

import datagen
import lag_inputs
import series_datagen
import typed_datagen

N, ROWS = 8192, 2
FRAME = N * ROWS
# the frames of the mixed stream and the candidate (elem, delta, lag, fold) the rule gives each at 16 KiB
FRAMES = (("stereo16", (2, 1, 2, 1)), ("text", (1, 0, 1, 0)), ("adc16x8", (2, 1, 8, 1)), ("ts64", (8, 1, 1, 1)), ("xyz32", (4, 1, 3, 1)),
          ("float32", (4, 0, 1, 0)))
TAIL = 3001


def frame_bytes(kind, n=FRAME):
    if kind in lag_inputs.KINDS:
        return lag_inputs.lag_bytes(kind, n)
    if kind == "text":
        return np.ascontiguousarray(datagen.text_bytes_fast(n))
    if kind in typed_datagen.KINDS:
        return np.frombuffer(typed_datagen.typed_bytes(kind, n), np.uint8).copy()
    return np.ascontiguousarray(series_datagen.series_bytes(kind, n))


def mixed_stream():
    """six frames of 16 KiB at n = 8192, rows 2 -- stereo audio, text, an 8-channel ADC dump, int64 timestamps, xyz points and
    float32 -- and a ragged tail of four interleaved int32 counters"""
    return np.concatenate([frame_bytes(k) for k, _ in FRAMES] + [lag_inputs.lag_bytes("i32x4", TAIL + 7)[:TAIL]])
