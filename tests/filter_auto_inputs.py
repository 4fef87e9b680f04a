"""Inputs of the filter-auto tests (tests/filter_auto_model.py, format version 10), shared by the CPU and the GPU tests."""
import numpy as np

import datagen
import series_datagen
import typed_datagen

N, ROWS = 16384, 8


def four_frames():
    """four frames at n = 16384, rows 8: int64 timestamps, text, float32 and a ragged tail of uint32 counters"""
    F = N * ROWS
    return np.concatenate([np.ascontiguousarray(series_datagen.series_bytes("ts64", F)), datagen.text_bytes_fast(F),
                           np.frombuffer(typed_datagen.typed_bytes("float32", F), np.uint8),
                           np.ascontiguousarray(series_datagen.series_bytes("ctr32", 5000))[:4999]])


def for_candidate(cand, n=N):
    """three blocks of n bytes that the rule gives candidate `cand` of filter_auto_model.CANDS"""
    m = 3 * n
    if cand == 0:
        return datagen.text_bytes_fast(m)
    if cand == 5:                                                  # uint64 values below 2^20: five zero planes, and a delta only hurts
        return np.random.default_rng(5).integers(0, 1 << 20, m // 8, dtype=np.uint64).astype("<u8").view(np.uint8)
    kind = {1: "quant16", 2: "adc16", 3: "float32", 4: "ctr32", 6: "ts64"}[cand]
    if kind in typed_datagen.KINDS:
        return np.frombuffer(typed_datagen.typed_bytes(kind, m), np.uint8)
    return np.ascontiguousarray(series_datagen.series_bytes(kind, m))
