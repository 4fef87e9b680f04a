"""Inputs of the choose-filters tests (tests/choose_filters_model.py), shared by the CPU and the GPU tests and by
tools/choose_filters_when.py: the mixed input of an archive -- text, float32 values, int64 timestamps, noise and an 8-bit greyscale
image, a few blocks of each, and a ragged tail -- and the inputs on which every block is typed with one element size."""
import numpy as np

import byte_delta_inputs as BI
import choose_inputs
import datagen
import series_datagen
import typed_datagen

KINDS = ("text", "float32", "ts64", "noise", "grey8")
GREY_WIDTH = 721


def section(kind, n):
    if kind == "text":
        return np.ascontiguousarray(datagen.text_bytes_fast(n))
    if kind == "float32":
        return np.frombuffer(typed_datagen.typed_bytes("float32", n), np.uint8)
    if kind == "ts64":
        return np.ascontiguousarray(series_datagen.series_bytes("ts64", n))
    if kind == "noise":
        return np.ascontiguousarray(choose_inputs.block("noise", n, 0xc1a55))
    assert kind == "grey8"
    return BI.grey8(n, GREY_WIDTH)


def mixed(block_len, counts=(3, 3, 3, 3, 3), tail=1235):
    """counts[i] blocks of KINDS[i], in that order, and `tail` bytes of text behind them"""
    parts = [section(k, c * block_len) for k, c in zip(KINDS, counts)]
    return np.concatenate(parts + [section("text", tail + 64)[64:]])


def uniform(kind, n):
    """n bytes on which every block is typed with one element size: float32 (4) or ts64 (8)"""
    return section(kind, n)
