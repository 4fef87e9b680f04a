"""Writes tests/golden/container_v4_series.bin: a version-4 container (the filter's delta mode) made by the
Python model, tests/container_model.py, with all three record kinds in it: two frames of 8 and 2 blocks of 4096 bytes and a
ragged tail frame of 1235 bytes (not a multiple of 8), writer plan n = 4096, rows = 8, elem = 8, of int64 timestamps
(tests/series_datagen.py) with a stretch of noise, the codec of each block forced in the cycle BWT, order-0, raw, order-0,
BWT.  python tests/golden/make_container_v4_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import container_model as M  # noqa: E402
import series_datagen  # noqa: E402

BLOCK, ROWS, ELEM = 4096, 8, 8
LENGTH = 10 * BLOCK + 1235
KINDS = (0, 2, 1, 2, 0)


def gold_input():
    x = np.concatenate([series_datagen.series_bytes("ts64", 10 * BLOCK + 1232), np.array([1, 2, 3], np.uint8)])
    x[5 * BLOCK + 3:5 * BLOCK + 900] = np.random.default_rng(2027).integers(0, 256, 897, dtype=np.uint8)
    assert x.size == LENGTH
    return x


def make():
    return M.write(gold_input(), BLOCK, ROWS, ELEM, delta=True, kinds=KINDS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v4_series.bin"), "wb") as f:
        f.write(make())
