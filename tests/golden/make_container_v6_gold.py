"""Writes tests/golden/container_v6_runs.bin: a version-6 container (the BWT codec's runs mode) made by the
Python model, tests/runs_model.py, with the four record kinds of version 6 in it: two frames of 4 and 2 blocks of 1024 bytes and
a ragged tail frame of 333 bytes, writer plan n = 1024, rows = 4, no filter.  The codec of each block is forced (KINDS): a text
block as kind 4, one as kind 0, noise (raw), sixteen symbols (order-0); a log block and a block of one repeated byte as kind 4;
and the tail, a kind-4 block whose MTF bytes hold no zero (nB = 0).  python tests/golden/make_container_v6_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import datagen  # noqa: E402
import runs_model as R  # noqa: E402
from runs_inputs import NO_ZERO_BLOCK  # noqa: E402

BLOCK, ROWS = 1024, 4
LENGTH = 6 * BLOCK + NO_ZERO_BLOCK.size
KINDS = (4, 0, 1, 2, 4, 4, 4)


def gold_input():
    rng = np.random.default_rng(2029)
    text = datagen.text_bytes(2 * BLOCK, seed=6)
    x = np.concatenate([text[:BLOCK], text[BLOCK:], rng.integers(0, 256, BLOCK, dtype=np.uint8),
                        rng.integers(0, 16, BLOCK, dtype=np.uint8) * 3 + 1, datagen.log_bytes(BLOCK, seed=7),
                        np.full(BLOCK, 0x41, np.uint8), NO_ZERO_BLOCK]).astype(np.uint8)
    assert x.size == LENGTH
    return x


def make():
    return R.write(gold_input(), BLOCK, ROWS, kinds=KINDS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v6_runs.bin"), "wb") as f:
        f.write(make())
