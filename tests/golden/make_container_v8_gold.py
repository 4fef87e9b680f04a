"""Writes tests/golden/container_v8_auto.bin: a version-8 container (the order-0 codec's auto mode) made by the
Python model, tests/auto_model.py: two frames of 3 blocks of 8192 bytes and a ragged tail frame of 1235 bytes, writer plan
n = 8192, rows = 3, elem = 8, delta on.  The blocks are laid out as the FILTERED frames hold them and the input is what the inverse
filter makes of those.  Every block's kind is the rule's (a sparse block: 3; noise: 1; a dense block: 2; skew: 5; the short skewed tail: 3) but for the
second, which is forced to kind 0 -- a kind no GPU writer of version 8 makes but every reader of it takes.
python tests/golden/make_container_v8_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import auto_inputs  # noqa: E402
import auto_model as U  # noqa: E402
import container_model as M  # noqa: E402
import datagen  # noqa: E402
import sparse_inputs  # noqa: E402
from ans_inputs import segment  # noqa: E402

BLOCK, ROWS, ELEM = 8192, 3, 8
LENGTH = 6 * BLOCK + 1235
KINDS = ("rule", 0, "rule", "rule", "rule", "rule", "rule")
WANT = (3, 0, 1, 2, 5, 5, 3)                                    # what the container holds


def filtered_blocks():
    rng = np.random.default_rng(2031)
    return [sparse_inputs.sparse_block(rng, BLOCK, 0x10, (3, 4, 5, 64)), datagen.text_bytes(BLOCK, seed=5), segment("noise", BLOCK, rng),
            sparse_inputs.dense_block(rng, BLOCK), segment("all256", BLOCK, rng), auto_inputs.skewed(rng, BLOCK),
            auto_inputs.skewed(rng, 1235)]


def gold_input():
    fmt = U.stream_format(U.VERSION, M.FLAG_DELTA, ELEM)
    b = filtered_blocks()
    frames = [np.concatenate(b[:3]), np.concatenate(b[3:6]), b[6]]
    x = np.concatenate([M.unfilter_frame(f, fmt) for f in frames])
    assert x.size == LENGTH
    return x


def make():
    return U.write(gold_input(), BLOCK, ROWS, ELEM, delta=True, kinds=KINDS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v8_auto.bin"), "wb") as f:
        f.write(make())
