"""Writes tests/golden/container_v7_ans.bin: a version-7 container (the order-0 codec's rANS mode) made by the
Python model, tests/ans_model.py, with its four legal record kinds in it: two frames of 3 blocks of 8192 bytes and a ragged tail
frame of 1235 bytes, writer plan n = 8192, rows = 3, elem = 8, delta on.  The blocks are laid out as the FILTERED frames hold them
and the input is what the inverse filter makes of those, so that a block can be constant or skewed behind delta + shuffle; the
codec of each block is forced (KINDS).  Among the kind-5 blocks: one of a single repeated byte (64 states and no unit), one with
all 256 symbols under 97 % zeros, whose quantiser takes the R < 0 path, and the tail.
python tests/golden/make_container_v7_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ans_model as A  # noqa: E402
import container_model as M  # noqa: E402
import datagen  # noqa: E402
from ans_inputs import segment  # noqa: E402

BLOCK, ROWS, ELEM = 8192, 3, 8
LENGTH = 6 * BLOCK + 1235
KINDS = (5, 0, 1, 2, 5, 5, 5)


def filtered_blocks():
    rng = np.random.default_rng(2030)
    return [segment("constant", BLOCK, rng), datagen.text_bytes(BLOCK, seed=5), segment("noise", BLOCK, rng),
            segment("geometric", BLOCK, rng), segment("all256", BLOCK, rng), segment("scattered", BLOCK, rng),
            segment("scattered", 1235, rng)]


def gold_input():
    fmt = A.stream_format(A.VERSION, M.FLAG_DELTA, ELEM)
    b = filtered_blocks()
    frames = [np.concatenate(b[:3]), np.concatenate(b[3:6]), b[6]]
    x = np.concatenate([M.unfilter_frame(f, fmt) for f in frames])
    assert x.size == LENGTH
    return x


def make():
    return A.write(gold_input(), BLOCK, ROWS, ELEM, delta=True, kinds=KINDS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v7_ans.bin"), "wb") as f:
        f.write(make())
