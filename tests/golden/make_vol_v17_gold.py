"""Writes tests/golden/vol_v17_container.bin: a version-17 container (INTEGRATION.md 4b "Delta: volume") made by the Python model,
tests/vol_model.py, under the writer's rule: writer plan n = 8192, rows = 3, elem 2, width 20 (period 2048), plane 300 (slab 6144
elements: a full frame is two slabs), fold 1; two frames of 3 blocks and a ragged tail frame of 1235 bytes.  The blocks are laid
out as the FILTERED frames hold them and the input is what the inverse filter makes of those, so that the rule gives a block of
each kind: sparse 3, noise 1, dense 2, skew 5.
python tests/golden/make_vol_v17_gold.py"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import auto_inputs  # noqa: E402
import lag_model  # noqa: E402
import sparse_inputs  # noqa: E402
import vol_model as V  # noqa: E402
from ans_inputs import segment  # noqa: E402

BLOCK, ROWS, ELEM, WIDTH, PLANE, FOLD = 8192, 3, 2, 20, 300, 1
LENGTH = 6 * BLOCK + 1235
WANT = (3, 1, 2, 2, 5, 5, 2)                                    # what the container holds
INPUT_CRC = 0xc6594b87                                         # zlib.crc32 of gold_input()


def filtered_blocks():
    rng = np.random.default_rng(1711)
    return [sparse_inputs.sparse_block(rng, BLOCK, 0x10, (3, 4, 5, 64)), segment("noise", BLOCK, rng), sparse_inputs.dense_block(rng, BLOCK),
            sparse_inputs.dense_block(rng, BLOCK), segment("all256", BLOCK, rng), auto_inputs.skewed(rng, BLOCK),
            auto_inputs.skewed(rng, 1235)]


def gold_input():
    b = filtered_blocks()
    frames = [np.concatenate(b[:3]), np.concatenate(b[3:6]), b[6]]
    x = np.concatenate([V.unvol_delta_unshuffle(f, ELEM, WIDTH, PLANE, FOLD) for f in frames])
    assert x.size == LENGTH
    return x


def make():
    return V.write(gold_input(), BLOCK, ROWS, ELEM, WIDTH, PLANE, FOLD)


if __name__ == "__main__":
    c = make()
    assert tuple(lag_model.kinds_of(c)) == WANT and len(c) < 300 << 10, lag_model.kinds_of(c)
    assert V.read(c).tobytes() == gold_input().tobytes()
    assert V.slab(WIDTH, PLANE) * ELEM < ROWS * BLOCK
    assert zlib.crc32(gold_input().tobytes()) == INPUT_CRC, hex(zlib.crc32(gold_input().tobytes()))
    with open(os.path.join(HERE, "vol_v17_container.bin"), "wb") as f:
        f.write(c)
