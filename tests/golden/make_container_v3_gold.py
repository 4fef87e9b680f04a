"""Writes tests/golden/container_v3_mixed.bin: a version-3 container (the order-0 Huffman codec) made by the
Python model, tests/container_model.py, with all three record kinds in it: 9 blocks of 4096 bytes and a tail of 1235 bytes
(not a multiple of 4), writer plan n = 4096, rows = 4, elem = 4, of float32 samples whose low mantissa bytes are noise (raw
planes) and whose high bytes code well, the codec of each block forced in the cycle BWT, order-0, raw, BWT, order-0 -- the
mix no GPU writer makes and every reader accepts.  python tests/golden/make_container_v3_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import container_model as M  # noqa: E402
import typed_datagen  # noqa: E402

BLOCK, ROWS, ELEM = 4096, 4, 4
LENGTH = 9 * BLOCK + 1235
KINDS = (0, 2, 1, 0, 2)


def gold_input():
    x = typed_datagen.typed_bytes("smooth32", LENGTH, seed=2026).copy()
    q = LENGTH // 4
    x[:4 * q].reshape(q, 4)[:, 0] = np.random.default_rng(2026).integers(0, 256, q, dtype=np.uint8)   # a noise plane
    return x


def make():
    return M.write(gold_input(), BLOCK, ROWS, ELEM, kinds=KINDS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v3_mixed.bin"), "wb") as f:
        f.write(make())
