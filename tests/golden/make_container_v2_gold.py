"""Writes tests/golden/container_v2_f32.bin: a version-2 BWT container (the byte-plane shuffle filter) made
by the Python model, tests/container_model.py, of a smooth float32 field: 9 blocks of 4096 bytes and a tail of 1235
bytes (not a multiple of 4: its last 3 bytes stay in place), writer plan n = 4096, rows = 4, elem = 4 -- two frames of four
blocks, each block one byte plane (the mantissa planes are raw records, the high planes Huffman ones), a frame of one block
and the tail's frame.  python tests/golden/make_container_v2_gold.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import container_model as M  # noqa: E402
import typed_datagen  # noqa: E402

BLOCK, ROWS, ELEM = 4096, 4, 4
LENGTH = 9 * BLOCK + 1235


def gold_input():
    return typed_datagen.typed_bytes("smooth32", LENGTH, seed=2025)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v2_f32.bin"), "wb") as f:
        f.write(M.write(gold_input(), BLOCK, ROWS, ELEM))
