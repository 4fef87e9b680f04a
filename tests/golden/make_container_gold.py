"""Writes tests/golden/container_v1.bin: a BWT container made by the Python model, tests/container_model.py,
of 3 blocks of 4096 bytes (text, Zipf, random bytes) and a 5-byte tail (a raw record: its Huffman record would not save a
quarter), writer plan n = 4096, rows = 2 -- frames of two and one blocks, then the tail's frame.  python tests/golden/make_container_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import container_model as M  # noqa: E402
import datagen  # noqa: E402

BLOCK, ROWS = 4096, 2


def gold_input():
    rng = np.random.default_rng(2024)
    return np.concatenate([datagen.text_bytes(BLOCK, seed=5), datagen.zipf_bytes(BLOCK, seed=6),
                           rng.integers(0, 256, BLOCK, dtype=np.uint8), rng.integers(0, 256, 5, dtype=np.uint8)])


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v1.bin"), "wb") as f:
        f.write(M.write(gold_input(), BLOCK, ROWS))
