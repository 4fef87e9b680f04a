"""Writes tests/golden/container_v5_sparse.bin: a version-5 container (the order-0 codec's sparse mode) made by
the Python model, tests/sparse_model.py, with all four record kinds in it: two frames of 8 and 2 blocks of 4096 bytes and a ragged
tail frame of 1235 bytes, writer plan n = 4096, rows = 8, elem = 8, delta on.  The blocks are laid out as the FILTERED frames hold
them and the input is what the inverse filter makes of those, so that a block can be constant or sparse behind delta + shuffle;
the codec of each block is forced (KINDS).  Among the kind-3 blocks: one with nothing kept (klen = 0), one whose fill byte is 0x10,
and the tail, whose short last chunk is kept.  python tests/golden/make_container_v5_gold.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import container_model as M  # noqa: E402
import datagen  # noqa: E402
import sparse_model as S  # noqa: E402
from sparse_inputs import sparse_block  # noqa: E402

BLOCK, ROWS, ELEM = 4096, 8, 8
LENGTH = 10 * BLOCK + 1235
KINDS = (3, 0, 1, 2, 3, 3, 2, 0, 3, 2, 3)


def filtered_blocks():
    rng = np.random.default_rng(2028)
    text = datagen.text_bytes(2 * BLOCK, seed=5)
    small = lambda: rng.integers(0, 16, BLOCK, dtype=np.uint8) * 3 + 1      # 16 symbols, no chunk of one byte: order-0
    tail = sparse_block(rng, 1235, 0, (2, 7, 11))
    tail[-3:] = (1, 2, 3)                                       # the short last chunk is kept
    return [np.zeros(BLOCK, np.uint8), text[:BLOCK], rng.integers(0, 256, BLOCK, dtype=np.uint8), small(),
            sparse_block(rng, BLOCK, 0x10, (0, 5, 6, 40, 63)), sparse_block(rng, BLOCK, 0, range(0, 64, 3)), small(), text[BLOCK:],
            sparse_block(rng, BLOCK, 0xFF, (1, 62)), small(), tail]


def gold_input():
    fmt = S.stream_format(S.VERSION, M.FLAG_DELTA, ELEM)
    b = filtered_blocks()
    frames = [np.concatenate(b[:8]), np.concatenate(b[8:10]), b[10]]
    x = np.concatenate([M.unfilter_frame(f, fmt) for f in frames])
    assert x.size == LENGTH
    return x


def make():
    return S.write(gold_input(), BLOCK, ROWS, ELEM, delta=True, kinds=KINDS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v5_sparse.bin"), "wb") as f:
        f.write(make())
