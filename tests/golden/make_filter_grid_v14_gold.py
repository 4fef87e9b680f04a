"""Writes the two fixtures of format version 14 (INTEGRATION.md 4b "Filter: auto with grid"), both made by the Python model,
tests/filter_grid_model.py:
  filter_grid_v14_container.bin   the container of the mixed stream of tests/filter_grid_inputs.py under the writer's rule: writer
                                  plan n = 65536, rows = 4; five frames of 256 KiB -- a 12-bit image 640 wide, text, an int32 2-D
                                  walk 300 wide, an 8-channel ADC dump, int64 timestamps -- which the rule gives the grid filter at
                                  (2, 640), no filter, the grid filter at (4, 300), (2, lag 8, fold) and (8, lag 1, fold), and a
                                  ragged tail of 3001 bytes of four interleaved int32 counters, (4, lag 4, fold)
  filter_grid_probe_256k.npz      "sums": the 3 * 65537 sums of the model for 256 KiB of the int32 walk 721 wide, where elem 2
                                  reaches Wmax = 65536 (the model needs about ten seconds for them)
python tests/golden/make_filter_grid_v14_gold.py        (about a minute)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import filter_auto_model as F  # noqa: E402
import filter_grid_inputs as QI  # noqa: E402
import filter_grid_model as Q  # noqa: E402
import grid_inputs  # noqa: E402

lagw = lambda elem, lag: elem | (1 | 2 | (lag - 1) << 8) << 16
gridw = lambda elem, width: elem | width << 8 | 1 << 30 | 1 << 31
WORDS = [gridw(2, 640), 0, gridw(4, 300), lagw(2, 8), lagw(8, 1), lagw(4, 4)]


def make():
    return Q.write(QI.mixed_stream(), QI.N, QI.ROWS)


def make_sums():
    kind, width, n = QI.PROBE_BIG
    return Q.sums(grid_inputs.grid_bytes(kind, n, width))


if __name__ == "__main__":
    c = make()
    assert F.frame_words(c) == WORDS and len(c) < 1 << 20, ([hex(w) for w in F.frame_words(c)], len(c))
    assert Q.read(c).tobytes() == QI.mixed_stream().tobytes()
    with open(os.path.join(HERE, "filter_grid_v14_container.bin"), "wb") as f:
        f.write(c)
    np.savez_compressed(os.path.join(HERE, "filter_grid_probe_256k.npz"), sums=make_sums())
