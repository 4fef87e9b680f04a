"""The "volume: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 512 KiB of each input of
tests/vol_inputs.py (smooth float32 and float64 fields, a field rounded to 1e-2, a clean and a noisy int16 stack, and one series
that is no volume) at each of its (row width, plane stride) pairs, block_len 65536, rows 8, the order-0 codec with the auto mode:
container bytes under the plain delta (tests/auto_model.py, version 8), the delta with the fold (tests/lag_model.py, version 11),
the 2-D predictor with the fold (tests/grid_model.py, version 12) and the 3-D predictor with the fold (tests/vol_model.py, version
17), the last two at the same row width.

python tools/vol_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import auto_model as U  # noqa: E402
import grid_model as G  # noqa: E402
import lag_model as L  # noqa: E402
import vol_inputs as VI  # noqa: E402
import vol_model as V  # noqa: E402

BLOCK, ROWS = 65536, 8


def sizes(x, elem, width, plane, block=BLOCK, rows=ROWS):
    """container bytes of x under (delta, delta + fold, grid + fold, volume + fold)"""
    c = V.write(x, block, rows, elem, width, plane, 1)
    assert np.array_equal(V.read(c), x)
    return len(U.write(x, block, rows, elem, True)), len(L.write(x, block, rows, elem, 1, 1)), len(G.write(x, block, rows, elem, width, 1)), len(c)


def inputs(n):
    """(name, elem, width, plane, bytes): every input at every stride pair"""
    return [(k, e, w, s, VI.vol_bytes(k, n, w, s)) for k, e in VI.KINDS.items() for w, s in VI.STRIDES]


def main():
    print("| input | elem | width | plane | delta (v8) | delta + fold (v11) | grid + fold (v12) | volume + fold (v17) | v12 / v17 |")
    print("|---|" + "---|" * 8)
    for name, e, w, s, x in inputs(BLOCK * ROWS):
        t = sizes(x, e, w, s)
        print("| %s | %d | %d | %d | %d | %d | %d | %d | %.2f |" % ((name, e, w, s) + t + (t[2] / t[3],)))


if __name__ == "__main__":
    main()
