"""The "grid: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 512 KiB of each grid of tests/grid_inputs.py
(the 12-bit image, the float32 field, the int32 2-D walk) at the row widths 1024, 1800 and 721, and of one input that is no grid,
series_datagen's ts64 (at "width" 1024), block_len 65536, rows 8, the order-0 codec with the auto mode: container bytes under the
shuffle alone, the plain delta (tests/auto_model.py, version 8), the delta with the fold (tests/lag_model.py, version 11) and the
2-D predictor with the fold (tests/grid_model.py, version 12).

python tools/grid_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import auto_model as U  # noqa: E402
import grid_inputs as GI  # noqa: E402
import grid_model as G  # noqa: E402
import lag_model as L  # noqa: E402

BLOCK, ROWS = 65536, 8
WIDTHS = (1024, 1800, 721)


def sizes(x, elem, width, block=BLOCK, rows=ROWS):
    """container bytes of x under (no delta, delta, delta + fold, grid + fold)"""
    c = G.write(x, block, rows, elem, width, 1)
    assert np.array_equal(G.read(c), x)
    return len(U.write(x, block, rows, elem, False)), len(U.write(x, block, rows, elem, True)), len(L.write(x, block, rows, elem, 1, 1)), len(c)


def inputs(n):
    """(name, elem, width, bytes): the three grids at the three widths, then the input that is no grid"""
    import series_datagen
    rows = [(k, e, w, GI.grid_bytes(k, n, w)) for k, e in GI.KINDS.items() for w in WIDTHS]
    return rows + [("ts64 (no grid)", 8, 1024, np.ascontiguousarray(series_datagen.series_bytes("ts64", n)))]


def main():
    print("| input | elem | width | no delta (v8) | delta (v8) | delta + fold (v11) | grid + fold (v12) | delta + fold / grid + fold |")
    print("|---|" + "---|" * 7)
    for name, e, w, x in inputs(BLOCK * ROWS):
        s = sizes(x, e, w)
        print("| %s | %d | %d | %d | %d | %d | %d | %.2f |" % ((name, e, w) + s + (s[2] / s[3],)))


if __name__ == "__main__":
    main()
