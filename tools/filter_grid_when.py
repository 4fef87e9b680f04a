"""The "filter-grid: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 256 KiB of the gridded inputs of
tests/grid_inputs.py at several row widths and of some inputs that are no grids, block_len 65536, rows 4, the order-0 codec with the
auto mode: what filter-auto with lag picks and writes (tests/filter_lag_model.py, version 13), what filter-auto with grid picks
and writes (tests/filter_grid_model.py, version 14) and, for the grids, what the plan set by hand to the data's element size and
row width writes (tests/grid_model.py, version 12).  The pick is the first frame's.  A few minutes: the model of the grid probe
walks 65535 widths.

python tools/filter_grid_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filter_auto_model as F  # noqa: E402
import filter_grid_model as Q  # noqa: E402
import filter_lag_model as FL  # noqa: E402
import grid_inputs as GI  # noqa: E402
import grid_model as G  # noqa: E402
import lag_inputs as LI  # noqa: E402

BLOCK, ROWS = 65536, 4
GRIDS = (("img16", 640), ("img16", 1024), ("img16", 4097), ("field32", 1800), ("walk32", 300), ("walk32", 721))
OTHERS = ("adc16x8", "xyz32", "ts64", "float32", "text", "noise")


def name_of(cand):
    e, d, l, f, w = cand
    if w:
        return "(%d, grid %d, fold)" % (e, w)
    if e == 1:
        return "none"
    return "(%d)" % e if not d else "(%d, delta)" % e if (l, f) == (1, 0) else "(%d, lag %d, fold)" % (e, l)


def main():
    n = BLOCK * ROWS
    typed = F.inputs(n)
    inputs = [("%s at %d" % (k, w), GI.grid_bytes(k, n, w), (GI.KINDS[k], w)) for k, w in GRIDS]
    inputs += [(k, LI.lag_bytes(k, n) if k in LI.KINDS else typed[k], None) for k in OTHERS]
    print("| input | v13 pick | v13 bytes | v14 pick | v14 bytes | v13 / v14 | v12 by hand |")
    print("|---|---|---|---|---|---|---|")
    for name, x, hand in inputs:
        p13 = FL.picks_of(x, BLOCK, ROWS)
        p14 = Q.picks_of(x, BLOCK, ROWS)
        c13, c14 = FL.write(x, BLOCK, ROWS, picks=p13), Q.write(x, BLOCK, ROWS, picks=p14)
        assert np.array_equal(Q.read(c14), x) and len(c14) <= len(c13)
        v12 = "%d" % len(G.write(x, BLOCK, ROWS, hand[0], hand[1], 1)) if hand else ""
        print("| %s | %s | %d | %s | %d | %.3f | %s |" % (name, name_of(p13[0] + (0,)), len(c13), name_of(p14[0]), len(c14), len(c13) / len(c14), v12), flush=True)


if __name__ == "__main__":
    main()
