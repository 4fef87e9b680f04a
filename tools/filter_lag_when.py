"""The "filter-lag: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 256 KiB of each of the twelve inputs of
filter_auto_model.inputs() and of the interleaved kinds of tests/lag_inputs.py, block_len 65536, rows 4, the order-0 codec with the
auto mode: what filter-auto picks and writes (tests/filter_auto_model.py, version 10) and what filter-auto with lag picks and writes
(tests/filter_lag_model.py, version 13), the pick of the first frame and the container bytes.

python tools/filter_lag_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filter_auto_model as F  # noqa: E402
import filter_lag_model as FL  # noqa: E402
import lag_inputs as LI  # noqa: E402

BLOCK, ROWS = 65536, 4


def name_of(cand):
    e, d, l, f = cand
    if e == 1:
        return "none"
    return "(%d)" % e if not d else "(%d, delta)" % e if (l, f) == (1, 0) else "(%d, lag %d, fold)" % (e, l)


def main():
    n = BLOCK * ROWS
    inputs = {k: LI.lag_bytes(k, n) for k in LI.KINDS}
    inputs.update(F.inputs(n))
    print("| input | v10 pick | v10 bytes | v13 pick | v13 bytes | v10 / v13 |")
    print("|---|---|---|---|---|---|")
    for name, x in inputs.items():
        p10 = F.picks_of(x, BLOCK, ROWS)
        p13 = FL.picks_of(x, BLOCK, ROWS)
        c10, c13 = F.write(x, BLOCK, ROWS, picks=p10), FL.write(x, BLOCK, ROWS, picks=p13)
        assert np.array_equal(FL.read(c13), x) and len(c13) <= len(c10)
        e, d = F.CANDS[p10[0]]
        print("| %s | %s | %d | %s | %d | %.3f |" % (name, name_of((e, d, 1, 0)), len(c10), name_of(p13[0]), len(c13), len(c10) / len(c13)))


if __name__ == "__main__":
    main()
