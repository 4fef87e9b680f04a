"""The "lag: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 512 KiB of each input of tests/lag_inputs.py
(the five interleaved kinds, and for the fold alone series_datagen's adc16 and typed_datagen's smooth32), block_len 65536, rows 8,
the order-0 codec with the auto mode: container bytes under the shuffle alone and the plain delta (tests/auto_model.py, version 8),
under the delta with lag = channels and under lag = channels with the fold (tests/lag_model.py, version 11).

python tools/lag_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import auto_model as U  # noqa: E402
import lag_inputs as LI  # noqa: E402
import lag_model as G  # noqa: E402

BLOCK, ROWS = 65536, 8


def main():
    n = BLOCK * ROWS
    print("| input | elem | lag | shuffle only (v8) | plain delta (v8) | lag (v11) | lag + fold (v11) | smallest v8 / lag + fold |")
    print("|---|" + "---|" * 7)
    rows = [(k, e, ch, LI.lag_bytes(k, n)) for k, (e, ch) in LI.KINDS.items()] + [(k, e, 1, LI.fold_bytes(k, n)) for k, e in LI.FOLD_ONLY.items()]
    for name, e, lag, x in rows:
        s0, s1 = len(U.write(x, BLOCK, ROWS, e, False)), len(U.write(x, BLOCK, ROWS, e, True))
        c = G.write(x, BLOCK, ROWS, e, lag, 1)
        assert np.array_equal(G.read(c), x)
        l0 = len(G.write(x, BLOCK, ROWS, e, lag, 0)) if lag > 1 else s1
        print("| %s | %d | %d | %d | %d | %s | %d | %.2f |" % (name, e, lag, s0, s1, "%d" % l0 if lag > 1 else "(the plain delta)", len(c), min(s0, s1) / len(c)))


if __name__ == "__main__":
    main()
