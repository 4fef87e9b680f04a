"""The "filter-bytes: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 256 KiB of the seven inputs of
tests/byte_delta_inputs.py and of the twelve of the filter-grid table, block_len 65536, rows 4, the order-0 codec with the auto
mode: what filter-auto with grid picks and writes (tests/filter_grid_model.py, version 14), what filter-auto with bytes picks and
writes (tests/filter_byte_model.py, version 16) and, for the 8-bit samples, what the byte-delta plan set by hand to the data's
channel count and row stride writes (tests/byte_delta_model.py, version 15).  The pick is the first frame's.  About five minutes:
the models of the grid and byte probes walk 65535 widths.  --small: 32 KiB as one frame of 4 x 8192, what
tests/test_cpu_container_filter_byte.py checks.

python tools/filter_byte_when.py [--small]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_delta_inputs as BI  # noqa: E402
import byte_delta_model as BD  # noqa: E402
import filter_auto_model as F  # noqa: E402
import filter_byte_model as B  # noqa: E402
import filter_grid_model as Q  # noqa: E402
import grid_inputs as GI  # noqa: E402
import lag_inputs as LI  # noqa: E402

BLOCK, ROWS = 65536, 4
GRIDS = (("img16", 640), ("img16", 1024), ("img16", 4097), ("field32", 1800), ("walk32", 300), ("walk32", 721))
OTHERS = ("adc16x8", "xyz32", "ts64", "float32", "text", "noise")


def name_of(cand):
    e, d, l, f, w = cand
    if B.is_byte(cand):
        return "byte (%d, %d)" % (l, w)
    if w:
        return "(%d, grid %d, fold)" % (e, w)
    if e == 1:
        return "none"
    return "(%d)" % e if not d else "(%d, delta)" % e if (l, f) == (1, 0) else "(%d, lag %d, fold)" % (e, l)


def inputs(n):
    """(name, bytes, (lag, stride) of the byte-delta plan set by hand or None): the seven 8-bit inputs, then the twelve of the
    filter-grid table"""
    typed = F.inputs(n)
    out = [("grey8 at 721", BI.grey8(n, 721), (1, 721)), ("grey8 at 1800", BI.grey8(n, 1800), (1, 1800)), ("grey8 at 640", BI.grey8(n, 640), (1, 640)),
           ("rgb8 at 427", BI.rgb8(n, 427), (3, 1281)), ("stereo8", BI.stereo8(n), (2, 0)), ("text (bytes)", BI.text(n), None),
           ("noise (bytes)", BI.noise(n), None)]
    out += [("%s at %d" % (k, w), GI.grid_bytes(k, n, w), None) for k, w in GRIDS]
    out += [(k, LI.lag_bytes(k, n) if k in LI.KINDS else typed[k], None) for k in OTHERS]
    return out


def row(x, block, rows, hand):
    """(v14 picks, v14 container, v16 picks, v16 container, v15 container or None)"""
    p14, p16 = Q.picks_of(x, block, rows), B.picks_of(x, block, rows)
    c14, c16 = Q.write(x, block, rows, picks=p14), B.write(x, block, rows, picks=p16)
    assert np.array_equal(B.read(c16), x)
    return p14, c14, p16, c16, BD.write(x, block, rows, hand[0], hand[1]) if hand else None


def main():
    small = "--small" in sys.argv
    block, rows = (8192, 4) if small else (BLOCK, ROWS)
    print("| input | v14 pick | v14 bytes | v16 pick | v16 bytes | v14 / v16 | v15 by hand |")
    print("|---|---|---|---|---|---|---|")
    for name, x, hand in inputs(block * rows):
        p14, c14, p16, c16, c15 = row(x, block, rows, hand)
        assert len(c16) <= len(c14), name
        print("| %s | %s | %d | %s | %d | %.3f | %s |" % (name, name_of(p14[0]), len(c14), name_of(p16[0]), len(c16), len(c14) / len(c16),
                                                          "%d" % len(c15) if c15 else ""), flush=True)


if __name__ == "__main__":
    main()
