"""The "filter: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 512 KiB of each of the twelve inputs of
tests/filter_auto_model.py (the four typed kinds, the four integer series, noise, zeros, scattered 90 % zeros, text), block_len
65536, rows 8, the order-0 codec with the auto mode (tests/auto_model.py, version 8) under each of the seven fixed filters, the
candidate the filter rule picks (csrc/filter_rule.h; the margin is --num / --den, 33 / 32 by default), the candidate the minimum of
the costs alone would pick, and the bytes of the filter-auto container (version 10), whose one frame has the pick's filter.  With
--mixed also the four-frame input of tests/filter_auto_inputs.py: every fixed filter against a filter per frame.

python tools/filter_when.py [--num 33] [--den 32] [--mixed]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import filter_auto_inputs as FI  # noqa: E402
import filter_auto_model as F  # noqa: E402

BLOCK, ROWS = 65536, 8


def name_of(cand):
    e, d = F.CANDS[cand]
    return "none" if e == 1 else "%d%s" % (e, " delta" if d else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num", type=int, default=F.MARGIN_NUM)
    ap.add_argument("--den", type=int, default=F.MARGIN_DEN)
    ap.add_argument("--mixed", action="store_true")
    args = ap.parse_args()
    F.MARGIN_NUM, F.MARGIN_DEN = args.num, args.den
    print("| input | " + " | ".join(name_of(c) for c in range(7)) + " | pick (%d / %d) | minimum cost | filter-auto (v10) | over the smallest |"
          % (args.num, args.den))
    print("|---|" + "---|" * 11)
    for name, x in F.inputs(BLOCK * ROWS).items():
        pick, cost = F.rule(x)
        sizes = F.fixed_sizes(x, BLOCK, ROWS)
        c10 = F.write(x, BLOCK, ROWS)
        assert np.array_equal(F.read(c10), x) and len(c10) == sizes[pick]
        print("| %s | %s | %s | %s | %d | %.3f %% |" % (name, " | ".join("%d" % s for s in sizes), name_of(pick), name_of(int(np.argmin(cost))),
                                                        len(c10), 100.0 * (len(c10) - min(sizes)) / min(sizes)))
    if args.mixed:
        x = FI.four_frames()
        sizes = F.fixed_sizes(x, FI.N, FI.ROWS)
        c10 = F.write(x, FI.N, FI.ROWS)
        print("\nfour frames (int64 timestamps, text, float32, a tail of uint32 counters), block_len %d, rows %d:" % (FI.N, FI.ROWS))
        print("| " + " | ".join(name_of(c) for c in range(7)) + " | filter-auto (v10) | picks |")
        print("|" + "---|" * 9)
        print("| %s | %d | %s |" % (" | ".join("%d" % s for s in sizes), len(c10), ", ".join(name_of(p) for p in F.picks_of(x, FI.N, FI.ROWS))))


if __name__ == "__main__":
    main()
