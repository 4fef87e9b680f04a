"""The "choose-filters: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): the class of one 1 MiB block of each of
the twelve inputs of the "filter: when" table at every level (tests/choose_filters_model.py), and, on the mixed input of
tests/choose_filters_inputs.py at 64 KiB blocks and 4 rows -- three blocks each of text, float32, ts64, noise and an 8-bit greyscale
image, and a tail -- the bytes and the frames of the model's BWT container, its CHOOSE container, the order-0 plan's container at
the settings of every level, and the choose-filters container at every level.

python tools/choose_filters_when.py [--fixture tests/golden/choose_filters_picks.json]

--fixture writes the picks of every frame of the containers at levels 4 and 5 (the grid rule of the models needs minutes on these
frames; tests/test_cpu_choose_filters.py takes the picks from the fixture and checks the rule on smaller inputs)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import choose_filters_inputs as CI  # noqa: E402
import choose_filters_model as CF  # noqa: E402
import choose_model as CM  # noqa: E402
import container_model as M  # noqa: E402
import filter_auto_model as F  # noqa: E402

BLOCK, ROWS = 65536, 4
KEYS = {CF.BWT: "BWT", 0: "order-0", 1: "typed, e = 1", 2: "typed, e = 2", 4: "typed, e = 4", 8: "typed, e = 8"}


def order0_picks(x, level):
    m = {2: CF.F, 3: CF.FL, 4: CF.Q, 5: CF.B}[level]
    return m.picks_of(x, BLOCK, ROWS)


SMALL = {"block_len": 8192, "rows": 8, "counts": [5, 5, 5, 4, 5], "tail": 1235}


def small_case():
    """the picks of the frames of the GPU tests' container (tests/test_gpu_container_choose_filters.py) at levels 4 and 5"""
    x = CI.mixed(SMALL["block_len"], SMALL["counts"], SMALL["tail"])
    out = dict(SMALL)
    for level in (4, 5):
        _, fr, picks = CF.write(x, SMALL["block_len"], SMALL["rows"], level, with_plan=True)
        out["level%d" % level] = {"choose": [list(p) for p in picks], "keys": [k for *_, k in fr]}
    return out


def main():
    fixture = sys.argv[sys.argv.index("--fixture") + 1] if "--fixture" in sys.argv else None
    print("| input, one 1 MiB block | level 0 and 1 | levels 2 to 4 | level 5 |")
    print("|---|---|---|---|")
    for name, v in F.inputs(1 << 20).items():
        k = [CF.key(v, level) for level in range(6)]
        assert k[0] == k[1] and k[2] == k[3] == k[4]
        print("| %s | %s | %s | %s |" % (name, KEYS[k[1]], KEYS[k[2]], KEYS[k[5]]))
    x = CI.mixed(BLOCK)
    print()
    print("| container of the mixed input (%d bytes), n = 64 KiB, rows = 4 | bytes | ratio | frames (BWT + order-0) |" % x.size)
    print("|---|---|---|---|")
    row = lambda name, c, fr: print("| %s | %d | %.3f | %s |" % (name, len(c), x.size / len(c), fr))   # noqa: E731
    row("BWT codec", M.write(x, BLOCK, ROWS, 0, 0), len(F.cut(x.size, BLOCK, ROWS)))
    c0, fr0, _ = CF.write(x, BLOCK, ROWS, 0, with_plan=True)
    row("CHOOSE (level 0)", c0, "%d + %d" % (sum(k == CF.BWT for *_, k in fr0), sum(k != CF.BWT for *_, k in fr0)))
    keep = {"block_len": BLOCK, "rows": ROWS, "bytes": x.size}
    for level in range(1, 6):
        if level == 1:
            o = CF.order0_write(x, BLOCK, ROWS, 1)
        else:
            op = order0_picks(x, level)
            o = {2: CF.F, 3: CF.FL, 4: CF.Q, 5: CF.B}[level].write(x, BLOCK, ROWS, op)
        row("order-0 codec at level %d's settings" % level, o, len(F.cut(x.size, BLOCK, ROWS)))
        c, fr, picks = CF.write(x, BLOCK, ROWS, level, with_plan=True)
        assert np.array_equal(CF.read(c, level), x)
        row("choose-filters level %d" % level, c, "%d + %d" % (sum(k == CF.BWT for *_, k in fr), sum(k != CF.BWT for *_, k in fr)))
        if level >= 4:
            keep["level%d" % level] = {"order0": [list(p) for p in op], "choose": [list(p) for p in picks], "keys": [k for *_, k in fr],
                                       "order0_bytes": len(o), "choose_bytes": len(c)}
    keep["choose_bytes"] = len(c0)
    keep["small"] = small_case()
    if fixture:
        with open(fixture, "w") as f:
            json.dump(keep, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
