"""The "auto: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 1 MiB of each input of tools/ans_when.py,
block_len 65536, rows 8 for elem 8 and otherwise 4, the order-0 codec with the sparse mode (tests/sparse_model.py, version 5), with
the rANS mode (tests/ans_model.py, version 7), with the auto mode (tests/auto_model.py, version 8), and the smallest container any
choice of kind per block could give; ratio = input bytes / container bytes, framing included.

python tools/auto_when.py"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ans_model as A  # noqa: E402
import auto_model as U  # noqa: E402
import container_model as M  # noqa: E402
import sparse_model as S  # noqa: E402


def inputs():
    spec = importlib.util.spec_from_file_location("ans_when", os.path.join(ROOT, "tools", "ans_when.py"))
    aw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aw)
    return aw.inputs()


def records(c):
    return [(e - s, k) for f in M.layout(c)["frames"] for s, e, k in f["records"]]


def rows_of(x, elem, delta):
    """(bytes of the three containers, the per-block minimum, the auto container's kinds)"""
    rows = 8 if elem == 8 else 4
    sp, an, au = (m.write(x, 65536, rows, elem, delta) for m in (S, A, U))
    assert np.array_equal(U.read(au), x)
    best = len(sp) - sum(a - min(a, b) for (a, _), (b, _) in zip(records(sp), records(an)))
    return len(sp), len(an), len(au), best, [k for _, k in records(au)]


def main():
    print("| input (filter) | sparse (v5) | rANS (v7) | auto (v8) | per-block minimum | kinds 1 / 2 / 3 / 5 of 16 |")
    print("|---|---|---|---|---|---|")
    for name, filt, x, elem, delta in inputs():
        sp, an, au, best, kinds = rows_of(x, elem, delta)
        print("| %s (%s) | %.3f | %.3f | %.3f | %.3f | %s |" % (name, filt, x.size / sp, x.size / an, x.size / au, x.size / best,
                                                                " / ".join(str(kinds.count(k)) for k in (1, 2, 3, 5))))


if __name__ == "__main__":
    main()
