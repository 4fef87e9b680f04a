"""The "dedup: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 2 MiB of each input of tests/dedup_inputs.py
(1 MiB of `shifted`, which stays below the 512 pages where its repeats start to line up), block_len 65536, rows 16 -- so a frame,
the window, is 1 MiB -- no filter, under the plain order-0 codec (tests/container_model.py, format version 3), its sparse mode
(tests/sparse_model.py, version 5), its auto mode (tests/auto_model.py, version 8) and its dedup mode (tests/dedup_model.py,
version 9); ratio = input bytes / container bytes, framing included.

python tools/dedup_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import auto_model as U  # noqa: E402
import container_model as M  # noqa: E402
import dedup_inputs as I  # noqa: E402
import dedup_model as D  # noqa: E402
import sparse_model as S  # noqa: E402

MiB = 1 << 20
BLOCK, ROWS = 65536, 16


def main():
    print("| input | order-0 | sparse | auto | dedup | kind-6 blocks | chunks elided |")
    print("|---|---|---|---|---|---|---|")
    for name in I.NAMES:
        x = I.make(name, MiB if name == "shifted" else 2 * MiB)
        plain = len(M.write(x, BLOCK, ROWS, 0, 1))
        sparse = len(S.write(x, BLOCK, ROWS))
        auto = len(U.write(x, BLOCK, ROWS))
        c = D.write(x, BLOCK, ROWS)
        assert np.array_equal(D.read(c), x)
        kinds, elided = [], 0
        for fr in M.layout(c)["frames"]:
            for b, (_, _, k) in enumerate(fr["records"]):
                kinds.append(k)
                if k == D.DEDUP:
                    elided += D.record_parts(c, fr, b)[1].size
        print("| %s | %.3f | %.3f | %.3f | %.3f | %d of %d | %d of %d |" % (name, x.size / plain, x.size / sparse, x.size / auto, x.size / len(c),
                                                                        kinds.count(D.DEDUP), len(kinds), elided, (x.size + 511) // 512))


if __name__ == "__main__":
    main()
