"""The "ans: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 1 MiB of each input of tools/sparse_when.py,
of scattered skew (90 % zeros, the rest uniform in 1 .. 15) and of the Zipf bytes of the benchmark's configs[1], block_len 65536,
rows 8 for elem 8 and otherwise 4, the order-0 codec alone (tests/container_model.py, format version 3 / 4), with the sparse mode
(tests/sparse_model.py, version 5) and with the rANS mode (tests/ans_model.py, version 7); ratio = input bytes / container
bytes, framing included.

python tools/ans_when.py"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ans_inputs  # noqa: E402
import ans_model as A  # noqa: E402
import container_model as M  # noqa: E402
import datagen  # noqa: E402
import sparse_model as S  # noqa: E402

MiB = 1 << 20


def inputs():
    spec = importlib.util.spec_from_file_location("sparse_when", os.path.join(ROOT, "tools", "sparse_when.py"))
    sw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sw)
    out = sw.inputs()
    out.append(("scattered 90 % zeros, rest uniform in 1..15", "no filter", ans_inputs.segment("scattered", MiB, np.random.default_rng(2031)), 0, False))
    out.append(("Zipf bytes (configs[1])", "no filter", datagen.zipf_bytes(MiB), 0, False))
    return out


def main():
    print("| input (filter) | order-0 | with the sparse mode | with the rANS mode | kind-5 blocks of 16 |")
    print("|---|---|---|---|---|")
    for name, filt, x, elem, delta in inputs():
        rows = 8 if elem == 8 else 4
        off = len(M.write(x, 65536, rows, elem, 1, delta=delta))
        sp = len(S.write(x, 65536, rows, elem, delta))
        c = A.write(x, 65536, rows, elem, delta)
        assert np.array_equal(A.read(c), x)
        kinds = [k for f in M.layout(c)["frames"] for _, _, k in f["records"]]
        print("| %s (%s) | %.3f | %.3f | %.3f | %d |" % (name, filt, x.size / off, x.size / sp, x.size / len(c), kinds.count(A.ANS)))


if __name__ == "__main__":
    main()
