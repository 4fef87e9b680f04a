"""The "sparse: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 1 MiB of each input, block_len 65536,
rows 8 for elem 8 and otherwise 4, the order-0 codec without (tests/container_model.py, format version 3 / 4) and with the sparse
mode (tests/sparse_model.py, version 5); ratio = input bytes / container bytes, framing included.

python tools/sparse_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import container_model as M  # noqa: E402
import series_datagen  # noqa: E402
import sparse_model as S  # noqa: E402

MiB = 1 << 20


def inputs():
    rng = np.random.default_rng(2029)
    out = [(k, "delta + shuffle %d" % series_datagen.ELEM[k], series_datagen.series_bytes(k, MiB), series_datagen.ELEM[k], True)
           for k in ("ts64", "ctr32", "ids32", "adc16")]
    step = (1_700_000_000_000_000 + 1000 * np.arange(MiB // 8, dtype=np.int64)).view(np.uint8)
    out.append(("regular-step int64 timestamps", "delta + shuffle 8", step, 8, True))
    f = np.zeros(MiB // 4, np.float32)
    nz = rng.choice(f.size, f.size // 200, replace=False)
    f[nz] = rng.standard_normal(nz.size).astype(np.float32)
    out.append(("float32 with 0.5 % non-zeros", "no filter", f.view(np.uint8), 0, False))
    mask = np.zeros(MiB, np.uint8)
    for s in rng.integers(0, MiB - 64, 40):
        mask[s:s + rng.integers(1, 64)] = 1
    out.append(("byte mask with 40 short runs per MiB", "no filter", mask, 0, False))
    return out


def main():
    print("| input (filter) | order-0 | with the sparse mode | kind-3 blocks of 16 |")
    print("|---|---|---|---|")
    for name, filt, x, elem, delta in inputs():
        rows = 8 if elem == 8 else 4
        off = len(M.write(x, 65536, rows, elem, 1, delta=delta))
        c = S.write(x, 65536, rows, elem, delta)
        assert np.array_equal(S.read(c), x)
        kinds = [k for f in M.layout(c)["frames"] for _, _, k in f["records"]]
        print("| %s (%s) | %.3f | %.2f | %d |" % (name, filt, x.size / off, x.size / len(c), kinds.count(S.SPARSE)))


if __name__ == "__main__":
    main()
