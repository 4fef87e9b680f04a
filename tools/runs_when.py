"""The "runs: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 1 MiB of each tests/datagen.py input cut
into blocks of 64 KiB and of 1 MiB, the BWT codec's record as it is (kind 0, tests/container_model.py) and with the runs mode
(kind 4, tests/runs_model.py); payload ratio = input bytes / record bytes with the raw rule applied, except for the Zipf line,
which is raw under either and is shown before the raw rule.  bzip2 -9 (Python's bz2, whole blocks) is given for scale.

python tools/runs_when.py"""
import bz2
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import container_model as M  # noqa: E402
import datagen  # noqa: E402
import oracle_lib as O  # noqa: E402
import runs_model as R  # noqa: E402

MiB = 1 << 20


def words_before_the_raw_rule(blk, kind):
    if kind == 0:
        return O.compress(blk)["size"]
    A, B = R.split(O.mtf(O.bwt(blk)[0]))
    return R.runs_words(np.bincount(A, minlength=256).astype(np.uint32), np.bincount(B, minlength=256).astype(np.uint32))


def ratio(x, block_len, kind, raw_rule=True):
    words = 0
    for p in range(0, x.size, block_len):
        blk = x[p:p + block_len]
        w = words_before_the_raw_rule(blk, kind)
        words += M.raw_words(blk.size) if raw_rule and 4 * w >= blk.size else w
    return x.size / (4.0 * words)


def bz(x, block_len):
    return x.size / float(sum(len(bz2.compress(x[p:p + block_len].tobytes(), 9)) for p in range(0, x.size, block_len)))


def main():
    page = datagen.text_bytes(4096, seed=11)
    rows = [("`text_bytes_fast`", datagen.text_bytes_fast(MiB), (65536, MiB), True, True),
            ("`log_bytes`", datagen.log_bytes(MiB), (65536, MiB), True, True),
            ("a 4096-byte text page repeated", np.tile(page, MiB // 4096), (MiB,), True, False),
            ("zeros", np.zeros(MiB, np.uint8), (MiB,), True, False),
            ("`zipf_bytes` (raw under either, shown before the raw rule)", datagen.zipf_bytes(MiB), (MiB,), False, True)]
    print("| input | block | kind 0 | with the runs mode | bzip2 -9 |")
    print("|---|---|---|---|---|")
    for name, x, blocks, raw_rule, with_bz in rows:
        for bl in blocks:
            print("| %s | %s | %.3f | %.3f | %s |" % (name, "1 MiB" if bl == MiB else "%d KiB" % (bl >> 10), ratio(x, bl, 0, raw_rule),
                                                     ratio(x, bl, 4, raw_rule), "%.3f" % bz(x, bl) if with_bz else ""))


if __name__ == "__main__":
    main()
