"""The "choose: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): the statistic X of the CHOOSE codec's rule
(tests/choose_model.py) on the named inputs at block sizes 64 KiB, 8 KiB and 2 KiB (8 blocks each); two dilution series at 64 KiB
-- text and log lines with a growing share of their bytes replaced by Zipf bytes -- with X and the words of the BWT record and of
the order-0 record per block (4 blocks each, every record under its raw rule); and, over the two series, the total words each
threshold k / 8 on X would have written, against the per-block minimum, beside the share of undiluted text blocks of 2, 4 and 8 KiB
(1 MiB cut into blocks) that the threshold would miss -- each such block costs about a third of its bytes, against the few per cent
a diluted block on the wrong side costs.

python tools/choose_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import choose_inputs as CI  # noqa: E402
import choose_model as CM  # noqa: E402
import container_model as M  # noqa: E402

NAMES = {"text": "text", "logs": "logs", "zipf": "Zipf 1.0", "zipf15": "Zipf 1.5", "noise": "uniform noise", "float": "float_bytes",
         "zeros90": "90 % scattered zeros"}
SHARES = (0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)
BLOCK, PER = 65536, 4


def diluted(kind, share, i):
    """block i of `kind` with `share` of its bytes, at random places, replaced by Zipf bytes"""
    x = CI.block(kind, BLOCK, 11 + i).copy()
    z = CI.block("zipf", BLOCK, 511 + i)
    at = np.random.default_rng(7000 + i).random(BLOCK) < share
    x[at] = z[at]
    return x


def series(kind):
    """[(share, [(X, BWT words, order-0 words)] per block)]"""
    rows = []
    for share in SHARES:
        blocks = []
        for i in range(PER):
            blk = diluted(kind, share, i)
            blocks.append((CM.X(blk), M.encode_block(blk, M.HUFF)[4].size, M.encode_block(blk, M.HUFF0)[4].size))
        rows.append((share, blocks))
    return rows


def main():
    print("| input | block size | X |")
    print("|---|---|---|")
    for kind, name in NAMES.items():
        x = CI.block(kind, 8 * BLOCK, 31)
        for bs in (65536, 8192, 2048):
            v = [CM.X(x[i * BLOCK: i * BLOCK + bs]) for i in range(8)]
            print("| %s | %d KiB | %.3f to %.3f |" % (name, bs >> 10, min(v), max(v)))
    both = {}
    for kind in ("text", "logs"):
        both[kind] = series(kind)
        print()
        print("| %s, share replaced by Zipf bytes | X | BWT words / block | order-0 words / block | BWT / order-0 |" % NAMES[kind])
        print("|---|---|---|---|---|")
        for share, blocks in both[kind]:
            xs, wb, w0 = (np.array(c, dtype=np.float64) for c in zip(*blocks))
            print("| %d %% | %.2f | %.0f | %.0f | %.3f |" % (round(100 * share), xs.mean(), wb.mean(), w0.mean(), wb.sum() / w0.sum()))
    allb = [b for kind in both for _, blocks in both[kind] for b in blocks]
    best = sum(min(wb, w0) for _, wb, w0 in allb)
    print()
    text = CI.block("text", 1 << 20, 31)
    small = {bs: np.array([CM.X(text[i:i + bs]) for i in range(0, text.size, bs)]) for bs in (2048, 4096, 8192)}
    print("| threshold on X | total words over the two series | over the per-block minimum | text blocks missed at 2 / 4 / 8 KiB |")
    print("|---|---|---|---|")
    totals = {}
    for k in range(8, 25):
        totals[k] = sum(wb if 8 * x >= k else w0 for x, wb, w0 in allb)       # (X >= k / 8)
        missed = " / ".join("%.1f %%" % (100.0 * float((8 * v < k).mean())) for v in small.values())
        print("| %d / 8 = %.3f%s | %d | %.2f %% | %s |" % (k, k / 8, " (the rule)" if 8 * CM.NUM == k * CM.DEN else "", totals[k],
                                                          100.0 * (totals[k] / best - 1), missed))
    k = min(totals, key=lambda t: (totals[t], t))
    print()
    print("smallest total: %d / 8; the rule's %d / %d writes %.2f %% more than it" % (k, CM.NUM, CM.DEN,
                                                                                      100.0 * (totals[8 * CM.NUM // CM.DEN] / totals[k] - 1)))


if __name__ == "__main__":
    main()
