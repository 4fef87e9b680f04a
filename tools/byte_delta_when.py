"""The "bytes: when" table of INTEGRATION.md 4b from the Python models alone (no GPU): 256 KiB of each input of
tests/byte_delta_inputs.py, block_len 65536, rows 4, the order-0 codec with the auto mode: container bytes unfiltered
(tests/auto_model.py, version 8) and under the byte predictor (tests/byte_delta_model.py, version 15) at lag 1, at lag = channels,
and with the row stride under either; "-" where a column does not apply.

python tools/byte_delta_when.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byte_delta_inputs as BI  # noqa: E402
import byte_delta_model as B  # noqa: E402

BLOCK, ROWS = 65536, 4
COLUMNS = ("unfiltered", "1-D, lag 1", "1-D, lag = channels", "2-D: lag 1 + stride", "2-D: lag = channels + stride")


def size(x, lag, stride, block=BLOCK, rows=ROWS):
    c = B.write(x, block, rows, lag, stride)
    assert np.array_equal(B.read(c), x)
    return len(c)


def inputs(n):
    """(name, bytes, channels or 0, row stride or 0)"""
    return [("grey8, width 721, column pattern", BI.grey8(n, 721), 0, 721),
            ("grey8, width 1800, column pattern", BI.grey8(n, 1800), 0, 1800),
            ("grey8, width 640, column pattern", BI.grey8(n, 640), 0, 640),
            ("rgb8, width 427 (stride 1281), column pattern", BI.rgb8(n, 427), 3, 1281),
            ("stereo u8 audio", BI.stereo8(n), 2, 0),
            ("text", BI.text(n), 0, 0),
            ("noise", BI.noise(n), 0, 0)]


def sizes(x, channels, stride):
    """the five columns of a row (None where one does not apply)"""
    return (size(x, 0, 0), size(x, 1, 0), size(x, channels, 0) if channels else None, size(x, 1, stride) if stride else None,
            size(x, channels, stride) if channels and stride else None)


def main():
    print("| input | " + " | ".join(COLUMNS) + " |")
    print("|---|" + "---|" * len(COLUMNS))
    for name, x, ch, stride in inputs(BLOCK * ROWS):
        print("| %s | %s |" % (name, " | ".join("-" if s is None else str(s) for s in sizes(x, ch, stride))))


if __name__ == "__main__":
    main()
