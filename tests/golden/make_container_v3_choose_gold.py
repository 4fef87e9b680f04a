"""Writes tests/golden/container_v3_choose.bin: a version-3 container as a writer plan with the CHOOSE codec makes it (INTEGRATION.md
4b "choose"), from the Python model tests/choose_model.py: n = 4096, rows = 4, two super-frames of four blocks and a ragged tail of
1235 bytes.  The rule cuts them into frames of 2, 2, 1, 3 and 1 blocks: text (BWT, kind 0), Zipf bytes (order-0, kind 2) and bytes of
a flat histogram (order-0, stored raw: kind 1); the tail of log lines is below the rule's minimum length and so order-0.
python tests/golden/make_container_v3_choose_gold.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import choose_inputs as CI  # noqa: E402
import choose_model as CM  # noqa: E402

BLOCK, ROWS = 4096, 4
LAYOUT = ("text", "text", "zipf", "flat", "zipf", "text", "logs", "text")
TAIL = ("logs", 1235)
WANT_NB = (2, 2, 1, 3, 1)                                       # the frames' block counts
WANT_KINDS = (0, 0, 2, 1, 2, 0, 0, 0, 2)                        # what the container holds


def gold_input():
    return CI.stream(BLOCK, LAYOUT, TAIL, seed=77)


def make():
    return CM.write(gold_input(), BLOCK, ROWS)


if __name__ == "__main__":
    with open(os.path.join(HERE, "container_v3_choose.bin"), "wb") as f:
        f.write(make())
