"""Writes tests/golden/filter_auto_v10_container.bin: a version-10 container (INTEGRATION.md 4b "filter: auto") made by the Python
model, tests/filter_auto_model.py, under the writer's rule: writer plan n = 16384, rows = 8; the four frames of
tests/filter_auto_inputs.py, four_frames() -- int64 timestamps, text, float32 and a ragged tail of 4999 bytes of uint32
counters -- which the rule gives delta + shuffle 8, no filter, shuffle 4 and delta + shuffle 4.
python tests/golden/make_filter_auto_v10_gold.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import filter_auto_inputs as FI  # noqa: E402
import filter_auto_model as F  # noqa: E402

WORDS = [8 | 1 << 16, 0, 4, 4 | 1 << 16]


def make():
    return F.write(FI.four_frames(), FI.N, FI.ROWS)


if __name__ == "__main__":
    c = make()
    assert F.frame_words(c) == WORDS and len(c) < 300 << 10
    assert F.read(c).tobytes() == FI.four_frames().tobytes()
    with open(os.path.join(HERE, "filter_auto_v10_container.bin"), "wb") as f:
        f.write(c)
