"""Writes tests/golden/filter_lag_v13_container.bin: a version-13 container (INTEGRATION.md 4b "Filter: auto with lag") made by
the Python model, tests/filter_lag_model.py, under the writer's rule: writer plan n = 8192, rows = 2; the mixed stream of
tests/filter_lag_inputs.py -- six frames of 16 KiB of stereo audio, text, an 8-channel ADC dump, int64 timestamps, xyz points and
float32, which the rule gives (2, lag 2, fold), no filter, (2, lag 8, fold), (8, lag 1, fold), (4, lag 3, fold) and shuffle 4, and
a ragged tail of 3001 bytes of four interleaved int32 counters, (4, lag 4, fold).
python tests/golden/make_filter_lag_v13_gold.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import filter_auto_model as F  # noqa: E402
import filter_lag_inputs as FI  # noqa: E402
import filter_lag_model as FL  # noqa: E402

lagw = lambda elem, lag: elem | (1 | 2 | (lag - 1) << 8) << 16
WORDS = [lagw(2, 2), 0, lagw(2, 8), lagw(8, 1), lagw(4, 3), 4, lagw(4, 4)]


def make():
    return FL.write(FI.mixed_stream(), FI.N, FI.ROWS)


if __name__ == "__main__":
    c = make()
    assert F.frame_words(c) == WORDS and len(c) < 300 << 10
    assert FL.read(c).tobytes() == FI.mixed_stream().tobytes()
    with open(os.path.join(HERE, "filter_lag_v13_container.bin"), "wb") as f:
        f.write(c)
