"""Writes the two fixtures of format version 16 (INTEGRATION.md 4b "Filter: auto with bytes"), both made by the Python model,
tests/filter_byte_model.py:
  filter_byte_v16_container.bin   the container of the mixed stream of tests/filter_byte_inputs.py under the writer's rule: writer
                                  plan n = 65536, rows = 4; six frames of 256 KiB -- a greyscale image 721 wide, text, an RGB image
                                  427 wide, a 12-bit image 640 wide, 8-bit stereo audio, int64 timestamps -- which the rule gives
                                  byte (1, 721), no filter, byte (3, 1281), the grid filter at (2, 640), byte (2, 0) and
                                  (8, lag 1, fold), and a ragged tail of 3001 bytes of a greyscale image 100 wide
  filter_byte_probe_256k.npz      the model's probe of 256 KiB of the RGB image 427 wide, where Wmax = 65536: "lag_sums" (16),
                                  "stride_sums" (65537), "winners" (2), "rows" (2 x 256) and "costs" (2)
python tests/golden/make_filter_byte_v16_gold.py        (a few minutes)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import filter_auto_model as F  # noqa: E402
import filter_byte_inputs as BFI  # noqa: E402
import filter_byte_model as B  # noqa: E402


def make():
    return B.write(BFI.mixed_stream(), BFI.N, BFI.ROWS)


def make_probe():
    kind, width, n = BFI.PROBE_BIG
    a, S, w, rows, costs = B.probe(BFI.frame_bytes(kind, width, n))
    return dict(lag_sums=np.asarray(a, np.int64), stride_sums=S, winners=np.asarray(w, np.int64), rows=rows, costs=np.asarray(costs, np.int64))


if __name__ == "__main__":
    c = make()
    picks = [B.word_format(w) for w in F.frame_words(c)]
    assert picks[:6] == [p for _, p in BFI.FRAMES] and len(c) < 1 << 20, (picks, len(c))
    assert B.read(c).tobytes() == BFI.mixed_stream().tobytes()
    with open(os.path.join(HERE, "filter_byte_v16_container.bin"), "wb") as f:
        f.write(c)
    np.savez_compressed(os.path.join(HERE, "filter_byte_probe_256k.npz"), **make_probe())
