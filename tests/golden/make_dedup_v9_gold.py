"""Writes tests/golden/dedup_v9_container.bin: a version-9 container (the order-0 codec's dedup mode) made by the
Python model, tests/dedup_model.py, under the writer's rule: writer plan n = 246372 (482 chunks, 16 mask words), rows = 3, elem = 8,
delta on; two frames of three blocks and a ragged tail frame of 1636 bytes (tests/dedup_inputs.py, golden_input, says what the
blocks hold).  cases() names the blocks the fixture is there for and is asserted before the file is written.
python tests/golden/make_dedup_v9_gold.py"""
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import container_model as M  # noqa: E402
import dedup_inputs as I  # noqa: E402
import dedup_model as D  # noqa: E402

KINDS = (1, 6, 6, 2, 2, 6, 6)


def make():
    G = I.GOLDEN
    return D.write(I.golden_input(), G["block_len"], G["rows"], G["elem"], G["delta"])


def cases(c):
    """{case: (frame, block)} of what the fixture must hold, found in the container itself"""
    lay = M.layout(c)
    fmt = D.stream_format(*struct.unpack("<HH", c[4:8]), I.GOLDEN["elem"])[0]
    data, pos = D.read(c), 0
    found = {}
    for fi, fr in enumerate(lay["frames"]):
        bl, nch = fr["blk_len"], D.nchunks(fr["blk_len"])
        T, W = D.frame_tables(c, fr)
        f = M.filter_frame(data[pos:pos + fr["nb"] * bl], fmt)
        pos += fr["nb"] * bl
        src = D.map_segments([f[b * bl:(b + 1) * bl] for b in range(fr["nb"])], bl).reshape(fr["nb"], nch)
        sourced = set()
        for b, (s, e, kind) in enumerate(fr["records"]):
            E = int((src[b] != np.arange(b * nch, (b + 1) * nch)).sum())
            if kind == D.DEDUP:
                mask, refs, stream = D.record_parts(c, fr, b)
                kept = D.mask_bits(mask, nch)
                blocks = {int(r) // nch for r in refs}
                sourced |= blocks
                if min(blocks) < b:
                    found.setdefault("sources in an earlier block", (fi, b))
                if blocks == {b} and int(W[T["bwt"] + b]) == b:
                    found.setdefault("sources in itself", (fi, b))
                if not kept.any() and stream.size == 0:
                    found.setdefault("nothing kept", (fi, b))
                if bl % D.CHUNK and not kept[-1]:
                    found.setdefault("short last chunk elided", (fi, b))
            elif kind == M.HUFF0 and E > 0:
                assert 15 * E < D.mask_words(bl)
                found.setdefault("E > 0 stays kind 2", (fi, b))
        for b in sourced:
            if fr["records"][b][2] == M.RAW:
                found.setdefault("raw block is a source", (fi, b))
    return found


WANT = {"sources in an earlier block": (0, 1), "sources in itself": (1, 2), "nothing kept": (0, 2), "short last chunk elided": (0, 1),
        "E > 0 stays kind 2": (1, 1), "raw block is a source": (0, 0)}


if __name__ == "__main__":
    c = make()
    assert cases(c) == WANT, cases(c)
    assert D.read(c, with_kinds=True)[1] == list(KINDS) and len(c) < 400 << 10
    with open(os.path.join(HERE, "dedup_v9_container.bin"), "wb") as f:
        f.write(c)
