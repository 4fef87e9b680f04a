"""Inputs of the rANS-mode tests (CPU and GPU).  The segment generators are the shapes the coder can go wrong on; the container
input is built in the FILTERED domain, where a block has to be skewed, constant or noise behind the plan's filter: the input is
what the inverse filter makes of the frame."""
import numpy as np

import ans_model as A
import container_model as M
import series_datagen

SERIES = {0: "ts64", 2: "adc16", 4: "ctr32", 8: "ts64"}
KINDS = ("constant", "noise", "scattered", "dominant", "geometric", "all256")


def segment(kind, n, rng):
    """n bytes: constant; uniform noise; scattered 90 % zeros with the rest uniform in 1..15; one symbol at 99.9 % with the other
    255 rare; geometric; all 256 symbols present under 97 % zeros (with n >= 2^13 the quantiser's sum passes 4096: the R < 0 path)"""
    if kind == "constant":
        return np.full(n, 0x5A, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "scattered":
        return np.where(rng.random(n) < 0.9, 0, rng.integers(1, 16, n)).astype(np.uint8)
    if kind == "dominant":
        return np.where(rng.random(n) < 0.999, 7, rng.integers(0, 256, n)).astype(np.uint8)
    if kind == "geometric":
        return np.minimum(rng.geometric(0.3, n) - 1, 255).astype(np.uint8)
    assert kind == "all256"
    x = np.where(rng.random(n) < 0.97, 0, rng.integers(1, 256, n)).astype(np.uint8)
    if n >= 256:
        x[rng.permutation(n)[:256]] = np.arange(256, dtype=np.uint8)
    return x


def rows_of(elem):
    return 8 if elem == 8 else 4


def container_input(elem, delta, n=70000, tail=1235):
    """one frame of the element size's series, one of a noise block (raw), a constant block, a scattered-skew block and all-256
    blocks (the R < 0 path), and `tail` ragged bytes of scattered skew"""
    rows = rows_of(elem)
    fmt = A.stream_format(A.VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert fmt is not None
    rng = np.random.default_rng(700 + elem + (50 if delta else 0))
    second = [segment("noise", n, rng), segment("constant", n, rng), segment("scattered", n, rng)]
    second += [segment("all256", n, rng) for _ in range(rows - 3)]
    parts = [series_datagen.series_bytes(SERIES[elem], rows * n + 8)[:rows * n]]
    parts += [M.unfilter_frame(np.concatenate(f), fmt) for f in (second, [segment("scattered", tail, rng)])]
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x
