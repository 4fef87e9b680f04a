"""Inputs of the sparse-mode tests (CPU and GPU), built in the FILTERED domain where a block has to be constant, sparse or dense
behind the plan's filter: the input is what the inverse filter makes of the frame."""
import numpy as np

import container_model as M
import series_datagen
import sparse_model as S

SERIES = {0: "ts64", 2: "adc16", 4: "ctr32", 8: "ts64"}


def sparse_block(rng, n, fill, chunks):
    """n bytes of `fill` with a few bytes of noise in each of the given 64-byte chunks"""
    b = np.full(n, fill, np.uint8)
    for c in chunks:
        lo, hi = 64 * c, min(64 * c + 64, n)
        b[rng.integers(lo, hi, 5)] = rng.integers(0, 256, 5, dtype=np.uint8)
        b[lo] = fill ^ 0x5A                                     # (never all fill)
    return b


def dense_block(rng, n):
    """16 symbols, no chunk of one repeated byte: an order-0 record"""
    return (rng.integers(0, 16, n, dtype=np.uint8) * 3 + 1).astype(np.uint8)


def rows_of(elem):
    return 8 if elem == 8 else 4


def container_input(elem, delta, n=8192, tail=1235):
    """one frame of the element size's series, one of noise (raw), one holding a constant block (klen = 0), a dense block (kind 2)
    and sparse blocks of fill 0x10 and 0xFF, two whole sparse blocks, and `tail` ragged bytes whose short last chunk is kept"""
    rows = rows_of(elem)
    fmt = S.stream_format(S.VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert fmt is not None
    rng = np.random.default_rng(100 + elem + (50 if delta else 0))
    nch = S.nchunks(n)
    third = [np.full(n, 0x07, np.uint8), dense_block(rng, n), sparse_block(rng, n, 0x10, range(1, nch, 5)),
             sparse_block(rng, n, 0xFF, (0, nch - 1))]
    third += [sparse_block(rng, n, 0, range(0, nch, 2)) for _ in range(rows - 4)]       # kept and elided alternating
    two = [sparse_block(rng, n, 0, (3, 4, 5, nch // 2)), sparse_block(rng, n, 0x80, range(nch // 4))]
    rag = sparse_block(rng, tail, 0, (2, 7, 11))
    rag[-3:] = (1, 2, 3)
    parts = [series_datagen.series_bytes(SERIES[elem], rows * n + 8)[:rows * n],
             rng.integers(0, 256, rows * n, dtype=np.uint8)]
    parts += [M.unfilter_frame(np.concatenate(f), fmt) for f in (third, two, [rag])]
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x
