"""Inputs of the auto-mode tests (CPU and GPU) beside ans_inputs.container_input, built in the FILTERED domain like it: a frame
whose blocks are not a multiple of 16 bytes long (so that every block but the first is misaligned and its last chunk is short) and
hold what the refusal cases of sparse_model and ans_model need."""
import numpy as np

import ans_inputs
import auto_model as U
import container_model as M
import sparse_inputs

ODD = 4099                                                      # 64 whole chunks and one of 3 bytes; 65 % 32 != 0


def rows_of(elem):
    return ans_inputs.rows_of(elem)


def skewed(rng, n):
    """94 % zeros, the rest uniform in 1 .. 7: well below Huffman's bit per byte with hardly a chunk of one byte to elide, so
    that rANS wins even in a block of 4099 bytes, where its 64 stored states weigh 256 bytes"""
    return np.where(rng.random(n) < 0.94, 0, rng.integers(1, 8, n)).astype(np.uint8)


def odd_input(elem, delta, n=ODD, tail=777):
    """two frames of blocks of n bytes -- sparse blocks with kept and elided chunks (kind 3; the second with its short last chunk
    kept), skewed blocks (kind 5), a dense block (kind 2), noise (raw) -- and a ragged tail"""
    rows = rows_of(elem)
    fmt = U.stream_format(U.VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert fmt is not None
    rng = np.random.default_rng(900 + elem + (50 if delta else 0))
    nch = (n + 63) // 64
    first = [sparse_inputs.sparse_block(rng, n, 0x10, (3, 4, 5, nch // 2)), skewed(rng, n),
             sparse_inputs.sparse_block(rng, n, 0, (1, 7, nch - 1)), sparse_inputs.dense_block(rng, n)]
    first += [skewed(rng, n) for _ in range(rows - 4)]
    second = [rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 0x33, np.uint8), skewed(rng, n), ans_inputs.segment("all256", n, rng)]
    second += [sparse_inputs.sparse_block(rng, n, 0xFF, range(0, nch, 3)) for _ in range(rows - 4)]
    x = np.concatenate([M.unfilter_frame(np.concatenate(f), fmt) for f in (first, second, [skewed(rng, tail)])])
    x.setflags(write=False)
    return x
