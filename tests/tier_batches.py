"""Blocks that send the suffix sorter down each of its tiers, shared by the tests that need a call in which all of them run
(test_gpu_resume.py, test_gpu_scratch_fill.py, test_gpu_call_history.py).  Pure numpy: no GPU, nothing computed at import."""
import functools

import numpy as np

import datagen


def zero_pages(n, seed):
    x = datagen.zipf_bytes(n, seed=seed).copy()
    for off in (n // 25, n // 3 + 123, n - n // 9):
        x[off:off + 4096] = 0
    return x


def duplicate(n, seed):
    x = datagen.text_bytes(n, seed=seed).copy()
    ln = n // 50
    x[n // 2 + 77:n // 2 + 77 + ln] = x[n // 10:n // 10 + ln]
    return x


def phrase(n, seed):
    x = datagen.text_bytes(n, seed=seed).copy()
    ph = np.random.default_rng(seed).integers(97, 123, 2000, dtype=np.uint8)
    for off in range(5000, n - 2000, 16384):
        x[off:off + 2000] = ph
    return x


def log_runs(n, seed):
    x = datagen.log_bytes(n, seed=seed).copy()
    x[n // 5:n // 5 + 1500] = 32
    x[n - n // 3:n - n // 3 + 9000] = 0
    return x


def tail_run(n, seed):
    """the deep part reaches the end of the block: suffixes shorter than the cap inside a run"""
    x = datagen.text_bytes(n, seed=seed).copy()
    x[n - 3000:] = 65
    return x


GENS = {"zero_pages": zero_pages, "duplicate": duplicate, "phrase": phrase, "log_runs": log_runs, "tail_run": tail_run}

# what glcPlanLastSortStatsEx / glcPlanLastSortResumed report of a call on all_tiers_blocks(1 << 20): flagged are all but the
# Zipf block and the zeros, given up on the six deep ones, and the two periodic blocks take the general sorter from scratch
ALL_TIERS_STATS, ALL_TIERS_RESUMED = (7, 6), 4


def all_tiers_blocks(n):
    """every way a block can go, in one call of nine: bucket sorter, sample sorter, resumed doubling, general sorter from
    scratch (periodic data: the tolerant form gives it up at sampling), the periodic tier, a block of one symbol"""
    return [datagen.zipf_bytes(n, seed=1), duplicate(n, 2), datagen.text_bytes(n, seed=3), phrase(n, 4),
            np.tile(np.frombuffer(b"xy", dtype=np.uint8), n // 2), log_runs(n, 5), np.zeros(n, dtype=np.uint8),
            tail_run(n, 6), np.tile(np.random.default_rng(7).integers(0, 256, 4096, dtype=np.uint8), n // 4096)]


@functools.lru_cache(maxsize=None)
def all_tiers_blocks_1m():
    """all_tiers_blocks(1 << 20), made once per process; callers do not write to the arrays"""
    blocks = all_tiers_blocks(1 << 20)
    for b in blocks:
        b.setflags(write=False)
    return tuple(blocks)


@functools.lru_cache(maxsize=None)
def all_tiers_compressed_1m():
    """the oracle's compress of each block of all_tiers_blocks_1m(), once per process for every module that needs it"""
    import oracle_lib
    return tuple(oracle_lib.compress(b) for b in all_tiers_blocks_1m())
