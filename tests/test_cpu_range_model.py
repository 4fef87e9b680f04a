"""Range reads without a GPU: the closed form of the blocks a byte range needs (tests/range_model.py, the form the library
computes) equals the brute-force form that follows every byte through the filter, for every legal format; its size for a small
range; and the library exports the new entry points of include/glc_container.h."""
import ctypes
import os

import numpy as np
import pytest

import range_model as R
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gpu-lossless-compression_amd", "libglc_amd.so")
FORMATS = [(v, f, e) for (v, f), (elems, _) in sorted(S.FORMATS.items()) for e in elems]
SHAPES = [(1, 4096), (3, 4096), (8, 4096), (1, 777)]
NEW_SYMBOLS = ["glcContainerIndexDevice", "glcContainerIndex", "glcContainerIndexFile", "glcContainerIndexFree", "glcContainerIndexInfo",
               "glcContainerReadRangeDevice", "glcContainerReadRange", "glcContainerReadRangeFile", "glcContainerLastRangeStats",
               "glcUnshuffleRangeDevice", "glcUndeltaUnshuffleRangeDevice"]


def _ranges(F, elem, seed):
    """about 200 ranges of [0, F): single bytes, the whole frame, ranges that end in the len % elem tail, and random ones"""
    rng = np.random.default_rng(seed)
    out = [(0, F), (0, 1), (F - 1, F)]
    out += [(int(p), int(p) + 1) for p in rng.integers(0, F, 20)]
    tail = F % elem if elem else 0
    for t in range(1, tail + 1):                                 # ends (and starts) inside the tail
        out += [(int(rng.integers(0, F - tail)), F - tail + t), (F - tail + t - 1, F - tail + t), (F - tail, F - tail + t)]
    while len(out) < 200:
        a = int(rng.integers(0, F))
        n = int(rng.integers(1, F - a + 1)) if rng.random() < 0.5 else int(min(F - a, rng.integers(1, 300)))
        out.append((a, a + n))
    return out


def test_the_formats_are_all_of_them():
    assert len(FORMATS) == 1 + 3 + 4 + 3 + 4 + 3 and (5, 1, 8) in FORMATS and (1, 0, 0) in FORMATS


@pytest.mark.parametrize("version,flags,elem", FORMATS)
def test_needed_blocks_equal_the_brute_force_form(version, flags, elem):
    for nb, bl in SHAPES:
        F = nb * bl
        for a, b in _ranges(F, elem, 1000 * version + 100 * flags + 10 * elem + nb):
            want = R.needed_blocks_brute(version, flags, elem, nb, bl, a, b)
            assert R.needed_blocks(version, flags, elem, nb, bl, a, b) == want, (nb, bl, a, b)
            assert want and set(want) <= set(range(nb))
        assert R.needed_blocks(version, flags, elem, nb, bl, 5, 5) == []


def test_the_tail_and_the_run_start_are_where_the_forms_could_differ():
    # 777 = 97 * 8 + 1: byte 776 is the tail; a range inside it needs no element, with or without the delta
    for flags in (0, 1):
        assert R.needed_blocks(5, flags, 8, 1, 777, 776, 777) == [0]
    # 3 blocks of 4096 with elem 8: q = 1536; byte 8 * 1000 = element 1000 lies in planes at j * 1536 + 1000
    assert R.needed_blocks(3, 0, 8, 3, 4096, 8000, 8001) == sorted({(j * 1536 + 1000) // 4096 for j in range(8)})
    # with the delta the run starts at element 0 there: [j q, j q + 1001) of every plane
    assert R.needed_blocks(4, 1, 8, 3, 4096, 8000, 8001) == [0, 1, 2]
    # 8 blocks, elem 2, element 2048 + 5 with the delta: from element 2048 on in both planes
    assert R.needed_blocks(4, 1, 2, 8, 4096, 2 * 2053, 2 * 2053 + 1) == [(2048) // 4096, (16384 + 2048) // 4096]


def test_a_small_range_needs_few_blocks():
    nb, bl = 8, 4096
    rng = np.random.default_rng(5)
    for a in [0, 1, nb * bl - 100] + [int(v) for v in rng.integers(0, nb * bl - 100, 50)]:
        got = R.needed_blocks(5, 1, 8, nb, bl, a, a + 100)
        assert 1 <= len(got) <= 8, (a, got)
    assert len(R.needed_blocks(1, 0, 0, nb, bl, 4000, 4100)) == 2


def test_stats_model():
    frames = [(8, 4096), (8, 4096), (2, 4096), (1, 777)]
    assert R.stats_of(frames, 0, 0, 1, 0, 0) == (0, 0)
    assert R.stats_of(frames, 0, 1, 1, 0, 0) == (1, 1)
    assert R.stats_of(frames, 8 * 4096 - 1, 2, 1, 0, 0) == (2, 2)
    assert R.stats_of(frames, 0, 18 * 4096 + 777, 3, 0, 4) == (4, 19)


def test_library_exports_the_range_entry_points():
    if not os.path.exists(LIB):
        pytest.skip("the library is not built")
    L = ctypes.CDLL(LIB)
    assert [n for n in NEW_SYMBOLS if not hasattr(L, n)] == []
