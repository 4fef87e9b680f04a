"""The runs mode of the container's BWT codec without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the model of the zero-run split, of record kind 4 and of format version 6
(tests/runs_model.py) round-trips, keeps the split's invariants, refuses every violated field check with (2, frame, block), is
refused by readers without the mode, and reproduces the golden fixture."""
import ctypes as C
import importlib.util
import os
import struct

import numpy as np
import pytest

import container_model as M
import runs_inputs as I
import runs_model as R
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v6_runs.bin")
NEW = ["glcZeroRunSplitSegments", "glcZeroRunJoinSegments", "glcPlanSetContainerRuns", "glcPlanGetContainerRuns"]


def _refused(buf, **kw):
    with pytest.raises(M.ContainerError) as e:
        R.read(buf, **kw)
    return e.value.what, e.value.frame, e.value.block


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_runs_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("container_set_runs", "container_get_runs", "zerorun_split_segments", "zerorun_join_segments"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    d = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for on in (0, 1, 2):
            assert L.glcPlanSetContainerRuns(h, on) == HANDLE
        assert L.glcPlanGetContainerRuns(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerRuns(h, None) == HANDLE
    assert d.value == 77
    x, o, n, a, b, la, lb = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
    split, join = L.glcZeroRunSplitSegments, L.glcZeroRunJoinSegments
    assert split(None, None, None, 0, 4096, None, None, None, None, None) == glc.CUDPP_SUCCESS       # nothing to do
    assert join(None, None, None, None, None, None, 0, 4096, None, None) == glc.CUDPP_SUCCESS
    good = [x, o, n, 3, 4096, a, b, la, lb]
    for i in (0, 1, 2, 5, 6, 7, 8):                                # each pointer null in turn
        args = list(good)
        args[i] = None
        assert split(*args, None) == ILLEGAL
    good = [a, b, o, la, lb, n, 3, 4096, x]
    for i in (0, 1, 2, 3, 4, 5, 8):
        args = list(good)
        args[i] = None
        assert join(*args, None) == ILLEGAL
    assert split(x, o, n, 3, 4096, x, b, la, lb, None) == ILLEGAL and split(x, o, n, 3, 4096, a, a, la, lb, None) == ILLEGAL   # equal bases
    assert join(a, b, o, la, lb, n, 3, 4096, a, None) == ILLEGAL and join(a, a, o, la, lb, n, 3, 4096, x, None) == ILLEGAL
    assert split(x, o, n, 3, (1 << 20) + 1, a, b, la, lb, None) == ILLEGAL                            # maxLen too large
    assert join(a, b, o, la, lb, n, 3, (1 << 20) + 1, x, None) == ILLEGAL
    assert split(x, o, n, 1 << 32, 4096, a, b, la, lb, None) == ILLEGAL                               # count too large


# --- split and join ----------------------------------------------------------------------------------------------------
def _naive_split(x):
    A, B, i, n = [], [], 0, len(x)
    while i < n:
        if x[i]:
            A.append(int(x[i]))
            i += 1
            continue
        r = 1
        while i + r < n and x[i + r] == 0 and (i + r) % R.TILE:
            r += 1
        A.append(0)
        B.append(r - 1)
        i += r
    return np.array(A, np.uint8), np.array(B, np.uint8)


@pytest.mark.parametrize("n", I.SPLIT_SIZES)
@pytest.mark.parametrize("density", I.SPLIT_DENSITIES)
def test_split_join_round_trip_and_invariants(n, density):
    x = I.density_segment(n, density)
    A, B = R.split(x)
    if n <= 4096:
        na, nb = _naive_split(x)
        assert np.array_equal(A, na) and np.array_equal(B, nb)
    assert int((A == 0).sum()) == B.size                          # nB = the zeros of A
    assert A.size <= n and B.size <= n
    assert (A.size - B.size) + int((B.astype(np.int64) + 1).sum()) == n
    assert B.size == 0 or int(B.max()) <= 255
    # no run crosses a tile: a run that starts at position p with length r ends at or before the next multiple of 256
    ln = np.ones(A.size, np.int64)
    ln[A == 0] = B.astype(np.int64) + 1
    start = np.cumsum(ln) - ln
    runs = A == 0
    assert bool(((start[runs] % R.TILE) + ln[runs] <= R.TILE).all())
    assert np.array_equal(R.join(A, B, n), x)


def test_join_is_tolerant():
    A = np.array([5, 0, 7, 0, 0, 9], np.uint8)
    assert R.join(A, np.array([2], np.uint8), 12).tolist() == [5, 0, 0, 0, 7, 0, 0, 9, 0, 0, 0, 0]      # too few B: runs of one, zeros behind
    assert R.join(A, np.array([255, 255, 255], np.uint8), 10).tolist() == [5] + [0] * 9                # B overruns n: nothing past it
    assert R.join(np.array([0, 0], np.uint8), np.array([0, 0], np.uint8), 5).tolist() == [0] * 5       # adjacent runs inside a tile
    assert R.join(np.zeros(0, np.uint8), np.zeros(0, np.uint8), 3).tolist() == [0, 0, 0]


# --- the container -----------------------------------------------------------------------------------------------------
def _data(n):
    import datagen
    return np.concatenate([datagen.text_bytes(n // 2, seed=31), np.zeros(n // 8, np.uint8), datagen.log_bytes(n - n // 2 - n // 8, seed=32)])


@pytest.mark.parametrize("block_len", (4096, 1000))
@pytest.mark.parametrize("elem,delta", ((0, False), (4, False), (8, True)))
def test_model_round_trip(block_len, elem, delta):
    x = _data(2 * 3 * block_len + 777)
    c = R.write(x, block_len, 3, elem, delta)
    assert struct.unpack("<HH", c[4:8]) == (6, 1 if delta else 0) and len(c) <= M.bound(x.size, block_len)
    d, kinds = R.read(c, with_kinds=True)
    assert np.array_equal(d, x) and set(kinds) <= {M.RAW, R.RUNS} and R.RUNS in kinds
    assert _refused(c, max_version=5) == (M.STREAM_HEADER, -1, -1)
    assert _refused(c, runs=False) == (M.STREAM_HEADER, -1, -1)
    with pytest.raises(M.ContainerError):
        S.read(c)


def test_the_raw_rule_and_mixed_kinds():
    rng = np.random.default_rng(3)
    x = np.concatenate([_data(4096), rng.integers(0, 256, 4096, dtype=np.uint8), _data(4096), _data(500)])
    d, kinds = R.read(R.write(x, 4096, 2), with_kinds=True)
    assert np.array_equal(d, x) and kinds == [4, 1, 4, 4]
    c = R.write(x, 4096, 2, kinds=(0, 2, 4, 1))
    d, kinds = R.read(c, with_kinds=True)
    assert np.array_equal(d, x) and kinds[0] == 0 and kinds[2] == 4 and kinds[3] == 1


def test_earlier_versions_read_with_the_mode_on_and_version_5_does_not():
    x = _data(3 * 1000 + 10)
    for c in (M.write(x, 1000, 2), M.write(x, 1000, 2, 4), M.write(x, 1000, 2, 0, M.CODEC_HUFF0), M.write(x, 1000, 2, 2, 0, True)):
        assert np.array_equal(R.read(c), x)
    c5 = S.write(x, 1000, 2)
    assert _refused(c5) == (M.STREAM_HEADER, -1, -1)
    assert np.array_equal(R.read(c5, runs=False), x)


@pytest.mark.parametrize("block_len,elem,delta", ((4096, 0, False), (1000, 0, False), (1000, 2, False), (4096, 8, True)))
def test_refusals_of_version_6(block_len, elem, delta):
    x = _data(2 * 3 * block_len + 321)
    c = R.write(x, block_len, 3, elem, delta)
    cases, _ = R.refusal_cases(c, elem)
    names = " ".join(name for name, _, _ in cases)
    assert all("%d:" % k in names for k in range(1, 10))           # every field check has a case
    for name, bad, want in cases:
        assert _refused(bad) == want, name


def test_kind_4_under_version_4_and_kind_3_under_version_6_are_frame_table_failures():
    x = _data(3 * 1000)
    c = R.write(x, 1000, 3)
    assert _refused(M.with_header(c, 3, 0, 0)) == (M.FRAME_TABLE, 0, 0)
    c4 = R.write(x, 1000, 3, 4, True)
    assert _refused(M.with_header(c4, 4, 1, 4)) == (M.FRAME_TABLE, 0, 0)
    c5 = S.write(np.zeros(3000, np.uint8), 1000, 3, kinds=(3,))
    assert _refused(M.with_header(c5, 6, 0, 0)) == (M.FRAME_TABLE, 0, 0)


# --- the golden fixture ------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_container_v6_gold", os.path.join(ROOT, "tests", "golden", "make_container_v6_gold.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def test_golden_fixture_is_what_its_generator_makes():
    g = _generator()
    c = open(GOLD, "rb").read()
    assert c == g.make() and len(c) < 16384
    d, kinds = R.read(c, with_kinds=True)
    assert np.array_equal(d, g.gold_input()) and kinds == list(g.KINDS) and set(kinds) == {0, 1, 2, 4}
    lay = M.layout(c)
    assert [(f["nb"], f["blk_len"]) for f in lay["frames"]] == [(4, 1024), (2, 1024), (1, 333)]
    s, e, kind = lay["frames"][2]["records"][0]
    assert kind == R.RUNS and struct.unpack("<I", c[s:s + 4])[0] == 0          # nB = 0: no pairs, no stream of B
    A, B = R.split(M.O.mtf(M.O.bwt(I.NO_ZERO_BLOCK)[0]))
    assert B.size == 0 and A.size == I.NO_ZERO_BLOCK.size
    s, e, kind = lay["frames"][1]["records"][1]                                # the block of one repeated byte
    assert kind == R.RUNS and struct.unpack("<3I", c[s:s + 12]) == (2, (254 << 24) | 1, (255 << 24) | 3)
