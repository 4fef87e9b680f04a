"""Filter-auto of the container (format version 10) without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the model of version 10 (tests/filter_auto_model.py) picks a filter per frame, round-trips, has
the size of the version-8 stream with the same filters, reproduces the golden fixture, reads the older versions of the order-0
codec and refuses what the format forbids; every other reader refuses version 10; the range model with a filter per frame."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import auto_model as U
import container_model as M
import filter_auto_inputs as FI
import filter_auto_model as F
import range_model
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "filter_auto_v10_container.bin")
NEW = ["glcFilterProbeSegments", "glcPlanSetContainerFilterAuto", "glcPlanGetContainerFilterAuto", "glcContainerLastFilters"]
NONE = (M.STREAM_HEADER, -1, -1)


def _refused(read, cont, **kw):
    with pytest.raises(M.ContainerError) as e:
        read(cont, **kw)
    return e.value.what, e.value.frame, e.value.block


@pytest.fixture(scope="module")
def four():
    x = FI.four_frames()
    return x, F.write(x, FI.N, FI.ROWS)


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("filter_probe_segments", "container_set_filter_auto", "container_get_filter_auto", "container_last_filters"):
        assert callable(getattr(glc, name))
    assert glc.FILTER_CANDS == F.CANDS and glc.FILTER_PROBE_ROWS == F.ROWS and glc.FILTER_PROBE_MAX_LEN == F.MAX_LEN
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW) and "GLC_FILTER_PROBE_MAX_LEN ((size_t)1 << 31)" in decl
    rule = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "filter_rule.h")).read()
    assert "FILTER_MARGIN_NUM = %d, FILTER_MARGIN_DEN = %d;" % (F.MARGIN_NUM, F.MARGIN_DEN) in rule
    internal = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "container_internal.h")).read()
    assert "CT_VERSION_FILTER = %d;" % F.VERSION in internal


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    d = C.c_uint(77)
    out = (C.c_ulonglong * 8)(*([7] * 8))
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for on in (0, 1, 2):
            assert L.glcPlanSetContainerFilterAuto(h, on) == HANDLE
        assert L.glcPlanGetContainerFilterAuto(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerFilterAuto(h, None) == HANDLE
        assert L.glcContainerLastFilters(h, out) == HANDLE and L.glcContainerLastFilters(h, None) == HANDLE
    assert d.value == 77 and list(out) == [7] * 8
    probe = L.glcFilterProbeSegments
    x, o, n, p, c = (0x100000 * k for k in range(1, 6))
    assert probe(None, None, None, 0, 4096, None, None, None) == glc.CUDPP_SUCCESS                 # nothing to do
    good = [x, o, n, 3, 1 << 31, p, c]
    for i in (0, 1, 2, 5, 6):                                    # each pointer null in turn
        args = list(good)
        args[i] = None
        assert probe(*args, None) == ILLEGAL
    for i, v in ((3, (1 << 22) + 1), (4, (1 << 31) + 1), (5, p + 4), (5, p + 8), (6, c + 4), (6, p)):   # too many, too long, misaligned, one array
        args = list(good)
        args[i] = v
        assert probe(*args, None) == ILLEGAL
    assert probe(None, None, None, (1 << 22) + 1, 64, None, None, None) == ILLEGAL


# --- the model of version 10 -------------------------------------------------------------------------------------------------
def test_four_frames_pick_their_own_filters_and_round_trip(four):
    x, c = four
    assert struct.unpack("<HHII", c[4:16]) == (10, 0, FI.N, 0)
    frames = M.layout(c)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(8, FI.N)] * 3 + [(1, 4999)]
    picks = F.picks_of(x, FI.N, FI.ROWS)
    assert [F.CANDS[p] for p in picks] == [(8, 1), (1, 0), (4, 0), (4, 1)] and len(set(picks)) >= 3
    assert F.frame_words(c) == [F.frame_word(p) for p in picks] == [8 | 1 << 16, 0, 4, 4 | 1 << 16]
    assert F.last_filters(picks) == (1, 0, 0, 1, 1, 0, 1, 4)
    back, words = F.read(c, with_filters=True)
    assert np.array_equal(back, x) and words == F.frame_words(c)
    # every frame is the version-8 frame of its bytes under the same filter, but for the word and the table CRC
    pos = 0
    for f, p in zip(frames, picks):
        e, d = F.CANDS[p]
        n = f["nb"] * f["blk_len"]
        v8 = U.write(x[pos:pos + n], FI.N, FI.ROWS, elem=e, delta=bool(d))
        mine = c[f["start"]:f["start"] + len(v8) - 48]
        assert mine[:12] == v8[32:44] and mine[16:24] == v8[48:56] and mine[32:] == v8[64:-16]
        pos += n
    assert len(c) == 48 + sum(len(U.write(x[o:o + nb * bl], FI.N, FI.ROWS, elem=F.CANDS[p][0], delta=bool(F.CANDS[p][1]))) - 48
                              for (o, nb, bl), p in zip(F.cut(x.size, FI.N, FI.ROWS), picks))
    # and smaller than any one filter for the whole stream
    assert len(c) < min(F.fixed_sizes(x, FI.N, FI.ROWS))


def test_forced_picks_and_small_inputs_round_trip():
    x = FI.four_frames()[:3 * FI.N + 77]
    for picks in ([0, 0], [6, 2], [5, 1], [3, 4]):
        c = F.write(x, FI.N, 3, picks=picks)
        back, words = F.read(c, with_filters=True)
        assert np.array_equal(back, x) and words == [F.frame_word(p) for p in picks]
    for n in (0, 1, 7, 8, 9):
        y = x[:n]
        c = F.write(y, FI.N, 3)
        assert np.array_equal(F.read(c), y)
        assert n >= 8 or F.frame_words(c) == [0] * (n > 0)        # (below eight bytes the probe counts nothing: every cost is 0)
    for cand in range(7):
        y = FI.for_candidate(cand)
        assert F.picks_of(y, FI.N, 3) == [cand], cand
        assert np.array_equal(F.read(F.write(y, FI.N, 3)), y)


def test_the_fixture_reads_back(four):
    gold = open(GOLD, "rb").read()
    assert gold == four[1] and len(gold) < 300 << 10
    assert np.array_equal(F.read(gold), four[0])


def test_the_reader_reads_the_older_versions_of_the_order0_codec():
    x = FI.four_frames()[:2 * FI.N + 5]
    older = [M.write(x, FI.N, 2), M.write(x, FI.N, 2, 4), M.write(x, FI.N, 2, 4, 1), M.write(x, FI.N, 2, 8, 1, delta=True),
             S.write(x, FI.N, 2, 8, True), U.write(x, FI.N, 2, 4, True)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4, 5, 8]
    for c in older:
        assert np.array_equal(F.read(c), x)


def test_refusal_cases(four):
    x, c = four
    cases, _ = F.refusal_cases(c)
    assert len(cases) >= 20
    names = [c[0] for c in cases]
    for must in ("version 10 with elem 4 in the stream header", "frame word: elem 3", "frame word: flags 2", "frame word: flags 1 with elem 0",
                 "a non-zero frame word under a version-8 header", "version 11", "version 10 to a reader without the setting: the auto mode's"):
        assert must in names
    for name, cont, want, reads in cases:
        assert _refused(F.read, cont, reads=reads) == want, name
    # version 10 to every reader without the setting: a stream-header failure, as an unknown version is
    for reads in (U.READS_AUTO, frozenset(), frozenset(("sparse",)), frozenset(("ans",))):
        assert _refused(F.read, c, reads=reads) == NONE
    assert _refused(U.read, c) == NONE and _refused(M.read, c) == NONE and _refused(S.read, c) == NONE


def test_range_model_with_a_filter_per_frame(four):
    x, c = four
    frames = [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]]
    words = F.frame_words(c)
    Fr = FI.N * FI.ROWS
    # inside the delta frame: the run's 2048 elements of 8 bytes are one block, in each of the eight planes
    assert F.range_stats(frames, words, 40000, 100) == (1, 8)
    # inside the unfiltered frame: the blocks the bytes lie in
    assert F.range_stats(frames, words, Fr + 20000, 100) == (1, 1) and F.range_stats(frames, words, Fr + FI.N - 1, 2) == (1, 2)
    # across the edge between them
    assert F.range_stats(frames, words, Fr - 10, 20) == (2, 8 + 1)
    # into the tail
    assert F.range_stats(frames, words, 3 * Fr - 5, 4999) == (2, 4 + 1)
    assert F.range_stats(frames, words, 0, x.size) == (4, 25) and F.range_stats(frames, words, x.size, 0) == (0, 0)
    for (nb, bl), w in zip(frames, words):
        for a, b in ((0, 1), (nb * bl - 1, nb * bl), (bl - 3, bl + 3) if nb > 1 else (5, 4000)):
            assert range_model.needed_blocks(5, w >> 16, w & 0xFFFF, nb, bl, a, b) == range_model.needed_blocks_brute(5, w >> 16, w & 0xFFFF, nb, bl, a, b)
