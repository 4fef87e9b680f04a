"""The container's byte-plane shuffle filter without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the Python model of format version 2 (tests/container_model.py) shuffles and
unshuffles, writes version 1 unchanged with the filter off, round-trips with it on, is refused by the version-1 reader, refuses
what the format forbids, and reproduces the golden fixture; and the filter does what it is for on float32 data."""
import ctypes as C
import functools
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import container_model as M
import datagen
import typed_datagen

READ1, READ2, READ3 = (functools.partial(M.read, max_version=k) for k in (1, 2, 3))   # the readers of the older versions
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v2_f32.bin")
NEW = ["glcShuffleSegments", "glcUnshuffleSegments", "glcShuffleDevice", "glcUnshuffleDevice", "glcPlanSetContainerShuffle",
       "glcPlanGetContainerShuffle"]


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_filter_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS)
    for name in ("container_set_shuffle", "container_get_shuffle", "shuffle", "unshuffle", "shuffle_segments"):
        assert callable(getattr(glc, name))


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE, OK = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE, glc.CUDPP_SUCCESS
    e = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        assert L.glcPlanSetContainerShuffle(h, 4) == HANDLE
        assert L.glcPlanGetContainerShuffle(h, C.byref(e)) == HANDLE
    assert e.value == 77
    a, b = 0x100000, 0x200000
    for fn in (L.glcShuffleDevice, L.glcUnshuffleDevice):
        for elem in (0, 1, 3, 5, 6, 16):
            assert fn(a, b, 4096, elem, None) == ILLEGAL, elem
        assert fn(a, b, 0, 4, None) == OK                       # nothing to do
        assert fn(None, b, 16, 4, None) == ILLEGAL and fn(a, None, 16, 4, None) == ILLEGAL
        assert fn(a, a, 16, 4, None) == ILLEGAL                 # in place
        assert fn(a, a + 15, 16, 4, None) == ILLEGAL and fn(a + 15, a, 16, 4, None) == ILLEGAL
        assert fn(a, a + 4096, 4097, 2, None) == ILLEGAL
    for fn in (L.glcShuffleSegments, L.glcUnshuffleSegments):
        assert fn(a, b, 0x300000, 0x400000, 3, 3, None) == ILLEGAL
        assert fn(a, b, 0x300000, 0x400000, 0, 4, None) == OK
        assert fn(a, a, 0x300000, 0x400000, 3, 4, None) == ILLEGAL
        assert fn(a, b, None, 0x400000, 3, 4, None) == ILLEGAL and fn(a, b, 0x300000, None, 3, 4, None) == ILLEGAL
        assert fn(None, b, 0x300000, 0x400000, 3, 4, None) == ILLEGAL


# --- shuffle / unshuffle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_model_shuffle_is_the_stated_permutation_and_inverts(elem):
    rng = np.random.default_rng(elem)
    for n in (0, 1, elem - 1, elem, elem + 1, 4099, 65536):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        y = M.shuffle(x, elem)
        q, m = n // elem, n - n % elem
        assert y.size == n
        for j in range(elem):                                  # out[j q + i] = in[i elem + j]
            assert np.array_equal(y[j * q:(j + 1) * q], x[j:m:elem]), (n, j)
        assert np.array_equal(y[m:], x[m:])                    # the tail stays in place
        assert np.array_equal(M.unshuffle(y, elem), x), n


# --- the writer and the reader -------------------------------------------------------------------------------------------
def _data(n, seed, elem):
    kind = {2: "quant16", 4: "smooth32", 8: "smooth64"}[elem] if seed % 2 else "float32"
    return typed_datagen.typed_bytes(kind, n, seed=seed) if n else np.zeros(0, np.uint8)


def _pins():
    """the pins generator (its grid and inputs) and the committed pins"""
    spec = importlib.util.spec_from_file_location("make_container_model_pins",
                                                  os.path.join(ROOT, "tests", "golden", "make_container_model_pins.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g, g.committed()


def test_filter_off_is_version_1_byte_for_byte():
    g, pins = _pins()
    for n, bl, rows in ((0, 4096, 2), (5, 4096, 1), (3 * 4096 + 77, 4096, 2), (70000, 65536, 4)):
        x = _data(n, 3, 4)
        v1 = M.write(x, bl, rows)
        assert struct.unpack("<HHII", v1[4:16]) == (1, 0, bl, 0)
        for elem in (0, 1):
            assert M.write(x, bl, rows, elem) == v1
        assert np.array_equal(READ2(v1), x)
        for elem in (0, 1):                                    # ... and is what the version-1 model wrote
            assert g.pin(M.write(g.grid_input(n, elem, False), bl, rows, elem)) == pins["written"][g.grid_name(n, bl, rows, elem, 0, False)]


@pytest.mark.parametrize("bl", [1000, 4096, 65536])
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_model_round_trip(bl, elem):
    for rows in (1, 3, 4):
        for i, n in enumerate((0, elem - 1, bl, 2 * rows * bl, rows * bl + bl + 1 + elem, 2 * bl + 3 * elem)):
            x = _data(n, 10 * rows + i, elem)
            c = M.write(x, bl, rows, elem)
            assert len(c) % 8 == 0 and len(c) <= M.bound(n, bl)
            assert struct.unpack("<HHII", c[4:16]) == (2, 0, bl, elem)
            assert struct.unpack("<I", c[-8:-4])[0] == zlib.crc32(x.tobytes())       # crc_all: the ORIGINAL input
            assert np.array_equal(READ2(c), x), (bl, rows, elem, n)


def _refused(reader, c):
    with pytest.raises(M.ContainerError) as e:
        reader(c)
    return e.value.what, e.value.frame, e.value.block


def _with_header(c, version, elem):
    h = c[:4] + struct.pack("<HHII", version, 0, struct.unpack("<I", c[8:12])[0], elem) + c[16:24]
    return h + struct.pack("<II", zlib.crc32(h), 0) + c[32:]


def test_version_1_reader_refuses_version_2_and_the_header_rules():
    x = _data(3 * 4096 + 123, 5, 4)
    c = M.write(x, 4096, 2, 4)
    assert _refused(READ1, c) == (M.STREAM_HEADER, -1, -1)
    for elem in (0, 1, 3, 16):                                 # version 2 names 2, 4 or 8
        assert _refused(READ2, _with_header(c, 2, elem)) == (M.STREAM_HEADER, -1, -1), elem
    v1 = M.write(x, 4096, 2)
    assert _refused(READ2, _with_header(v1, 1, 4)) == (M.STREAM_HEADER, -1, -1)       # version 1 with the word set
    assert _refused(READ2, _with_header(c, 3, 4)) == (M.STREAM_HEADER, -1, -1)
    # a wrong but legal elem passes every per-block check: only crc_all, the CRC of the original bytes, sees it
    assert _refused(READ2, _with_header(c, 2, 2)) == (M.DECODED_CRC, -1, -1)
    lay = M.layout(c)
    s, e, _ = lay["frames"][1]["records"][0]
    b = bytearray(c)
    b[(s + e) // 2] ^= 0x20
    assert _refused(READ2, bytes(b)) == (M.RECORD_CRC, 1, 0)
    assert _refused(READ2, c[:lay["frames"][1]["start"] + 40])[0] == M.TRUNCATED


def test_golden_fixture_is_what_its_generator_makes():
    spec = importlib.util.spec_from_file_location("make_container_v2_gold",
                                                  os.path.join(ROOT, "tests", "golden", "make_container_v2_gold.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    gold = open(GOLD, "rb").read()
    x = g.gold_input()
    assert x.size % g.ELEM != 0 and x.size % g.BLOCK != 0
    assert len(gold) < 64 << 10
    assert M.write(x, g.BLOCK, g.ROWS, g.ELEM) == gold
    data, kinds = READ2(gold, with_kinds=True)
    assert np.array_equal(data, x)
    assert M.HUFF in kinds and M.RAW in kinds and len(kinds) == 10


# --- what the filter is for ------------------------------------------------------------------------------------------------
def test_float32_container_is_smaller_with_the_filter():
    """float32 ~ N(0,1): interleaved, the four bytes of a float look like noise to the sorter and nearly every block is stored
    raw; as planes, the sign-and-exponent plane and the high mantissa plane code well"""
    n = 1 << 20
    x = datagen.float_bytes(n)
    v1, v2 = len(M.write(x, 65536, 4)), len(M.write(x, 65536, 4, 4))
    print("float32 1 MiB, block_len 65536, rows 4: version 1 %d bytes (ratio %.3f), version 2 elem 4 %d bytes (ratio %.3f)"
          % (v1, n / v1, v2, n / v2))
    assert v2 < v1
