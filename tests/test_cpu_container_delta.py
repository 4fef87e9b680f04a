"""The delta mode of the container's typed-data filter without a GPU: the library exports the new entry points and validates
their arguments before touching a device; the numpy transform of the model (tests/container_model.py) equals a naive
per-element loop and is undone by its inverse; the model of format version 4 round-trips with both codecs, writes versions 1 to 3
unchanged with the delta off, reproduces the golden fixture and refuses what the format forbids; and what the mode is for, as a
condition on the model alone: integer series under the order-0 codec."""
import ctypes as C
import functools
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import container_model as M
import series_datagen
import typed_datagen

READ1, READ2, READ3 = (functools.partial(M.read, max_version=k) for k in (1, 2, 3))   # the readers of the older versions
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v4_series.bin")
NEW = ["glcDeltaShuffleDevice", "glcUndeltaUnshuffleDevice", "glcPlanSetContainerDelta", "glcPlanGetContainerDelta"]
RUN = 2048


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_delta_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS)
    for name in ("container_set_delta", "container_get_delta", "delta_shuffle", "undelta_unshuffle"):
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
            assert L.glcPlanSetContainerDelta(h, on) == HANDLE
        assert L.glcPlanGetContainerDelta(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerDelta(h, None) == HANDLE
    assert d.value == 77
    a, b = 0x100000, 0x900000
    for fn in (L.glcDeltaShuffleDevice, L.glcUndeltaUnshuffleDevice):
        for elem in (0, 1, 3, 5, 16):
            assert fn(a, b, 4096, elem, None) == ILLEGAL            # a bad elem, a zero length included
            assert fn(a, b, 0, elem, None) == ILLEGAL
        for elem in (2, 4, 8):
            assert fn(a, b, 0, elem, None) == glc.CUDPP_SUCCESS     # nothing to do
            assert fn(None, None, 0, elem, None) == glc.CUDPP_SUCCESS
            assert fn(None, b, 64, elem, None) == ILLEGAL and fn(a, None, 64, elem, None) == ILLEGAL
            assert fn(a, a, 64, elem, None) == ILLEGAL              # in place
            assert fn(a, a + 63, 64, elem, None) == ILLEGAL and fn(a + 63, a, 64, elem, None) == ILLEGAL    # overlapping


# --- the transform ---------------------------------------------------------------------------------------------------------
def _naive_forward(x, e):
    x = bytes(x)
    q = len(x) // e
    v = [int.from_bytes(x[i * e:(i + 1) * e], "little") for i in range(q)]
    out = bytearray(len(x))
    for i in range(q):
        d = v[i] if i % RUN == 0 else (v[i] - v[i - 1]) % (1 << (8 * e))
        for j in range(e):
            out[j * q + i] = (d >> (8 * j)) & 255
    out[q * e:] = x[q * e:]
    return bytes(out)


def _naive_inverse(y, e):
    y = bytes(y)
    q = len(y) // e
    out = bytearray(len(y))
    acc = 0
    for i in range(q):
        d = sum(y[j * q + i] << (8 * j) for j in range(e))
        acc = d if i % RUN == 0 else (acc + d) % (1 << (8 * e))
        out[i * e:(i + 1) * e] = acc.to_bytes(e, "little")
    out[q * e:] = y[q * e:]
    return bytes(out)


@pytest.mark.parametrize("e", [2, 4, 8])
def test_numpy_transform_equals_the_naive_loop(e):
    rng = np.random.default_rng(e)
    for n in (0, 1, e - 1, e, e + 1, RUN * e - 1, RUN * e, RUN * e + e + 1, 3 * RUN * e + 5):
        for x in (rng.integers(0, 256, n, dtype=np.uint8), series_datagen.series_bytes({2: "adc16", 4: "ctr32", 8: "ts64"}[e], n + 8)[:n]):
            y = M.delta_shuffle(x, e)
            assert y.tobytes() == _naive_forward(x, e), (e, n)
            assert _naive_inverse(y, e) == x.tobytes(), (e, n)
            assert np.array_equal(M.undelta_unshuffle(y, e), x), (e, n)
    # wrap-around: a descending series, and 0 followed by the maximum
    for x in (np.arange(3000, 0, -1).astype("<u%d" % e).view(np.uint8), np.array([0, (1 << (8 * e)) - 1] * 1500, dtype="<u%d" % e).view(np.uint8)):
        y = M.delta_shuffle(x, e)
        assert y.tobytes() == _naive_forward(x, e) and np.array_equal(M.undelta_unshuffle(y, e), x)


# --- the writer and the reader -------------------------------------------------------------------------------------------
def _data(n, seed, elem):
    if n == 0:
        return np.zeros(0, np.uint8)
    if seed % 2:
        return series_datagen.series_bytes({2: "adc16", 4: "ids32", 8: "ts64"}[elem], n + 8)[:n].copy()
    return typed_datagen.typed_bytes({2: "quant16", 4: "smooth32", 8: "smooth64"}[elem], n, seed=seed)


def _pins():
    """the pins generator (its grid and inputs) and the committed pins"""
    spec = importlib.util.spec_from_file_location("make_container_model_pins",
                                                  os.path.join(ROOT, "tests", "golden", "make_container_model_pins.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g, g.committed()


def test_delta_off_is_versions_1_to_3_byte_for_byte():
    g, pins = _pins()
    x = _data(3 * 4096 + 77, 1, 4)
    for elem in (0, 2, 4, 8):
        for codec in (0, 1):
            c = M.write(x, 4096, 2, elem, codec, delta=False)
            assert c == M.write(x, 4096, 2, elem, codec)
            assert struct.unpack("<HHII", c[4:16]) == ((3 if codec else 2 if elem else 1), 0, 4096, elem)
            assert np.array_equal(M.read(c), x) and np.array_equal(READ3(c), x)
            # ... and is what the models of versions 1 to 3 wrote
            assert g.pin(M.write(g.grid_input(3 * 4096 + 77, elem, False), 4096, 2, elem, codec, False)) == \
                pins["written"][g.grid_name(3 * 4096 + 77, 4096, 2, elem, codec, False)]
    assert M.write(x, 4096, 2, 1) == M.write(x, 4096, 2, 0) and M.write(x, 4096, 2, 1, 1) == M.write(x, 4096, 2, 0, 1)


@pytest.mark.parametrize("bl", [1000, 4096])
@pytest.mark.parametrize("elem", [2, 4, 8])
@pytest.mark.parametrize("codec", [0, 1])
def test_model_round_trip(bl, elem, codec):
    for rows in (1, 3, 8):
        for i, n in enumerate((0, elem - 1, bl, rows * bl + bl + 1 + elem, 2 * rows * bl + bl + 3 * elem + 1)):
            x = _data(n, rows + i, elem)
            c = M.write(x, bl, rows, elem, codec, delta=True)
            assert len(c) % 8 == 0 and len(c) <= M.bound(n, bl)
            assert struct.unpack("<IHHII", c[:16])[1:] == (4, 1, bl, elem) and struct.unpack("<I", c[4:8])[0] == 0x00010004
            assert struct.unpack("<I", c[-8:-4])[0] == zlib.crc32(x.tobytes())       # crc_all: the ORIGINAL input
            data, kinds = M.read(c, with_kinds=True)
            assert np.array_equal(data, x), (bl, rows, elem, codec, n)
            assert set(kinds) <= ({M.RAW, M.HUFF0} if codec else {M.RAW, M.HUFF})
            if n > bl and (n % bl) % elem:                      # a ragged tail that is no whole number of elements: its own frame,
                fr = M.layout(c)["frames"][-1]                   # element numbering restarted
                assert fr["nb"] == 1 and fr["blk_len"] == n % bl
    assert M.write(b"", bl, 2, elem, codec, delta=True)[32:36] == M.MAGIC_END


def test_crc_raw_is_of_the_filtered_frame():
    x = _data(3 * 4096, 1, 4)
    c = M.write(x, 4096, 4, 4, 1, delta=True)
    fr = M.layout(c)["frames"][0]
    T = M.tables_layout(fr["nb"], fr["blk_len"])
    W = np.frombuffer(c[fr["tables"][0]:fr["tables"][0] + 4 * T["words"]], np.uint32)
    f = M.delta_shuffle(x, 4)
    assert [int(W[T["crc_raw"] + b]) for b in range(3)] == [zlib.crc32(f[b * 4096:(b + 1) * 4096].tobytes()) for b in range(3)]


def _refused(reader, c):
    with pytest.raises(M.ContainerError) as e:
        reader(c)
    return e.value.what, e.value.frame, e.value.block


def test_refusal_matrix_of_version_4():
    n, rows, elem = 4096, 2, 4
    x = _data(5 * n + 123, 1, elem)
    for codec in (0, 1):
        c4, c3 = M.write(x, n, rows, elem, codec, delta=True), M.write(x, n, rows, elem, 1)
        for older in (READ1, READ2, READ3):
            assert _refused(older, c4) == (M.STREAM_HEADER, -1, -1)
        cases, lay = M.refusal_cases(c4, c3, elem)
        assert len(cases) >= 17
        for cont, want in cases:
            assert _refused(M.read, cont) == want
        assert (M.with_header(c4, 4, 0, elem), (1, -1, -1)) in cases                # what the version-3 tests build and expect refused
        assert M.with_header(c4, 4, 0, elem)[4:16] == struct.pack("<HHII", 4, 0, n, elem)
        assert _refused(M.read, c4[:lay["frames"][1]["start"] + 40])[0] == M.TRUNCATED
        assert _refused(M.read, c4[:-1])[0] == M.TRUNCATED
        assert np.array_equal(M.read(c4), x)
    # kinds 0, 1 and 2 are all legal in one version-4 frame; kind 3 is not
    c = M.write(x, n, 4, elem, delta=True, kinds=[0, 2, 1, 2])
    data, kinds = M.read(c, with_kinds=True)
    assert np.array_equal(data, x) and {0, 1, 2} <= set(kinds[:4])
    fr = M.layout(c)["frames"][0]
    bad = bytearray(c)
    bad[fr["tables"][0]:fr["tables"][0] + 4] = struct.pack("<I", 3)
    assert _refused(M.read, M.retable(bytes(bad), fr["start"])) == (M.FRAME_TABLE, 0, 0)


def test_golden_fixture_is_what_its_generator_makes():
    spec = importlib.util.spec_from_file_location("make_container_v4_gold", os.path.join(ROOT, "tests", "golden", "make_container_v4_gold.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    gold = open(GOLD, "rb").read()
    x = g.gold_input()
    assert (g.BLOCK, g.ROWS, g.ELEM) == (4096, 8, 8) and x.size % g.ELEM != 0 and x.size % g.BLOCK != 0
    assert len(gold) <= 64 << 10
    assert g.make() == gold
    assert struct.unpack("<HHII", gold[4:16]) == (4, 1, g.BLOCK, g.ELEM)
    data, kinds = M.read(gold, with_kinds=True)
    assert np.array_equal(data, x)
    assert kinds == [0, 2, 1, 2, 0, 0, 2, 1, 2, 0, 0]          # the forced cycle, no block fallen back to raw
    frames = M.layout(gold)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(8, 4096), (2, 4096), (1, 1235)]
    assert _refused(READ3, gold) == (M.STREAM_HEADER, -1, -1)


# --- what the mode is for ----------------------------------------------------------------------------------------------------
MiB = 1 << 20


@pytest.mark.parametrize("kind", series_datagen.KINDS)
def test_order0_with_delta_is_under_three_quarters_of_order0_without(kind):
    """a condition on the model alone: 1 MiB of each series, block_len 65536, rows 4 (8 for ts64), the order-0 codec, framing
    included"""
    x = series_datagen.series_bytes(kind, MiB)
    elem = series_datagen.ELEM[kind]
    rows = 8 if kind == "ts64" else 4
    off = len(M.write(x, 65536, rows, elem, 1))
    on = len(M.write(x, 65536, rows, elem, 1, delta=True))
    print("%s: order-0 container %d bytes with shuffle %d, %d with delta + shuffle: %.3f of it (ratios %.3f, %.3f)"
          % (kind, off, elem, on, on / off, x.size / off, x.size / on))
    assert on < 0.75 * off
