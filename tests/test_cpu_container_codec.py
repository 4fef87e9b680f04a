"""The container's order-0 Huffman codec without a GPU: the library exports the new container and glc_hd.h entry points and
validates their arguments before touching a device; the Python model of format version 3 (tests/container_model.py)
writes versions 1 / 2 unchanged with the BWT codec, round-trips with the order-0 one, writes records that equal the library's
host encoder word for word, is refused by the older readers, refuses what the format forbids, and reproduces the golden
fixture; the kinds and sizes the codec is for, counted on the model."""
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
import hd_table_model as H
import typed_datagen

READ1, READ2, READ3 = (functools.partial(M.read, max_version=k) for k in (1, 2, 3))   # the readers of the older versions
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v3_mixed.bin")
NEW_CONTAINER = ["glcPlanSetContainerCodec", "glcPlanGetContainerCodec"]
NEW_HD = ["glcHdSegmentsWorkBytes", "glcHdSegmentsTablesDevice", "glcHdSegmentsEncodeDevice", "glcHdSegmentsDecodeDevice"]


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_codec_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW_CONTAINER + NEW_HD if not hasattr(L, n)] == []
    assert set(NEW_CONTAINER) <= set(glc.CONTAINER_SYMBOLS) and set(NEW_HD) <= set(glc.HD_SYMBOLS)
    for name in ("container_set_codec", "container_get_codec", "hd_segments_tables", "hd_segments_encode", "hd_segments_decode"):
        assert callable(getattr(glc, name))
    assert (glc.CONTAINER_CODEC_BWT, glc.CONTAINER_CODEC_HUFF0) == (0, 1)
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert "GLC_CONTAINER_CODEC_BWT = 0" in decl and "GLC_CONTAINER_CODEC_HUFF0 = 1" in decl


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    c = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for codec in (0, 1, 2):
            assert L.glcPlanSetContainerCodec(h, codec) == HANDLE
        assert L.glcPlanGetContainerCodec(h, C.byref(c)) == HANDLE and L.glcPlanGetContainerCodec(h, None) == HANDLE
    assert c.value == 77
    assert ILLEGAL == 2
    a = [0x100000 * (i + 1) for i in range(12)]
    MiB = 1 << 20
    assert L.glcHdSegmentsWorkBytes(0, MiB) == 0 or L.glcHdSegmentsWorkBytes(0, MiB) < 4096
    assert L.glcHdSegmentsWorkBytes(4, MiB + 1) == 0            # a larger maxLen is refused
    w64k, w1m = L.glcHdSegmentsWorkBytes(2048, 65536), L.glcHdSegmentsWorkBytes(2048, MiB)
    assert 2048 * 2048 <= w64k < w1m and w1m >= 2048 * 45 * 256 * 48        # the span-function prefixes: 48 B per 128 B of stream
    tables = lambda **k: L.glcHdSegmentsTablesDevice(*[k.get(n, a[i]) for i, n in enumerate(     # noqa: E731
        ("base", "off", "len"))], k.get("count", 3), k.get("max_len", MiB), *[k.get(n, a[3 + i]) for i, n in enumerate(
            ("hist", "lens", "codes", "nunits"))], None)
    assert tables(count=0) == 1 and tables(count=0, base=None, hist=None) == 1      # nothing to do is a success
    assert tables(max_len=MiB + 1) == 0 and tables(count=0, max_len=MiB + 1) == 0
    assert tables(count=(1 << 22) + 1) == 0                     # more segments than one launch takes
    for name in ("base", "off", "len", "hist", "lens", "codes", "nunits"):
        assert tables(**{name: None}) == 0, name

    def encode(**k):
        v = dict(base=a[0], off=a[1], len=a[2], count=3, max_len=MiB, lens=a[3], codes=a[4], nunits=a[5], units=a[6], uoff=a[7],
                 cap=1 << 30, skip=None, work=a[8])
        v.update(k)
        return L.glcHdSegmentsEncodeDevice(v["base"], v["off"], v["len"], v["count"], v["max_len"], v["lens"], v["codes"], v["nunits"],
                                           v["units"], v["uoff"], v["cap"], v["skip"], v["work"], None)
    assert encode(count=0) == 1 and encode(count=0, work=None) == 1
    assert encode(max_len=MiB + 1) == 0 and encode(units=a[6] + 2) == 0             # unaligned units
    for name in ("base", "off", "len", "lens", "codes", "nunits", "units", "uoff", "work"):
        assert encode(**{name: None}) == 0, name

    def decode(**k):
        v = dict(units=a[0], uoff=a[1], nunits=a[2], hist=a[3], out=a[4], ooff=a[5], len=a[6], count=3, max_len=MiB, skip=None, work=a[7])
        v.update(k)
        return L.glcHdSegmentsDecodeDevice(v["units"], v["uoff"], v["nunits"], v["hist"], v["out"], v["ooff"], v["len"], v["count"],
                                           v["max_len"], v["skip"], v["work"], None)
    assert decode(count=0) == 1
    assert decode(max_len=MiB + 1) == 0 and decode(units=a[0] + 1) == 0
    for name in ("units", "uoff", "nunits", "hist", "out", "ooff", "len", "work"):
        assert decode(**{name: None}) == 0, name


# --- the order-0 record ----------------------------------------------------------------------------------------------------
def _record_inputs():
    return [("zipf", datagen.zipf_bytes(20000, seed=3)), ("text", datagen.text_bytes(9000, seed=2)),
            ("one symbol", np.full(5000, 7, np.uint8)), ("two symbols", np.array([1, 2] * 300 + [1], np.uint8)),
            ("all 256 equal", np.arange(256, dtype=np.uint8).repeat(3)), ("one byte", np.array([200], np.uint8))]


def test_model_record_equals_the_host_encoder_word_for_word(glc):
    for name, x in _record_inputs():
        hist, words = M.h0_encode(x)
        lens, codes = glc.hd_build_table(hist)
        assert np.array_equal(glc.hd_encode_host(x, lens, codes), words), name
        mlens, _ = H.build_table(hist)
        bits = int((hist.astype(np.int64) * mlens).sum())
        assert words.size == (bits + 31) // 32 + 1 == M.h0_words(hist) and words[-1] == 0, name
        if bits % 32:
            assert words[-2] & ((1 << (32 - bits % 32)) - 1) == 0, name             # zero bits after the last code
        back, used = M.h0_decode(hist, words, x.size)
        assert np.array_equal(back, x) and used == bits, name
    h, w = M.h0_encode(np.full(5000, 7, np.uint8))
    assert w.size == (5000 + 31) // 32 + 1                      # a one-symbol block: length 1, blk_len bits


# --- the writer and the reader -------------------------------------------------------------------------------------------
def _data(n, seed, elem):
    if n == 0:
        return np.zeros(0, np.uint8)
    if elem == 0:
        return datagen.zipf_bytes(n, seed=seed) if seed % 2 else datagen.text_bytes_fast(n, seed=seed)
    kind = {2: "quant16", 4: "smooth32", 8: "smooth64"}[elem] if seed % 2 else "float32"
    return typed_datagen.typed_bytes(kind, n, seed=seed)


def _pins():
    """the pins generator (its grid and inputs) and the committed pins"""
    spec = importlib.util.spec_from_file_location("make_container_model_pins",
                                                  os.path.join(ROOT, "tests", "golden", "make_container_model_pins.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g, g.committed()


def test_codec_bwt_is_version_1_and_2_byte_for_byte():
    g, pins = _pins()
    for n, bl, rows in ((0, 4096, 2), (5, 4096, 1), (3 * 4096 + 77, 4096, 2), (70000, 65536, 4)):
        x = _data(n, 3, 4)
        for elem in (0, 1, 2, 4, 8):
            c = M.write(x, bl, rows, elem, 0)
            assert struct.unpack("<HHII", c[4:16]) == ((2, 0, bl, elem) if elem > 1 else (1, 0, bl, 0))
            assert np.array_equal(READ3(c), x) and np.array_equal(READ2(c), x)
            # ... and is what the models of versions 1 and 2 wrote
            assert g.pin(M.write(g.grid_input(n, elem, False), bl, rows, elem, 0)) == pins["written"][g.grid_name(n, bl, rows, elem, 0, False)]
        assert M.write(x, bl, rows, 1) == M.write(x, bl, rows, 0) == M.write(x, bl, rows)


@pytest.mark.parametrize("bl", [1000, 4096, 65536])
@pytest.mark.parametrize("elem", [0, 2, 4, 8])
def test_model_round_trip(bl, elem):
    e1 = max(elem, 2)
    for rows in (1, 3, 4):
        for i, n in enumerate((0, e1 - 1, bl, 2 * rows * bl, rows * bl + bl + 1 + e1, 2 * bl + 3 * e1)):
            x = _data(n, 10 * rows + i, elem)
            c = M.write(x, bl, rows, elem, 1)
            assert len(c) % 8 == 0 and len(c) <= M.bound(n, bl)
            assert struct.unpack("<HHII", c[4:16]) == (3, 0, bl, elem)
            assert struct.unpack("<I", c[-8:-4])[0] == zlib.crc32(x.tobytes())       # crc_all: the ORIGINAL input
            data, kinds = READ3(c, with_kinds=True)
            assert np.array_equal(data, x), (bl, rows, elem, n)
            assert set(kinds) <= {M.RAW, M.HUFF0}
    assert M.write(b"", bl, 2, elem, 1)[32:36] == M.MAGIC_END      # an empty input: header + trailer


def test_mixed_kinds_in_one_frame_round_trip():
    x = np.concatenate([datagen.text_bytes(3 * 4096, seed=1), datagen.zipf_bytes(4 * 4096 + 100, seed=2)])
    for elem in (0, 4):
        c = M.write(x, 4096, 4, elem, kinds=[0, 2, 1, 2, 0, 1])
        data, kinds = READ3(c, with_kinds=True)
        assert np.array_equal(data, x) and {0, 1, 2} <= set(kinds[:4])


def _refused(reader, c):
    with pytest.raises(M.ContainerError) as e:
        reader(c)
    return e.value.what, e.value.frame, e.value.block


def test_older_readers_refuse_version_3_and_the_version_3_reader_refuses_what_the_format_forbids():
    n, rows, elem = 4096, 3, 4
    x = np.concatenate([typed_datagen.typed_bytes("smooth32", 5 * n, seed=4), datagen.zipf_bytes(2 * n + 123, seed=4)])
    c = M.write(x, n, rows, elem, 1)
    assert _refused(READ1, c) == (M.STREAM_HEADER, -1, -1)
    assert _refused(READ2, c) == (M.STREAM_HEADER, -1, -1)
    assert _refused(READ2, M.write(x, n, rows, 0, 1)) == (M.STREAM_HEADER, -1, -1)
    cases, lay = M.corrupted_cases(c, x, n, rows, elem)
    whats = set()
    for cont, want in cases:
        assert _refused(READ3, cont) == want
        whats.add(want[0])
    assert whats == {1, 2, 3, 4} and len(cases) >= 13            # one word short and one word long are among them
    assert _refused(READ3, c[:lay["frames"][1]["start"] + 40])[0] == M.TRUNCATED
    assert _refused(READ3, c[:-1])[0] == M.TRUNCATED
    assert np.array_equal(READ3(c), x)


def test_golden_fixture_is_what_its_generator_makes():
    spec = importlib.util.spec_from_file_location("make_container_v3_gold",
                                                  os.path.join(ROOT, "tests", "golden", "make_container_v3_gold.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    gold = open(GOLD, "rb").read()
    x = g.gold_input()
    assert x.size % g.ELEM != 0 and x.size % g.BLOCK != 0
    assert len(gold) < 64 << 10
    assert g.make() == gold
    assert struct.unpack("<HHII", gold[4:16]) == (3, 0, g.BLOCK, g.ELEM)
    data, kinds = READ3(gold, with_kinds=True)
    assert np.array_equal(data, x)
    assert {M.HUFF, M.RAW, M.HUFF0} <= set(kinds) and len(kinds) == 10
    assert _refused(READ2, gold) == (M.STREAM_HEADER, -1, -1)


# --- what the codec is for ---------------------------------------------------------------------------------------------------
MiB = 1 << 20


def _kinds(x, elem, codec=1):
    c = M.write(x, 65536, 4, elem, codec)
    return [k for f in M.layout(c)["frames"] for _, _, k in f["records"]], len(c)


def test_kinds_are_what_the_inputs_were_chosen_for():
    """conditions of the inputs the tests and the bench use, at block_len 65536, rows 4, 1 MiB: 16 blocks each"""
    for name, x, elem in (("zipf", np.asarray(datagen.zipf_philox_bytes(0, MiB), np.uint8), 0),
                          ("text", datagen.text_bytes_fast(MiB, seed=1), 0), ("log", datagen.log_bytes(MiB, seed=1), 0),
                          ("quant16", typed_datagen.typed_bytes("quant16", MiB, seed=1), 2),
                          ("quant16 unfiltered", typed_datagen.typed_bytes("quant16", MiB, seed=1), 0)):
        kinds, _ = _kinds(x, elem)
        assert kinds.count(M.HUFF0) == 16 and kinds.count(M.RAW) == 0, name
    kinds, _ = _kinds(np.random.default_rng(1).integers(0, 256, MiB, dtype=np.uint8), 0)
    assert kinds.count(M.RAW) == 16                              # uniform bytes: every block raw
    kinds, _ = _kinds(typed_datagen.typed_bytes("float32", MiB, seed=1), 4)
    assert kinds.count(M.RAW) == 8 and kinds.count(M.HUFF0) == 8   # float32 N(0,1): the mantissa planes raw, the high planes coded


def test_order0_is_smaller_on_zipf_and_larger_on_text():
    z = np.asarray(datagen.zipf_philox_bytes(0, MiB), np.uint8)
    t = datagen.text_bytes_fast(MiB // 4, seed=1)
    (_, z0), (_, z1) = _kinds(z, 0, 0), _kinds(z, 0, 1)
    (_, t0), (_, t1) = _kinds(t, 0, 0), _kinds(t, 0, 1)
    print("Zipf(1.0) 1 MiB, block_len 65536, rows 4: BWT codec ratio %.3f, order-0 %.3f; text 256 KiB: BWT %.3f, order-0 %.3f"
          % (z.size / z0, z.size / z1, t.size / t0, t.size / t1))
    assert z1 < z0 and t1 > t0
