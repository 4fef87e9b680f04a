"""The sparse mode of the container's order-0 codec without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the model of record kind 3 and format version 5 (tests/sparse_model.py) round-trips for every
legal header triple, follows the writer's rule at its boundaries, never makes a block larger than its kind-2 record, is refused by
the readers of version 4, reproduces the golden fixture and refuses what the format forbids; and what the mode is for, as a
condition on the model alone."""
import ctypes as C
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import container_model as M
import series_datagen
import sparse_inputs as I
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v5_sparse.bin")
NEW = ["glcSparseSplitSegments", "glcSparseJoinSegments", "glcPlanSetContainerSparse", "glcPlanGetContainerSparse"]
TRIPLES = [(0, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)]


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_sparse_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS)
    for name in ("container_set_sparse", "container_get_sparse", "sparse_split_segments", "sparse_join_segments"):
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
            assert L.glcPlanSetContainerSparse(h, on) == HANDLE
        assert L.glcPlanGetContainerSparse(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerSparse(h, None) == HANDLE
    assert d.value == 77
    a, b, o, n, f, m, k = 0x100000, 0x900000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    split, join = L.glcSparseSplitSegments, L.glcSparseJoinSegments
    assert split(None, None, None, 0, 4096, None, None, None, None, None) == glc.CUDPP_SUCCESS       # nothing to do
    assert join(None, None, None, 0, 4096, None, None, None, None) == glc.CUDPP_SUCCESS
    good = [a, o, n, 3, 4096, f, m, b, k]
    for i in (0, 1, 2, 5, 6, 7, 8):                                # each pointer null in turn
        args = list(good)
        args[i] = None
        assert split(*args, None) == ILLEGAL
    for i in (0, 1, 2, 5, 6, 7):
        args = list(good[:8])
        args[i] = None
        assert join(*args, None) == ILLEGAL
    assert split(a, o, n, 3, 4096, f, m, a, k, None) == ILLEGAL and join(a, o, n, 3, 4096, f, m, a, None) == ILLEGAL    # in place
    assert split(a, o, n, 3, 4096, f, m + 2, b, k, None) == ILLEGAL and join(a, o, n, 3, 4096, f, m + 1, b, None) == ILLEGAL
    assert split(a, o, n, 3, (1 << 28) + 1, f, m, b, k, None) == ILLEGAL and join(a, o, n, 3, (1 << 28) + 1, f, m, b, None) == ILLEGAL
    assert split(a, o, n, 1 << 32, 4096, f, m, b, k, None) == ILLEGAL and join(a, o, n, 1 << 32, 4096, f, m, b, None) == ILLEGAL


# --- split and join --------------------------------------------------------------------------------------------------------
def _naive_split(blk, fill):
    blk = bytes(blk)
    nch = (len(blk) + 63) // 64
    words, K = [0] * ((nch + 31) // 32), b""
    for c in range(nch):
        chunk = blk[64 * c:64 * c + 64]
        if chunk != bytes([fill]) * len(chunk):
            words[c // 32] |= 1 << (c % 32)
            K += chunk
    return words, K


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 4096 + 77])
def test_split_equals_the_naive_loop_and_join_inverts_it(n):
    rng = np.random.default_rng(n)
    for fill in (0, 0x10, 0xFF):
        for chunks in ((), range(S.nchunks(n)), range(0, S.nchunks(n), 2), (S.nchunks(n) - 1,)):
            blk = I.sparse_block(rng, n, fill, chunks)
            f, mask, K = S.split(blk, fill)
            words, Kn = _naive_split(blk, fill)
            assert (f, mask.tolist(), K.tobytes()) == (fill, words, Kn)
            assert S.klen_of(mask, n) == K.size
            assert np.array_equal(S.join(fill, mask, K, n), blk)
    blk = np.full(n, 9, np.uint8)                                  # a chunk of one repeated non-fill byte is kept
    assert S.split(blk, 0)[2].size == n and S.split(blk, 9)[2].size == 0 and S.split(blk)[0] == 9


# --- the writer's rule -----------------------------------------------------------------------------------------------------
def _block_with_elided(nch, E, rng):
    """nch whole chunks of which exactly E are all zero; the others hold noise from 1..255 around a zero (the fill stays 0)"""
    b = rng.integers(1, 256, nch * 64, dtype=np.uint8)
    b.reshape(nch, 64)[:, ::2] = 0                                 # half of every kept chunk is the fill
    b.reshape(nch, 64)[:E] = 0
    return b


def test_writer_rule_at_its_boundaries():
    rng = np.random.default_rng(7)
    for nch, E, want in ((64, 1, M.HUFF0), (64, 2, S.SPARSE), (65, 2, M.HUFF0), (65, 3, S.SPARSE), (33, 1, M.HUFF0), (32, 1, S.SPARSE),
                         (32, 0, M.HUFF0)):
        blk = _block_with_elided(nch, E, rng)
        assert S.fill_of(blk) == 0 and S.elided(blk) == E
        assert (32 * E >= nch) == (want == S.SPARSE)
        assert S.encode_block(blk, "rule")[0] == want, (nch, E)
    # a tie for the most frequent byte takes the lower value
    tie = np.concatenate([np.full(640, 200, np.uint8), np.full(640, 3, np.uint8), np.arange(256, dtype=np.uint8)])
    assert S.fill_of(tie) == 3
    kind, fill, hist, _, words = S.encode_block(tie, "rule")
    assert (kind, fill) == (S.SPARSE, 3) and int(hist[3]) == 1 and int(hist[200]) == 641 and int(hist.sum()) == 640 + 256
    # a chunk of one repeated non-fill byte is kept
    blk = np.zeros(4096, np.uint8)
    blk[128:192] = 0x33
    blk[1000] = 1
    fill, mask, K = S.split(blk)
    assert fill == 0 and mask.tolist() == [(1 << 2) | (1 << 15), 0] and K[:64].tobytes() == b"\x33" * 64
    # hist of K = hist of the block with the elided bytes taken off the fill's count
    hk = np.bincount(K, minlength=256)
    hb = np.bincount(blk, minlength=256)
    hb[fill] -= blk.size - K.size
    assert np.array_equal(hk, hb)
    # nothing kept: the record is the mask alone
    kind, fill, hist, _, words = S.encode_block(np.full(4096, 0x41, np.uint8), "rule")
    assert (kind, fill, int(hist.sum()), words.tolist()) == (S.SPARSE, 0x41, 0, [0, 0])


def _test_blocks():
    out = []
    for elem, delta in TRIPLES:
        x = I.container_input(elem, delta)
        fmt = S.stream_format(S.VERSION, M.FLAG_DELTA if delta else 0, elem)
        rows, n = I.rows_of(elem), 8192
        pos = 0
        while pos < x.size:
            left = x.size - pos
            nb, bl = (min(rows, left // n), n) if left >= n else (1, left)
            f = M.filter_frame(x[pos:pos + nb * bl], fmt)
            out += [f[i * bl:(i + 1) * bl] for i in range(nb)]
            pos += nb * bl
    for kind in series_datagen.KINDS:
        e = series_datagen.ELEM[kind]
        f = M.delta_shuffle(series_datagen.series_bytes(kind, 1 << 18), e)
        out += [f[i:i + 65536] for i in range(0, f.size, 65536)]
    return out


def test_a_sparse_record_is_never_longer_than_the_order0_record():
    seen3 = 0
    for blk in _test_blocks():
        if 32 * S.elided(blk) < S.nchunks(blk.size):
            continue
        fill, mask, K = S.split(blk)
        w3 = mask.size + (M.h0_words(np.bincount(K, minlength=256)) if K.size else 0)
        w2 = M.h0_words(np.bincount(blk, minlength=256))
        assert w3 <= w2, (blk.size, w3, w2)
        seen3 += 1
    assert seen3 >= 40


# --- the writer and the reader -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", TRIPLES)
def test_model_round_trip(elem, delta):
    x = I.container_input(elem, delta)
    rows = I.rows_of(elem)
    for n, data in ((8192, x), (1000, x[:7 * 1000 + 123]), (8192, x[:0]), (8192, x[:1]), (4096, x[3 * 8192 * rows - 5:])):
        c = S.write(data, n, rows, elem, delta)
        assert len(c) % 8 == 0 and len(c) <= M.bound(data.size, n)
        assert struct.unpack("<IHHII", c[:16])[1:] == (5, 1 if delta else 0, n, elem)
        assert struct.unpack("<I", c[-8:-4])[0] == zlib.crc32(data.tobytes())
        back, kinds = S.read(c, with_kinds=True)
        assert np.array_equal(back, data) and set(kinds) <= {1, 2, 3}
    c = S.write(x, 8192, rows, elem, delta)
    assert set(S.read(c, with_kinds=True)[1]) == {1, 2, 3}
    # a version-5 frame may hold all four kinds in any mix
    c = S.write(x[:9 * 4096 + 100], 4096, 4, elem, delta, kinds=[3, 0, 2, 1, 0, 3])
    back, kinds = S.read(c, with_kinds=True)
    assert np.array_equal(back, x[:9 * 4096 + 100]) and {0, 1} <= set(kinds) <= {0, 1, 2, 3}


def test_the_reader_takes_any_fill_and_mask_that_pass_the_checks():
    """not the writer's canonical choice: a kept chunk that is all fill, and a fill that is not the most frequent byte"""
    blk = np.zeros(4096, np.uint8)
    blk[64:128] = 7
    blk[640:700] = np.arange(60, dtype=np.uint8) + 1
    rec = S.encode_block3(blk, fill=7)                             # fill 7: one chunk elided, the zero chunks kept
    assert rec[0] == S.SPARSE and rec[1] == 7 and int(rec[2][0]) == 4096 - 64 - 60
    c = bytearray(S.write(blk, 4096, 1, kinds=[3]))
    T = M.tables_layout(1, 4096)
    W = np.zeros(T["words"], np.uint32)
    W[T["kind"]], W[T["bwt"]] = S.SPARSE, 7
    W[T["crc_raw"]], W[T["crc_rec"]] = zlib.crc32(blk.tobytes()), zlib.crc32(rec[4].tobytes())
    W[T["hist"]:T["hist"] + 256] = rec[2]
    W[T["pay_off"]:T["pay_off"] + 4] = np.asarray([0, rec[4].size], np.uint64).view(np.uint32)
    P = rec[4].size
    hdr24 = M.MAGIC_FRAME + struct.pack("<III", 1, 4096, 0) + struct.pack("<Q", P)
    frame = hdr24 + struct.pack("<II", zlib.crc32(hdr24 + W.tobytes()), 0) + W.tobytes() + rec[4].tobytes() + (b"\0" * 4 if P & 1 else b"")
    other = bytes(c[:32]) + frame + bytes(c[-16:])
    assert other != bytes(c) and np.array_equal(S.read(other), blk)


def _refused(reader, c, **kw):
    with pytest.raises(M.ContainerError) as e:
        reader(c, **kw)
    return e.value.what, e.value.frame, e.value.block


@pytest.mark.parametrize("elem,delta", [(0, False), (4, False), (8, True)])
def test_refusals_of_version_5(elem, delta):
    x = I.container_input(elem, delta)
    c5 = S.write(x, 8192, I.rows_of(elem), elem, delta)
    assert _refused(M.read, c5) == (M.STREAM_HEADER, -1, -1)                   # the reader of version 4
    assert _refused(S.read, c5, max_version=4) == (M.STREAM_HEADER, -1, -1)
    assert np.array_equal(S.read(c5), x)
    cases, lay = S.refusal_cases(c5, elem)
    names = [name for name, _, _ in cases]
    for need in ("kind 3 under a version-4 header", "version 5 with flags 2", "fill 256", "an unused mask bit set",
                 "a kept and an elided bit swapped", "one word too many", "one word too few", "a flipped stream bit", "a flipped fill",
                 "cut inside the mask"):
        assert need in names
    whats = set()
    for name, cont, want in cases:
        assert _refused(S.read, cont) == want, name
        whats.add(want[0])
    assert whats == {1, 2, 3, 4, 5}
    # versions 1 to 4 read as container_model reads them
    for c in (M.write(x, 8192, 4), M.write(x, 8192, 4, 4), M.write(x, 8192, 4, 4, 1), M.write(x, 8192, 4, 4, 1, delta=True)):
        assert np.array_equal(S.read(c), x)
        assert _refused(S.read, M.with_header(c, 5, 2, 4)) == (M.STREAM_HEADER, -1, -1)


def test_golden_fixture_is_what_its_generator_makes():
    spec = importlib.util.spec_from_file_location("make_container_v5_gold", os.path.join(ROOT, "tests", "golden", "make_container_v5_gold.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    gold = open(GOLD, "rb").read()
    x = g.gold_input()
    assert (g.BLOCK, g.ROWS, g.ELEM) == (4096, 8, 8) and x.size % g.ELEM != 0 and x.size % g.BLOCK != 0
    assert len(gold) <= 64 << 10
    assert g.make() == gold
    assert struct.unpack("<HHII", gold[4:16]) == (5, 1, g.BLOCK, g.ELEM)
    data, kinds = S.read(gold, with_kinds=True)
    assert np.array_equal(data, x)
    assert kinds == list(g.KINDS)                                  # the forced kinds, no block fallen back to raw
    frames = M.layout(gold)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(8, 4096), (2, 4096), (1, 1235)]
    T = M.tables_layout(8, 4096)
    W = np.frombuffer(gold[frames[0]["tables"][0]:frames[0]["tables"][1]], np.uint32)
    assert int(W[T["hist"]:T["hist"] + 256].sum()) == 0 and frames[0]["records"][0][1] - frames[0]["records"][0][0] == 8   # klen = 0
    assert int(W[T["bwt"] + 4]) == 0x10                            # a fill byte that is not zero
    assert _refused(M.read, gold) == (M.STREAM_HEADER, -1, -1)


# --- what the mode is for ----------------------------------------------------------------------------------------------------
MiB = 1 << 20


def test_ts64_with_the_sparse_mode_is_at_most_070_of_version_4():
    """a condition on the model alone: 1 MiB of ts64, block_len 65536, rows 8, elem 8, delta on, framing included"""
    x = series_datagen.series_bytes("ts64", MiB)
    v4 = len(M.write(x, 65536, 8, 8, 1, delta=True))
    v5 = len(S.write(x, 65536, 8, 8, delta=True))
    print("ts64: version 4 %d bytes, version 5 %d: %.3f of it (ratios %.3f, %.3f)" % (v4, v5, v5 / v4, x.size / v4, x.size / v5))
    assert v5 <= 0.70 * v4
