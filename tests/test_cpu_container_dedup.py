"""Frame-wide chunk dedup without a GPU: the library exports the batched passes and validates their arguments before touching a
device; the model of record kind 6 and format version 9 (tests/dedup_model.py) hashes as the format says, round-trips every input
of tests/dedup_inputs.py, never makes a kind-6 record longer than the block's kind-2 record, is refused by readers of versions up
to 8, reproduces the golden fixture with the blocks it is there for, refuses what the format forbids; and the range-read rule of
csrc/dedup_rule.h, dumped by tools/dedup_rule_check.cpp built under the host sanitizers, agrees with the model."""
import importlib.util
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import container_model as M
import dedup_inputs as I
import dedup_model as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "dedup_v9_container.bin")
NEW = ["glcDedupWorkBytes", "glcDedupMapSegments", "glcDedupFillSegments"]
BLOCKS = (1536, 4196, 65536)
SIZE = 300000 + 77                                                 # under 512 pages: `shifted` dedups nothing


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_dedup_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("dedup_map_segments", "dedup_fill_segments", "dedup_chunks"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW) and "GLC_DEDUP_MAX_LEN" in decl and "GLC_DEDUP_MAX_COUNT" in decl


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, OK = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_SUCCESS
    a, o, n, s, w = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    wb = L.glcDedupWorkBytes(3, 4096)
    assert wb == 16 * (64 + 1) + 8 * 24                            # 24 chunks: 64 slots (the smallest table), one spare, the hashes
    assert L.glcDedupWorkBytes(512, 1 << 20) == 16 * ((1 << 21) + 1) + 8 * (1 << 20)     # about 40 MiB for rows 512, n 1 MiB
    assert L.glcDedupWorkBytes(0, 4096) == 0 and L.glcDedupWorkBytes(3, 0) == 0
    assert L.glcDedupWorkBytes(3, (1 << 20) + 1) == 0 and L.glcDedupWorkBytes((1 << 22) + 1, 512) == 0
    assert L.glcDedupWorkBytes(1 << 22, 1 << 17) != 0 and L.glcDedupWorkBytes(1 << 22, (1 << 17) + 1) == 0                # 2^30 chunks at most
    mp, fill = L.glcDedupMapSegments, L.glcDedupFillSegments
    assert mp(None, None, None, 0, 4096, None, None, 0, None) == OK and fill(None, None, None, 0, 4096, None, None) == OK
    assert mp(None, None, None, 3, 0, None, None, 0, None) == OK and fill(None, None, None, 3, 0, None, None) == OK
    good = [a, o, n, 3, 4096, s, w, wb]
    for i in (0, 1, 2, 5, 6):                                      # each pointer null in turn
        args = list(good)
        args[i] = None
        assert mp(*args, None) == ILLEGAL
    for args in (good[:5] + [s + 2, w, wb], good[:6] + [w + 8, wb], good[:7] + [wb - 1], good[:4] + [(1 << 20) + 1] + good[5:],
                 good[:3] + [(1 << 22) + 1, 512] + good[5:], good[:3] + [1 << 22, (1 << 17) + 1] + good[5:]):
        assert mp(*args, None) == ILLEGAL
    fgood = [a, o, n, 3, 4096, s]
    for i in (0, 1, 2, 5):
        args = list(fgood)
        args[i] = None
        assert fill(*args, None) == ILLEGAL
    for args in (fgood[:5] + [s + 1], fgood[:4] + [(1 << 20) + 1, s], fgood[:3] + [(1 << 22) + 1, 512, s], fgood[:3] + [1 << 22, (1 << 17) + 1, s]):
        assert fill(*args, None) == ILLEGAL


# --- the hash and the map ----------------------------------------------------------------------------------------------------
def _naive_hash(chunk):
    """the format's words, one chunk, in Python integers"""
    b = bytes(chunk) + b"\0" * (512 - len(chunk))
    w = struct.unpack("<128I", b)
    k = [((0x9E3779B97F4A7C15 * (j + 1)) & D.MASK64) >> 32 for j in range(128)]
    s = sum(((w[2 * i] + k[2 * i]) & 0xFFFFFFFF) * ((w[2 * i + 1] + k[2 * i + 1]) & 0xFFFFFFFF) for i in range(64)) + len(chunk)
    h = s & D.MASK64
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & D.MASK64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & D.MASK64
    return h ^ (h >> 33)


def test_the_hash_is_the_formats():
    rng = np.random.default_rng(1)
    assert D.KEYS[0] == 0x9E3779B9 and D.KEYS[1] == 0x3C6EF372 and D.KEYS[127] == ((0x9E3779B97F4A7C15 * 128) & D.MASK64) >> 32
    for n in (1, 3, 4, 100, 511, 512, 513, 1031, 2048):
        blk = rng.integers(0, 256, n, dtype=np.uint8)
        assert D.chunk_hashes(blk).tolist() == [_naive_hash(blk[i:i + 512]) for i in range(0, n, 512)]
    full = np.full(1024, 0xFF, np.uint8)                           # every sum wraps
    assert D.chunk_hashes(full).tolist() == [_naive_hash(full[:512])] * 2
    # the length is hashed: a short chunk of zeros and a longer one differ, and both differ from the padded full chunk
    z = [int(D.chunk_hashes(np.zeros(n, np.uint8))[0]) for n in (1, 2, 511, 512)]
    assert len(set(z)) == 4


def test_the_map_follows_the_writers_rule():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 256, (2, 512), dtype=np.uint8)
    a0, a511 = a.copy(), a.copy()
    a0[0] ^= 1
    a511[511] ^= 0x80
    segs = [np.concatenate([a, b, a, a0, a[:100]]), np.concatenate([a511, b, a0, a, b[:100]]), np.concatenate([b, b, a511, b, a[:100]])]
    src = D.map_segments(segs, 2148).reshape(3, 5)
    assert src.tolist() == [[0, 1, 0, 3, 4], [5, 1, 3, 0, 9], [1, 1, 5, 1, 4]]
    # a source is always kept, and smaller than what it serves
    flat = src.reshape(-1)
    assert all(flat[flat[g]] == flat[g] and flat[g] <= g for g in range(flat.size))
    # a short chunk that is the head of a full one stays kept; ids past a segment's end are their own
    assert D.map_segments([a, a[:100]], 512).tolist() == [0, 1]
    assert D.map_segments([a[:100], a[:100], a], 1024).tolist() == [0, 1, 0, 3, 4, 5]
    # a hash collision keeps the chunk: two chunks with one (forced) hash and other bytes
    real = D.chunk_hashes
    try:
        D.chunk_hashes = lambda blk: np.zeros(D.nchunks(len(blk)), np.uint64)
        assert D.map_segments([np.concatenate([a, b, a])], 1536).tolist() == [0, 1, 0]
    finally:
        D.chunk_hashes = real
    # fill is the inverse
    holes = [s.copy() for s in segs]
    for i in range(3):
        for c in range(5):
            if src[i, c] != 5 * i + c:
                holes[i][512 * c:512 * c + 512] = 0xEE
    assert all(np.array_equal(x, y) for x, y in zip(D.fill_segments(holes, flat, 2148), segs))


# --- the writer and the reader -------------------------------------------------------------------------------------------
_MADE = {}


def _made(name, bl):
    """(input, container, kinds) of one input at one block length, rows 4: written and read once"""
    if (name, bl) not in _MADE:
        x = I.make(name, SIZE)
        c = D.write(x, bl, 4)
        back, kinds = D.read(c, with_kinds=True)
        assert np.array_equal(back, x)
        _MADE[(name, bl)] = (x, c, kinds)
    return _MADE[(name, bl)]


@pytest.mark.parametrize("bl", BLOCKS)
@pytest.mark.parametrize("name", I.NAMES)
def test_model_round_trip(name, bl):
    x, c, kinds = _made(name, bl)
    assert len(c) % 8 == 0 and len(c) <= M.bound(x.size, bl)
    assert D.size(x, bl, 4) == (len(c), kinds)                     # the sizing-only model, what benchmark-size inputs are held against
    assert struct.unpack("<IHHII", c[:16])[1:] == (9, 0, bl, 0)
    assert struct.unpack("<I", c[-8:-4])[0] == zlib.crc32(x.tobytes())
    assert set(kinds) <= {1, 2, 6}
    if name in ("pages", "pages_noise", "zeros", "tar_like") and (bl == 65536 or name == "zeros"):
        assert 6 in kinds                                          # (the window is the frame: four blocks)
    if name == "shifted":
        assert 6 not in kinds                                      # nothing to find: the stream is the plain order-0 codec's but for
        c3 = M.write(x, bl, 4, 0, 1)                               # its version
        assert c[32:] == c3[32:] and struct.unpack("<H", c3[4:6])[0] == 3


@pytest.mark.parametrize("elem,delta", [(0, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)])
def test_model_round_trip_behind_the_filters(elem, delta):
    x = I.make("pages", 70000 + 13)
    for bl, data in ((4196, x), (1536, x[:0]), (1536, x[:1]), (512, x[:5 * 512]), (513, x[:5 * 513 + 512])):
        c = D.write(data, bl, 4, elem, delta)
        assert D.size(data, bl, 4, elem, delta)[0] == len(c)
        assert struct.unpack("<IHHII", c[:16])[1:] == (9, 1 if delta else 0, bl, elem)
        assert np.array_equal(D.read(c), data)
    # a version-9 frame may hold kinds 0, 1, 2 and 6 in any mix
    c = D.write(x[:9 * 4196 + 100], 4196, 4, elem, delta, kinds=[6, 0, 2, 1, 0, 6, "rule"])
    back, kinds = D.read(c, with_kinds=True)
    assert np.array_equal(back, x[:9 * 4196 + 100]) and {0, 1} <= set(kinds) <= {0, 1, 2, 6}


def test_a_dedup_record_is_never_longer_than_the_order0_record():
    """rule (4): with E elided chunks and 15 E >= mask words, mask + refs + the stream of K is no longer than the block's kind-2
    record: every elided chunk takes at least 512 bits of codes away and costs 32, the mask 32 a word"""
    seen6 = 0
    for name in I.NAMES:
        for bl in BLOCKS:
            x = I.make(name, SIZE)
            for pos in range(0, x.size - bl + 1, 4 * bl):
                blocks = [x[pos + i * bl:pos + (i + 1) * bl] for i in range(min(4, (x.size - pos) // bl))]
                src = D.map_segments(blocks, bl)
                nch = D.nchunks(bl)
                for b, blk in enumerate(blocks):
                    row = src[b * nch:(b + 1) * nch]
                    if D.rule_kind(row, b, bl) != D.DEDUP:
                        continue
                    kept = row == np.arange(b * nch, (b + 1) * nch)
                    K = D.kept_bytes(blk, kept)
                    w6 = D.mask_words(bl) + int((~kept).sum()) + (M.h0_words(np.bincount(K, minlength=256)) if K.size else 0)
                    w2 = M.h0_words(np.bincount(blk, minlength=256))
                    assert w6 <= w2, (name, bl, b, w6, w2)
                    seen6 += 1
    assert seen6 >= 100


def test_rule_4_at_its_boundary():
    rng = np.random.default_rng(5)
    for nch, E, want in ((480, 1, D.DEDUP), (481, 1, M.HUFF0), (481, 2, D.DEDUP), (961, 2, M.HUFF0), (961, 3, D.DEDUP), (32, 0, M.HUFF0), (1, 0, M.HUFF0)):
        blk = rng.integers(0, 4, nch * 512, dtype=np.uint8)
        for e in range(E):
            blk[512 * (e + 1):512 * (e + 2)] = blk[:512]
        row = D.map_segments([blk], blk.size)
        assert int((row != np.arange(nch)).sum()) == E and (15 * E >= D.mask_words(blk.size)) == (want == D.DEDUP)
        assert D.rule_kind(row, 0, blk.size) == want
        assert D.encode_frame_blocks([blk], ["rule"])[0][0] == want
    # nothing kept: the record is the mask and the refs alone; bwt_index is the lowest block a source lies in
    a = rng.integers(0, 256, 1536, dtype=np.uint8)
    recs = D.encode_frame_blocks([a, rng.integers(0, 4, 1536, dtype=np.uint8), a], ["rule"] * 3)
    kind, lo, hist, _, words = recs[2]
    assert (kind, lo, int(hist.sum()), words.tolist()) == (D.DEDUP, 0, 0, [0, 0, 1, 2])


def _refused(reader, c, **kw):
    with pytest.raises(M.ContainerError) as e:
        reader(c, **kw)
    return e.value.what, e.value.frame, e.value.block


def test_the_reader_takes_sources_the_writer_would_not_choose():
    """any source that passes the field checks: block 0 is forced to kind 2 and so keeps both of its equal chunks; block 1's ref
    is moved from the first of them (the writer's choice) to the second"""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 8, 512, dtype=np.uint8)
    x = np.concatenate([a, rng.integers(0, 8, 512, dtype=np.uint8), a, rng.integers(0, 8, 1024, dtype=np.uint8), a])
    c = D.write(x, 1536, 2, kinds=[2, 6])
    fr = M.layout(c)["frames"][0]
    assert [r[2] for r in fr["records"]] == [2, 6]
    mask, refs, stream = D.record_parts(c, fr, 1)
    assert mask.tolist() == [3] and refs.tolist() == [0]
    words = np.concatenate([mask, np.array([2], np.uint32), stream])
    s, e, _ = fr["records"][1]
    T = M.tables_layout(2, 1536)
    y = bytearray(c)
    y[s:e] = words.tobytes()
    o = fr["tables"][0] + 4 * (T["crc_rec"] + 1)
    y[o:o + 4] = struct.pack("<I", zlib.crc32(words.tobytes()))
    other = M.retable(bytes(y), fr["start"])
    assert other != c and np.array_equal(D.read(other), x) and np.array_equal(D.read(c), x)


# --- refusals and the fixture ------------------------------------------------------------------------------------------------
_GOLD = {}


def _gold():
    if not _GOLD:
        spec = importlib.util.spec_from_file_location("make_dedup_v9_gold", os.path.join(ROOT, "tests", "golden", "make_dedup_v9_gold.py"))
        g = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(g)
        _GOLD.update(g=g, made=g.make(), file=open(GOLD, "rb").read())
    return _GOLD


def test_golden_fixture_is_what_the_model_writes_and_holds_its_cases():
    G = _gold()
    g, gold = G["g"], G["file"]
    assert G["made"] == gold and len(gold) < 400 << 10
    assert struct.unpack("<HHII", gold[4:16]) == (9, 1, I.GOLDEN["block_len"], 8)
    x = I.golden_input()
    data, kinds = D.read(gold, with_kinds=True)
    assert np.array_equal(data, x) and kinds == list(g.KINDS)
    frames = M.layout(gold)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(3, 246372), (3, 246372), (1, 1636)]
    assert x.size % 8 != 0 and frames[2]["records"][0][2] == D.DEDUP                     # the ragged tail dedups within itself
    assert g.cases(gold) == g.WANT and set(g.WANT) == {"sources in an earlier block", "sources in itself", "nothing kept",
                                                        "short last chunk elided", "E > 0 stays kind 2", "raw block is a source"}


def test_readers_of_versions_up_to_8_refuse_the_fixture_at_the_stream_header():
    gold = _gold()["file"]
    import ans_model
    import auto_model
    import runs_model
    import sparse_model
    for mv in range(1, 9):
        assert _refused(D.read, gold, max_version=mv) == (M.STREAM_HEADER, -1, -1)
    for reader in (M.read, sparse_model.read, runs_model.read, ans_model.read, auto_model.read):
        assert _refused(reader, gold) == (M.STREAM_HEADER, -1, -1)


def test_refusals_of_version_9():
    gold = _gold()["file"]
    cases, lay = D.refusal_cases(gold, 8)
    names = [name for name, _, _ in cases]
    for need in ("kind 6 under a version-4 header", "version 9 with flags 2", "version 10", "kind 3 under version 9", "kind 4 under version 9",
                 "kind 5 under version 9", "enc_off set", "a ref equal to its own id", "a ref into a later block", "a ref to an elided chunk",
                 "a full chunk sourced from a short one", "a ref below bwt_index", "bwt_index above the block", "an unused mask bit set",
                 "a wrong sum of hist", "one word too many", "one word too few", "a flipped stream bit", "a ref to another kept chunk",
                 "cut inside the mask"):
        assert need in names
    whats = set()
    for name, cont, want in cases:
        assert _refused(D.read, cont) == want, name
        whats.add(want[0])
    assert whats == {1, 2, 3, 4, 5}
    # an unfiltered stream's cases as well, header case of flags 1 with elem 0 included
    x = I.make("pages", 5 * 4196 + 100).copy()
    x[4196 + 1024:4196 + 2560] = x[2560:4096]                      # block 1: three chunks of block 0
    cases0, _ = D.refusal_cases(D.write(x, 4196, 4), 0)
    assert "version 9, flags 1, elem 0" in [n for n, _, _ in cases0]
    for name, cont, want in cases0:
        assert _refused(D.read, cont) == want, name
    # versions 1 to 4 read as container_model reads them
    for c in (M.write(x, 8192, 4), M.write(x, 8192, 4, 4), M.write(x, 8192, 4, 4, 1), M.write(x, 8192, 4, 4, 1, delta=True)):
        assert np.array_equal(D.read(c), x)
        assert _refused(D.read, M.with_header(c, 9, 2, 4)) == (M.STREAM_HEADER, -1, -1)


# --- range reads: csrc/dedup_rule.h ----------------------------------------------------------------------------------------------
def test_the_range_rule_equals_the_model_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/dedup_rule_check.cpp")
    exe = str(tmp_path / "dedup_rule_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "dedup_rule_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    frames = {"inside-kind6": 0, "own-sources": 0, "across": 0, "no-kind6": 0, "kind0-index-is-no-source": 0, "whole": 0}
    kind, bwt = [2, 1, 2, 2, 6, 2, 6, 0], [0, 0, 0, 0, 1, 0, 6, 77]
    seen = 0
    for _, name, nb, first, last, lo, decoded in lines:
        if name in frames:
            first, last = int(first), int(last)
            assert int(nb) == 8 and int(lo) == D.first_block(kind, bwt, first, last), name
            assert int(decoded) == D.blocks_decoded(kind, bwt, first, last), name
            seen += 1
    assert seen == len(frames) and "dedup_rule_check: ok" in r.stdout
    # and on the fixture's own tables: a range inside frame 0's block 2 needs blocks 0 and 1 as sources
    gold = _gold()["file"]
    fr = M.layout(gold)["frames"][0]
    T, W = D.frame_tables(gold, fr)
    kinds = [r[2] for r in fr["records"]]
    idx = [int(W[T["bwt"] + b]) for b in range(3)]
    assert D.blocks_decoded(kinds, idx, 2, 2) == 3 and D.blocks_decoded(kinds, idx, 0, 0) == 1 and D.first_block(kinds, idx, 1, 2) == 0
