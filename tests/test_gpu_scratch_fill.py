"""No result may depend on what the library's scratch memory held when it was allocated (-m gpu).

Every block of device and pinned memory the library allocates for itself comes from the helpers of csrc/glc_internal.h
(test_cpu_alloc_sites.py), and glcDebugSetScratchFill makes them fill each block with a chosen 32-bit word before use.  Each
test here sets a fill, creates its plans BEHIND it, runs calls that reach every sorter tier, both Huffman decoders and the
inverse MTF, every container mode and the other entry points that allocate, and compares with the CPU side only -- the
oracle and the container models, never a run with the seam off -- and asserts that blocks were in fact filled.  A word that
is read before the call wrote it shows as a wrong result under one of the words: 0 (what a fresh process mostly sees), 1 and
0x100 (plausible small counters and flags), 0xFFFFFFFF (the largest count, every flag bit).

The seam is process-wide and the suite shares a process: the autouse fixture below switches it off behind every test."""
import contextlib
import functools
import os
import zlib

import numpy as np
import pytest

import container_model as M
import datagen
import dec_huff_inputs as D
import oracle_lib as O
import small_container as S
import tier_batches as T

FILLS = (0x00000000, 0x00000001, 0x00000100, 0xFFFFFFFF)
fills = pytest.mark.parametrize("word", FILLS, ids=["fill_%08x" % w for w in FILLS])
gpu = pytest.mark.gpu
N1M = 1 << 20
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _seam_off_behind_every_test(glc):
    try:
        yield
    finally:
        glc.debug_set_scratch_fill(None)


@contextlib.contextmanager
def _filled(glc, word, what):
    """the seam on with `word`; on the way out: blocks and bytes were filled (and are printed, for profiles/scratch_state.md)"""
    glc.debug_set_scratch_fill(word)
    before = glc.debug_scratch_fill_stats()
    yield
    blocks, nbytes = glc.debug_scratch_fill_stats()
    print("scratch fill %08x, %s: %d blocks, %d bytes" % (word, what, blocks, nbytes))
    assert blocks > before[0] and nbytes > before[1], "no allocation went through the seam"


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


# --- expected values, from the CPU side, once per module ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_bwt(key):
    return [O.bwt(b) for b in _blocks(key)]


@functools.lru_cache(maxsize=None)
def _want_compress(key):
    if key == "all_tiers":
        return list(T.all_tiers_compressed_1m())               # (shared with the other modules that make this call)
    return [O.compress(b) for b in _blocks(key)]


@functools.lru_cache(maxsize=None)
def _want_sa(key):
    return [O.suffix_array(b) for b in _blocks(key)]


@functools.lru_cache(maxsize=None)
def _blocks(key):
    if key == "all_tiers":
        return T.all_tiers_blocks_1m()
    if key == "second_attempt":
        # tests/golden/log_block_bucket_overflow.bin.bz2 (test_gpu_sample_sorter.py): the first samples leave a bucket past its
        # slot.  The two text blocks are finished by the first attempt, so a COMPRESS plan runs their stages on the side
        # stream beside the second one (ss_mask, aux, ev_fork / ev_join); the Zipf block never leaves the bucket sorter.
        import bz2
        blk = np.frombuffer(bz2.decompress(open(os.path.join(HERE, "golden", "log_block_bucket_overflow.bin.bz2"), "rb").read()), dtype=np.uint8)
        assert blk.size == N1M
        return (datagen.zipf_bytes(N1M, seed=900), blk, datagen.text_bytes(N1M, seed=901), datagen.text_bytes(N1M, seed=902))
    if key == "sixteen":
        # 16 blocks: k_fs_part2's large-tile instance (8192 suffixes a tile).  n = 140001: 18 tiles, two workgroups a block, a
        # ragged last tile; every fourth block text, which the bucket sorter flags
        n = 140001
        return tuple(datagen.text_bytes(n, seed=40 + i) if i % 4 == 1 else datagen.zipf_bytes(n, seed=40 + i) for i in range(16))
    kind, n = key                                              # one short block on a plan of n = 65536, as the rigs' tails
    return (datagen.text_bytes(n, seed=n) if kind == "text" else np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8),)


def _bwt_batch(glc, plan, blocks):
    import torch
    n, rows = blocks[0].size, len(blocks)
    d_in = _gpu(np.concatenate(blocks))
    d_out = torch.zeros(n * rows, dtype=torch.uint8, device=d_in.device)
    d_idx = torch.zeros(rows, dtype=torch.int32, device=d_in.device)
    assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, rows) == 0
    plan.synchronize()
    return _host(d_out), _host(d_idx)


def _assert_bwt(got, gidx, want, n, what):
    for i, (w, widx) in enumerate(want):
        assert int(gidx[i]) == widx, "%s: BWT index of block %d" % (what, i)
        assert np.array_equal(got[i * n:(i + 1) * n], w), "%s: BWT of block %d" % (what, i)


def _assert_compress(out, want, what):
    for i, w in enumerate(want):
        size = int(out["size"][i].item())
        assert int(out["bwt_index"][i].item()) == w["bwt_index"] and size == w["size"], "%s: index / size of block %d" % (what, i)
        words = _host(out["words"][i * out["stride"]:i * out["stride"] + size]).view(np.uint32)
        assert np.array_equal(words, w["words"]), "%s: stream of block %d" % (what, i)
        assert np.array_equal(_host(out["hist"][i * 256:(i + 1) * 256]).view(np.uint32), w["hist"]), "%s: histogram of block %d" % (what, i)
        nsub = out["nsub"]
        assert np.array_equal(_host(out["offsets"][i * nsub:i * nsub + w["offsets"].size]).view(np.uint32), w["offsets"]), "%s: offsets of block %d" % (what, i)


def _compress_round_trip(glc, plan, blocks, want, what):
    n, rows = blocks[0].size, len(blocks)
    x = np.concatenate(blocks)
    out = glc.compress_batch(plan, _gpu(x), n, rows)
    plan.synchronize()
    stats = plan.last_sort_stats(), plan.last_sort_resumed(), plan.last_sort_retries()
    _assert_compress(out, want, what)
    back = glc.decompress_batch(plan, out, n, rows)
    plan.synchronize()
    assert np.array_equal(_host(back), x), "%s: glcDecompressBatch" % what
    return stats


# --- 1. the sorter's tiers -------------------------------------------------------------------------------------------------
@gpu
@fills
@pytest.mark.parametrize("sorter", [0, 4])
def test_all_tiers_through_a_bwt_plan(glc, cuda, word, sorter):
    """test_gpu_resume.py's nine-block call: bucket sorter, sample sorter, periodic tier, resumed doubling, general sorter, a
    constant block.  Sorter mode 4 sends every block to the sample sorter first."""
    blocks = _blocks("all_tiers")
    with _filled(glc, word, "all tiers, BWT plan, sorter %d" % sorter):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_BWT, N1M, rows=len(blocks)) as plan:
            plan.set_sorter(sorter)
            got, gidx = _bwt_batch(glc, plan, blocks)
            if sorter == 0:                                    # the tiers really ran
                assert plan.last_sort_stats() == T.ALL_TIERS_STATS and plan.last_sort_resumed() == T.ALL_TIERS_RESUMED, (
                    plan.last_sort_stats(), plan.last_sort_resumed())
            else:
                # no attempt of the bucket sorter: every block but the constant one (finished by k_fs_tables) starts flagged,
                # the Zipf and the text block are finished by the sample sorter, the six deep ones go on as under sorter 0
                assert plan.last_sort_skipped()[0] is True
                assert plan.last_sort_stats() == (8, T.ALL_TIERS_STATS[1]) and plan.last_sort_resumed() == T.ALL_TIERS_RESUMED, (
                    plan.last_sort_stats(), plan.last_sort_resumed())
            _assert_bwt(got, gidx, _want_bwt("all_tiers"), N1M, "sorter %d" % sorter)


@gpu
@fills
def test_all_tiers_through_an_sa_plan(glc, cuda, word):
    """cudppSuffixArray takes one block a call and writes the suffix array itself (bwt_out == nullptr: k_fs_sort, the rows of
    s.sa, no periodic tier): the nine blocks one after the other on one plan.  Sorter mode 6 is mode 0 that resumes a lone
    deep block too (by default a call needs two of them), so that the resumed doubling runs here as well."""
    import torch
    blocks = _blocks("all_tiers")
    with _filled(glc, word, "all tiers, SA plan"):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_SA, N1M) as plan:
            plan.set_sorter(6)
            flagged = general = resumed = 0
            for i, b in enumerate(blocks):
                d_out = torch.zeros(N1M + 1, dtype=torch.int32, device=cuda)
                assert glc.lib().cudppSuffixArray(plan.handle, _gpu(b).data_ptr(), d_out.data_ptr(), N1M) == glc.CUDPP_SUCCESS
                plan.synchronize()
                got = _host(d_out).view(np.uint32)
                assert got[0] == N1M and np.array_equal(got[1:], _want_sa("all_tiers")[i]), "suffix array of block %d" % i
                f, g = plan.last_sort_stats()
                flagged, general, resumed = flagged + f, general + g, resumed + plan.last_sort_resumed()
            # block by block, the same blocks leave each tier as in the one call of nine
            assert (flagged, general) == T.ALL_TIERS_STATS and resumed == T.ALL_TIERS_RESUMED, (flagged, general, resumed)


@gpu
@fills
def test_all_tiers_through_compress_and_decompress(glc, cuda, word):
    blocks = _blocks("all_tiers")
    with _filled(glc, word, "all tiers, COMPRESS plan"):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, N1M, rows=len(blocks)) as plan:
            stats, resumed, _ = _compress_round_trip(glc, plan, blocks, _want_compress("all_tiers"), "all tiers")
            assert stats == T.ALL_TIERS_STATS and resumed == T.ALL_TIERS_RESUMED, (stats, resumed)


@gpu
@fills
def test_second_attempt_of_the_sample_sorter(glc, cuda, word):
    blocks = _blocks("second_attempt")
    with _filled(glc, word, "second attempt"):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, N1M, rows=len(blocks)) as plan:
            _, _, retries = _compress_round_trip(glc, plan, blocks, _want_compress("second_attempt"), "second attempt")
            assert retries > 0, "no block took the second attempt: the call exercises nothing"
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_BWT, N1M, rows=len(blocks)) as plan:
            got, gidx = _bwt_batch(glc, plan, blocks)
            assert plan.last_sort_retries() > 0
            _assert_bwt(got, gidx, _want_bwt("second_attempt"), N1M, "second attempt, BWT plan")


@gpu
@fills
def test_a_call_of_sixteen_blocks(glc, cuda, word):
    blocks = _blocks("sixteen")
    n = blocks[0].size
    with _filled(glc, word, "sixteen blocks"):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_BWT, n, rows=16) as plan:
            got, gidx = _bwt_batch(glc, plan, blocks)
            assert plan.last_sort_stats()[0] >= 4                # the text blocks left the bucket sorter
            _assert_bwt(got, gidx, _want_bwt("sixteen"), n, "sixteen blocks")
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=16) as plan:
            _compress_round_trip(glc, plan, blocks, _want_compress("sixteen"), "sixteen blocks")


@gpu
@fills
@pytest.mark.parametrize("sorter", [0, 4])
@pytest.mark.parametrize("kind", ["text", "random"])
@pytest.mark.parametrize("n", [1203, 12345])
def test_one_short_block_on_a_plan_of_64k(glc, cuda, word, sorter, kind, n):
    """the rigs' tail frames: one block of 1203 or 12345 bytes on a young plan made for 65536"""
    key = (kind, n)
    with _filled(glc, word, "one block of %d (%s), sorter %d" % (n, kind, sorter)):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, 65536, rows=2) as plan:
            plan.set_sorter(sorter)
            _compress_round_trip(glc, plan, _blocks(key), _want_compress(key), "n = %d" % n)
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_BWT, 65536, rows=2) as plan:
            plan.set_sorter(sorter)
            got, gidx = _bwt_batch(glc, plan, _blocks(key))
            _assert_bwt(got, gidx, _want_bwt(key), n, "n = %d, BWT plan" % n)


# --- 2. the decoder's stages -----------------------------------------------------------------------------------------------
DEC_SINGLE = ("size_1", "size_4097", "last_sub_block_of_5", "skewed_sub_block", "code_of_28_bits")
DEC_BATCHES = ((4099, 4099, 3), (70001, 4099, 3))


@functools.lru_cache(maxsize=None)
def _dec_cases():
    """name -> (plan n, n, blocks of symbols, the oracle's stream of each, what the inverse MTF makes of each)"""
    single = D.single_block_cases()
    out = {k: (single[k].size, single[k].size, [single[k]]) for k in DEC_SINGLE}
    for plan_n, n, nblk in DEC_BATCHES:
        out["batch_%d_on_%d" % (n, plan_n)] = (plan_n, n, D.batch_blocks(n, nblk))
    return {k: (pn, n, blks, [D.encode(b) for b in blks], [O.imtf(b) for b in blks]) for k, (pn, n, blks) in out.items()}


def _strided(glc, cuda, streams, n):
    import torch
    nblk, nsub, stride = len(streams), (n + D.SUB - 1) // D.SUB, glc.compressed_stride_words(n)
    words = np.zeros(nblk * stride, dtype=np.uint32)
    for b, r in enumerate(streams):
        words[b * stride:b * stride + r["size"]] = r["words"]
    return dict(hist=torch.from_numpy(np.concatenate([r["hist"] for r in streams]).view(np.int32).copy()).to(cuda),
                offsets=torch.from_numpy(np.concatenate([r["offsets"] for r in streams]).view(np.int32).copy()).to(cuda),
                words=torch.from_numpy(words.view(np.int32)).to(cuda), nsub=nsub, stride=stride)


@gpu
@fills
@pytest.mark.parametrize("mode", [1, 2])
def test_huffman_decoders_and_inverse_mtf_stage_by_stage(glc, cuda, word, mode):
    """glcHuffmanDecodeBatch under each kernel and glcMtfInverseBatch on dec_huff_inputs.py's arrays, one block and a few: the
    symbols are the oracle encoder's input, the bytes behind the inverse MTF the oracle's"""
    with _filled(glc, word, "decode stages, decoder %d" % mode):
        for name, (plan_n, n, blks, streams, plain) in _dec_cases().items():
            with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, plan_n, rows=len(blks)) as plan:
                plan.set_huff_decoder(mode)
                sym = glc.huffman_decode_batch(plan, _strided(glc, cuda, streams, n), n, len(blks))
                plan.synchronize()
                assert np.array_equal(_host(sym), np.concatenate(blks)), "%s: symbols" % name
                back = glc.mtf_inverse_batch(plan, _gpu(np.concatenate(blks)), n, len(blks))
                plan.synchronize()
                assert np.array_equal(_host(back), np.concatenate(plain)), "%s: inverse MTF" % name


# --- 3. the container ------------------------------------------------------------------------------------------------------
def test_the_small_container_takes_every_path():
    """CPU: the frames are the rigs' scaled down, and every mode writes the record kind it exists for"""
    for name, (_, _, kind) in S.CONFIGS.items():
        lay = M.layout(S.want(name))
        frames = [(f["nb"], f["blk_len"]) for f in lay["frames"]]
        if name != "choose":                                  # (the CHOOSE codec cuts a frame wherever its choice changes)
            assert frames == [(4, S.N), (4, S.N), (1, S.N), (1, S.TAIL)], name
        else:
            assert frames[-1] == (1, S.TAIL) and sum(nb for nb, _ in frames) == 10
        kinds = {k for f in lay["frames"] for (_, _, k) in f["records"]}
        assert kind is None or kind in kinds, (name, kinds)
    kinds = [k for f in M.layout(S.want("choose"))["frames"] for (_, _, k) in f["records"]]
    assert M.HUFF in kinds and 2 in kinds                      # both codecs chosen


def test_the_filter_inputs_pick_what_their_formats_add():
    """CPU: from the frame words of the expected containers, the inputs of S.FILTERS between them pick a lag above 1 at each of
    elem 2 and elem 4, a grid width, a byte candidate with a stride and one with a lag alone; the hand-set byte predictor's
    header names its pair; and each model reads its container back to the input.  Without this the entries could go as hollow
    as four more names in S.CONFIGS would be: on S.data() formats 13, 14 and 16 all pick what format 10 picks."""
    import struct
    import byte_delta_model as BD
    import filter_auto_model as F
    import filter_byte_model as B
    import filter_grid_model as Q
    import filter_lag_model as FL
    picks = {name: [mod.word_format(w) for w in F.frame_words(S.entry(name)[3])]
             for name, mod in (("filter_lag", FL), ("filter_grid", Q), ("filter_byte", B))}
    for elem in (2, 4):
        assert any(e == elem and d == 1 and lag > 1 for e, d, lag, _ in picks["filter_lag"]), (elem, picks["filter_lag"])
    assert any(w > 0 and e > 1 for e, _, _, _, w in picks["filter_grid"]), picks["filter_grid"]
    byte = [p for p in picks["filter_byte"] if B.is_byte(p)]
    assert any(p[4] > 0 for p in byte), byte                   # a stride
    assert any(p[4] == 0 and p[2] > 1 for p in byte), byte     # a lag alone
    for name, (lag, stride) in (("byte_delta", (3, 1281)), ("byte_delta_lag", (1, 0))):
        flags, _, word3 = struct.unpack("<HHII", S.entry(name)[3][4:16])[1:]
        assert struct.unpack("<H", S.entry(name)[3][4:6])[0] == BD.VERSION and BD.lag_stride_of(flags, word3) == (lag, stride), name
    versions = dict(filter_lag=13, filter_grid=14, filter_byte=16, byte_delta=15, byte_delta_lag=15)
    for name, (n, rows, _, _, _, read) in S.FILTERS.items():
        pn, prows, x, want = S.entry(name)
        assert (pn, prows) == (n, rows) and struct.unpack("<H", want[4:6])[0] == versions[name], name
        frames = [(f["nb"], f["blk_len"]) for f in M.layout(want)["frames"]]
        assert frames[0] == (rows, n) and len(frames) >= 2 and frames[-1][0] == 1 and frames[-1][1] < n, (name, frames)   # a full frame, a ragged tail
        assert np.array_equal(read(want), x), name


# further range reads of an entry: filter_byte's first frame is a greyscale image 721 wide whose band is 24576 bytes, so this one
# starts mid-band in it (test_gpu_container_filter_byte.py::test_range_reads)
MORE_RANGES = {"filter_byte": ((30000, 3000),)}


@gpu
@fills
@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
@pytest.mark.parametrize("name", list(S.ALL))
def test_container_modes(glc, cuda, word, name, pipelined):
    """bytes equal the model's; the same plan and a fresh plan decode them; one range read across a frame boundary"""
    n, rows, x, want = S.entry(name)
    with _filled(glc, word, "container %s%s" % (name, ", pipelined" if pipelined else "")):
        with glc.Cudpp() as ctx:
            with S.configure(glc, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows), name, pipelined) as plan:
                d_c = glc.container_compress(plan, _gpu(x))
                assert _host(d_c).tobytes() == want, "container bytes"
                assert np.array_equal(_host(glc.container_decompress(plan, d_c)), x), "decode on the plan that wrote it"
                assert glc.container_last_error(plan) == (0, -1, -1)
            with S.configure(glc, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows), name, pipelined) as fresh:
                d_w = _gpu(np.frombuffer(want, np.uint8))
                assert np.array_equal(_host(glc.container_decompress(fresh, d_w)), x), "decode on a fresh plan"
                ranges = ((rows - 1) * n + 100, n + 500),      # the last block of frame 0 and the first of frame 1
                with glc.container_index(fresh, d_w) as ix:
                    for off, count in ranges + MORE_RANGES.get(name, ()):
                        got = _host(glc.container_read_range(fresh, ix, d_w, off, count))
                        assert np.array_equal(got, x[off:off + count]), "range read (%d, %d)" % (off, count)


@gpu
@fills
def test_container_host_pointer_form(glc, cuda, word):
    """glcContainerCompressHost / DecompressHost: their device buffers and pinned staging are the library's, and get the fill"""
    x = S.data()
    with _filled(glc, word, "container, host pointers"):
        with glc.Cudpp() as ctx:
            for name in ("bwt", "huff0_delta"):
                with S.configure(glc, glc.Plan(ctx, glc.CUDPP_COMPRESS, S.N, rows=S.ROWS), name, True) as plan:
                    c = glc.container_compress_host(plan, x)
                    assert c.tobytes() == S.want(name), name
                    assert np.array_equal(glc.container_decompress_host(plan, c), x), name


# --- 4. the rest of the C ABI that allocates --------------------------------------------------------------------------------
@gpu
@fills
def test_mtf_plan(glc, cuda, word):
    import torch
    n, rows = 70001, 3
    blocks = [datagen.text_bytes(n, seed=1), datagen.zipf_bytes(n, seed=2), np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8)]
    with _filled(glc, word, "MTF plan"):
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_MTF, n, rows=rows) as plan:
            d_in = _gpu(np.concatenate(blocks))
            d_out = torch.zeros_like(d_in)
            assert glc.lib().glcMtfBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), n, rows) == glc.CUDPP_SUCCESS
            plan.synchronize()
            assert np.array_equal(_host(d_out), np.concatenate([O.mtf(b) for b in blocks]))


@gpu
@fills
def test_crc32_segments(glc, cuda, word):
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, 70000, dtype=np.uint8)
    offs = [0, 1, 3, 7, 4096, 100]
    lens = [0, 1, 4097, 65535, 1203, 12345]
    with _filled(glc, word, "glcCrc32Segments"):
        got = glc.crc32_segments(_gpu(buf), offs, lens)
    assert got == [zlib.crc32(buf[o:o + L].tobytes()) for o, L in zip(offs, lens)]


@gpu
@fills
def test_culzss_pair(glc, cuda, word):
    """culzss_compress / culzss_decompress: the ring's slots and the decode scratch.  The slots live as long as the process:
    deleteGPUStreams releases them first, so that this call allocates them again behind the fill"""
    import ctypes as C
    L = glc.lib()
    y = datagen.log_bytes(3 * 4096, seed=99)                   # (the oracle's matcher takes whole 4096-byte packets)
    want = O.lzss_pack(O.lzss_candidates(y), y.size)
    L.deleteGPUStreams()
    with _filled(glc, word, "CULZSS"):
        packed = np.zeros(L.glcLzssPackStride(y.size), dtype=np.uint8)
        m, k = C.c_int(0), C.c_int(0)
        assert L.culzss_compress(y.ctypes.data, y.size, packed.ctypes.data, C.byref(m)) == 1
        assert m.value == want.size and np.array_equal(packed[:m.value], want)
        back = np.zeros(y.size, dtype=np.uint8)
        assert L.culzss_decompress(packed.ctypes.data, m.value, back.ctypes.data, C.byref(k)) == 1
        assert k.value == y.size and np.array_equal(back, y)
    L.deleteGPUStreams()                                       # and nothing filled outlives the test
