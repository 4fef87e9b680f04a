"""The dedup mode of the container's order-0 codec on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points
write the bytes of the Python model of format version 9 (tests/dedup_model.py), pipelining off and on, and read them back; the
golden fixture decodes; with it off a plan writes versions 3 and 4 as ever and refuses version 9 as ever; the setters' rules;
refusals with their glcContainerLastError triples; capacity; and range reads with the block counts csrc/dedup_rule.h predicts."""
import os
import struct
import zlib

import numpy as np
import pytest

import container_model as M
import dedup_inputs as I
import dedup_model as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL, UNKNOWN = 2, 9999
N, ROWS = I.N, I.ROWS
CASES = [(0, False), (4, False), (8, True)]


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


_WANT = {}


def _want(elem, delta):
    if (elem, delta) not in _WANT:
        _WANT[elem, delta] = D.write(I.container_input(elem, delta), N, ROWS, elem, delta)
    return _WANT[elem, delta]


def _plan(glc, ctx, elem, delta=False, pipelined=False, dedup=True, n=N, rows=ROWS, codec=1):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if delta:
        glc.container_set_delta(plan, 1)
    if dedup:
        glc.container_set_dedup(plan, 1)
    return plan


# --- 1. dedup on: byte-identical to the model, and read back -------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", CASES)
@pytest.mark.parametrize("pipelined", [False, True])
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, elem, delta, pipelined):
    x, want = I.container_input(elem, delta), _want(elem, delta)
    assert struct.unpack("<HHII", want[4:16]) == (9, 1 if delta else 0, N, elem)
    frames = M.layout(want)["frames"]
    assert [f["nb"] for f in frames] == [ROWS, ROWS, 2, 1] and frames[-1]["blk_len"] == I.TAIL
    assert [k for _, _, k in frames[0]["records"]] == [1, 2, 2, 6, 6, 6, 1, 6] and [k for _, _, k in frames[1]["records"]][:2] == [2, 6]
    s, e, _ = frames[0]["records"][3]
    assert e - s == 4 * (D.mask_words(N) + D.nchunks(N))         # nothing kept: the mask and the refs alone
    with _plan(glc, ctx, elem, delta, pipelined) as plan:
        assert glc.container_get_dedup(plan) == 1
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert c.numel() <= glc.container_bound(x.size, N)
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        assert glc.container_last_error(plan) == (0, -1, -1)
        ch = glc.container_compress_host(plan, x)
        assert ch.tobytes() == want
        assert np.array_equal(glc.container_decompress_host(plan, ch), x)
        src, dst, back = tmp_path / "in.bin", tmp_path / "out.glcb", tmp_path / "back.bin"
        x.tofile(src)
        glc.container_compress_file(plan, str(src), str(dst))
        assert dst.read_bytes() == want
        glc.container_decompress_file(plan, str(dst), str(back))
        assert back.read_bytes() == x.tobytes()
        for L in (0, 1, 513, 2 * N + 1024):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == D.write(y, N, ROWS, elem, delta), L
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused
    assert np.array_equal(D.read(want), x)


def test_frames_larger_than_a_decoder_chunk_and_zeros(glc, ctx, cuda):
    """rows 40 of 1536 bytes: every block of zeros but the first sources chunk 0 of block 0; and pages with rows 40"""
    for x in (np.zeros(100 * 1536 + 700, np.uint8), I.make("pages", 130 * 1536 + 5)):
        want = D.write(x, 1536, 40)
        with _plan(glc, ctx, 0, n=1536, rows=40) as plan:
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        with _plan(glc, ctx, 0, n=1536, rows=3) as plan:          # a reader of fewer rows: several decoder chunks a frame
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(want, np.uint8)))), x)


# --- 2. decoding -----------------------------------------------------------------------------------------------------------
def test_gpu_reads_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "dedup_v9_container.bin"), "rb").read()
    x, kinds = D.read(gold, with_kinds=True)
    assert {1, 2, 6} == set(kinds)
    g = np.frombuffer(gold, np.uint8)
    G = I.GOLDEN
    for n, rows, elem, delta, pipelined in ((G["block_len"], 3, 8, True, False), (G["block_len"], 1, 0, False, True), (300000, 2, 4, True, False)):
        with _plan(glc, ctx, elem, delta, pipelined, n=n, rows=rows) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert glc.container_last_error(plan) == (0, -1, -1)
    with _plan(glc, ctx, 8, True, n=G["block_len"], rows=3) as plan:   # and the writer makes the fixture
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == gold
        assert np.array_equal(glc.container_decompress_host(plan, g), x)


def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_a_plan_with_dedup_off_refuses_version_9_and_writes_versions_3_and_4_as_ever(glc, ctx, cuda):
    import torch
    for elem, delta in CASES:
        x, c9 = I.container_input(elem, delta), _want(elem, delta)
        want = M.write(x, N, ROWS, elem, 1, delta=delta)
        with _plan(glc, ctx, elem, delta, dedup=False) as plan:
            assert glc.container_get_dedup(plan) == 0
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want and struct.unpack("<H", want[4:6])[0] == (4 if delta else 3)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            for mode in (None, glc.container_set_sparse, glc.container_set_ans, glc.container_set_auto):   # every other plan refuses it
                if mode:
                    mode(plan, 1)
                out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
                with pytest.raises(glc.CudppError) as err:
                    _decompress_into(glc, plan, c9, out, x.size)
                assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
                assert bool((out == 0xAB).all())
                if mode:
                    mode(plan, 0)
            glc.container_set_dedup(plan, 1)                     # on: version 9, and the older versions are still read
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == c9
            for older in (c9, want):
                assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(older, np.uint8)))), x)
            glc.container_set_dedup(plan, 0)                     # off again: the old bytes again
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want


# --- 3. the setters --------------------------------------------------------------------------------------------------------
def test_setters(glc, ctx, cuda):
    x = I.container_input(4, False)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plan:
        assert glc.container_get_dedup(plan) == 0
        with pytest.raises(glc.CudppError) as e:                # the codec is the BWT one
            glc.container_set_dedup(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_dedup(plan) == 0
        glc.container_set_dedup(plan, 0)                        # off is always legal
        glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)
        with pytest.raises(glc.CudppError):
            glc.container_set_dedup(plan, 1)
        glc.container_set_codec(plan, 1)
        for bad in (2, 3, 255, 1 << 31):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_dedup(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_dedup(plan) == 0
        for other, get in ((glc.container_set_sparse, glc.container_get_sparse), (glc.container_set_ans, glc.container_get_ans),
                           (glc.container_set_auto, glc.container_get_auto)):
            other(plan, 1)                                      # another order-0 mode is on: refused, nothing changed
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_dedup(plan, 1)
            assert e.value.code == ILLEGAL and glc.container_get_dedup(plan) == 0 and get(plan) == 1
            other(plan, 0)
        glc.container_set_dedup(plan, 1)
        for other, get in ((glc.container_set_sparse, glc.container_get_sparse), (glc.container_set_ans, glc.container_get_ans),
                           (glc.container_set_auto, glc.container_get_auto)):
            with pytest.raises(glc.CudppError) as e:            # and the other way round
                other(plan, 1)
            assert e.value.code == ILLEGAL and get(plan) == 0 and glc.container_get_dedup(plan) == 1
            other(plan, 0)
            assert glc.container_get_dedup(plan) == 1
        for bad in (2, 1 << 31):
            with pytest.raises(glc.CudppError):
                glc.container_set_dedup(plan, bad)
            assert glc.container_get_dedup(plan) == 1           # unchanged
        with pytest.raises(glc.CudppError):                     # a refused codec changes nothing
            glc.container_set_codec(plan, 7)
        assert glc.container_get_dedup(plan) == 1 and glc.container_get_codec(plan) == 1
        glc.container_set_shuffle(plan, 4)                      # the filter settings leave it alone
        glc.container_set_delta(plan, 1)
        glc.container_set_delta(plan, 0)
        assert glc.container_get_dedup(plan) == 1
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(4, False)
        glc.container_set_codec(plan, 0)                        # back to the BWT codec: the mode off, and it stays off
        assert glc.container_get_dedup(plan) == 0
        glc.container_set_codec(plan, 1)
        assert glc.container_get_dedup(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, N, ROWS, 4, 1)
        glc.container_set_dedup(plan, 1)
        glc.container_set_shuffle(plan, 0)
        glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)   # CHOOSE switches it off as well
        assert glc.container_get_dedup(plan) == 0


# --- 4. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", [(0, False), (8, True)])
def test_refusals_of_version_9(glc, ctx, cuda, elem, delta):
    import torch
    x, c9 = I.container_input(elem, delta), _want(elem, delta)
    cases, lay = D.refusal_cases(c9, elem)
    assert len(cases) >= 24
    guard = 64
    with _plan(glc, ctx, elem, delta) as plan:
        for name, cont, want in cases:
            with pytest.raises(M.ContainerError) as merr:          # the model
                D.read(cont)
            assert (merr.value.what, merr.value.frame, merr.value.block) == want, name
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN, name
            assert glc.container_last_error(plan) == want, name
            assert bool((out[x.size:] == 0xAB).all())
        for name, cont, want in cases[::5]:
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want, name
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c9, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_dedup_mode_on(glc, ctx, cuda):
    import torch
    elem, delta = 8, True
    x, need = I.container_input(elem, delta), len(_want(elem, delta))
    with _plan(glc, ctx, elem, delta) as plan:
        for cap in (need - 1, need // 2, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need and _host(c).tobytes() == _want(elem, delta)


def test_timing_with_the_dedup_mode_on(glc, ctx, cuda):
    """the dedup frame is frame_order0's with its own kinds part: with the stage events on, the four marks come in order and the
    bytes are the model's.  The input has kind-6 blocks (frame 0) and a ragged tail frame."""
    x, want = I.container_input(0, False), _want(0, False)
    frames = M.layout(want)["frames"]
    assert 6 in [k for _, _, k in frames[0]["records"]] and frames[-1]["blk_len"] == I.TAIL < N
    with _plan(glc, ctx, 0) as plan:
        plan.enable_timing(1)
        c = glc.container_compress(plan, _gpu(x))
        plan.synchronize()
        assert _host(c).tobytes() == want
        ms = plan.last_timing()
        assert len(ms) == 4 and all(np.isfinite(v) and v >= 0 for v in ms) and sum(ms) > 0
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


# --- 5. range reads ----------------------------------------------------------------------------------------------------------
def _want_blocks(c, a, n):
    """(frames, blocks decoded) of a read of [a, a + n) of the unfiltered container c: the needed blocks of every frame and, in
    front of them, the source-only blocks csrc/dedup_rule.h asks for"""
    frames = blocks = pos = 0
    for fr in M.layout(c)["frames"]:
        nb, bl = fr["nb"], fr["blk_len"]
        lo, hi = max(a, pos), min(a + n, pos + nb * bl)
        if lo < hi:
            T, W = D.frame_tables(c, fr)
            kinds, idx = [r[2] for r in fr["records"]], [int(W[T["bwt"] + b]) for b in range(nb)]
            frames += 1
            blocks += D.blocks_decoded(kinds, idx, (lo - pos) // bl, (hi - 1 - pos) // bl)
        pos += nb * bl
    return frames, blocks


def test_range_reads(glc, ctx, cuda):
    x, c = I.container_input(0, False), _want(0, False)
    F = ROWS * N
    reads = {"inside a kind-6 block whose sources sit three blocks earlier": (4 * N + 600, 3000), "the block of a repeat inside itself": (5 * N + 10, N - 20),
             "nothing kept": (3 * N + 1, 100), "sources in a raw block": (7 * N + 512, 1024), "across a frame edge": (F - 700, 1500),
             "the second frame's repeat of its first block": (F + N + 5, 50), "in the tail": (x.size - 700, 650), "a block without sources": (2 * N, N),
             "everything": (0, x.size)}
    assert _want_blocks(c, *reads["inside a kind-6 block whose sources sit three blocks earlier"]) == (1, 4)
    assert _want_blocks(c, *reads["the block of a repeat inside itself"]) == (1, 1) and _want_blocks(c, *reads["nothing kept"]) == (1, 4)
    assert _want_blocks(c, *reads["across a frame edge"]) == (2, 3) and _want_blocks(c, *reads["in the tail"]) == (1, 1)
    d_c = _gpu(np.frombuffer(c, np.uint8))
    with _plan(glc, ctx, 0) as plan, glc.container_index(plan, d_c) as ix:
        for name, (a, n) in reads.items():
            got = glc.container_read_range(plan, ix, d_c, a, n)
            assert np.array_equal(_host(got), x[a:a + n]), name
            assert glc.container_last_range_stats(plan)[:2] == _want_blocks(c, a, n), name
        hc = np.frombuffer(c, np.uint8)
        a, n = reads["inside a kind-6 block whose sources sit three blocks earlier"]
        out = np.zeros(n, np.uint8)
        glc.container_read_range_host(plan, ix, hc, a, n, out=out)
        assert np.array_equal(out, x[a:a + n]) and glc.container_last_range_stats(plan)[:2] == (1, 4)
    # behind the filters: the bytes (the planes of a range need blocks all over the frame)
    for elem, delta in ((4, False), (8, True)):
        x, c = I.container_input(elem, delta), _want(elem, delta)
        d_c = _gpu(np.frombuffer(c, np.uint8))
        with _plan(glc, ctx, elem, delta) as plan, glc.container_index(plan, d_c) as ix:
            for a, n in ((4 * N + 600, 3000), (F - 700, 1500), (x.size - 700, 650), (0, x.size)):
                assert np.array_equal(_host(glc.container_read_range(plan, ix, d_c, a, n)), x[a:a + n]), (elem, a, n)
    # a damaged source block is caught by the needed block's own crc_raw: frame 0's block 1 is a kind-2 source of block 4
    x, c = I.container_input(0, False), _want(0, False)
    fr = M.layout(c)["frames"][0]
    T = M.tables_layout(fr["nb"], fr["blk_len"])
    y = bytearray(c)
    s, e, _ = fr["records"][1]
    y[e - 12] ^= 0x10                                           # among the last symbols: the short last chunk, which block 4 copies
    o = fr["tables"][0] + 4 * (T["crc_rec"] + 1)
    y[o:o + 4] = struct.pack("<I", zlib.crc32(bytes(y[s:e])))
    bad = M.retable(bytes(y), fr["start"])
    d_b = _gpu(np.frombuffer(bad, np.uint8))
    with _plan(glc, ctx, 0) as plan, glc.container_index(plan, d_b) as ix:
        with pytest.raises(glc.CudppError):
            glc.container_read_range(plan, ix, d_b, 4 * N + 600, 3000)
        assert glc.container_last_error(plan)[:2] == (4, 0)
        assert np.array_equal(_host(glc.container_read_range(plan, ix, d_b, 2 * N, N)), x[2 * N:3 * N])
