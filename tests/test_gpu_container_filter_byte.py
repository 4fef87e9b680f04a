"""Filter-byte of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points write the bytes of
the Python model of format version 16 (tests/filter_byte_model.py), pipelining off and on, for the mixed stream of
tests/filter_byte_inputs.py (a greyscale image 721 wide, text, an RGB image 427 wide, a 12-bit image 640 wide, 8-bit stereo, int64
timestamps and a ragged tail; frames of 4 x 64 KiB), which is the golden fixture -- the model needs minutes for its rule, so the
expected bytes and picks are the fixture's -- and read them back; the four reports agree with the model; small and misaligned inputs
equal the model's rule; the model's forced-pick containers (lag 16, strides 65536 and 2, a byte frame next to a grid frame) decode;
every refusal case answers the model's triple; version 16 is refused by every plan without the setting and version 15 by a plan
with it; index and range reads, one starting mid-band in a byte frame; with the setting off the bytes are the version-14 fixture's;
the setter's rules."""
import os
import struct

import numpy as np
import pytest

import byte_delta_inputs as BI
import byte_delta_model as BD
import container_model as M
import filter_auto_model as F
import filter_byte_inputs as BFI
import filter_byte_model as B
import filter_grid_inputs as QI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GOLDEN, "filter_byte_v16_container.bin")
GOLD14 = os.path.join(GOLDEN, "filter_grid_v14_container.bin")
UNKNOWN = 9999


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


@pytest.fixture(scope="module")
def mixed():
    """(the stream, the fixture, the picks its frame words name)"""
    x = BFI.mixed_stream()
    want = open(GOLD, "rb").read()
    picks = [B.word_format(w) for w in F.frame_words(want)]
    assert picks[:6] == [p for _, p in BFI.FRAMES] and len(picks) == 7 and np.array_equal(B.read(want), x)
    return x, want, picks


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


def _plan(glc, ctx, pipelined=False, rows=BFI.ROWS, on=True, n=BFI.N, grid=True, lag=True):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_filter_auto(plan, 1)
    if lag:
        glc.container_set_filter_lag(plan, 1)
    if lag and grid:
        glc.container_set_filter_grid(plan, 1)
    if lag and grid and on:
        glc.container_set_filter_byte(plan, 1)
    return plan


def _byte_plan(glc, ctx, lag=1, stride=0, rows=BFI.ROWS, n=BFI.N):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_byte_delta(plan, lag, stride)
    return plan


def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


# --- 1. the setting on: the fixture's bytes from all six entry points, and read back -----------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_mixed_stream_on_all_entry_points(glc, ctx, cuda, tmp_path, mixed, pipelined):
    x, want, picks = mixed
    assert struct.unpack("<HHII", want[4:16]) == (16, 0, BFI.N, 0)
    with _plan(glc, ctx, pipelined) as plan:
        assert glc.container_get_filter_byte(plan) == 1 and glc.container_last_byte_filters(plan) == (0,) * 3
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert glc.container_last_filters(plan) == B.last_filters(picks)
        assert glc.container_last_lag_filters(plan) == B.last_lag_filters(picks)
        assert glc.container_last_grid_filters(plan) == B.last_grid_filters(picks) == (1, 0, 0, 1)
        assert glc.container_last_byte_filters(plan) == B.last_byte_filters(picks)
        assert B.last_filters(picks)[7] == 7 and B.last_filters(picks)[0] == 1 and B.last_byte_filters(picks)[2] >= 3
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
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused


def test_small_and_misaligned_inputs_equal_the_models_rule(glc, ctx, cuda):
    """lengths around the first byte the probes count and the first length with a byte candidate; then the frame is probed where
    it lies: an input 3 bytes off a 16-byte boundary in frames of 3 * 4099 bytes, each about 120 rows of a greyscale image 100
    wide"""
    x = BFI.mixed_stream()
    with _plan(glc, ctx) as plan:
        for L in (0, 1, 7, 8, 9, 1023, 1024, 4103):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == B.write(y, BFI.N, BFI.ROWS), L
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
    y = BI.grey8(5 * 3 * 4099 + 50, 100)
    want = B.write(y, 4099, 3)
    assert sum(1 for w in F.frame_words(want) if B.is_byte_word(w)) >= 4
    buf = _gpu(np.concatenate([np.zeros(3, np.uint8), y]))
    with _plan(glc, ctx, rows=3, n=4099) as plan:
        c = glc.container_compress(plan, buf[3:])
        assert _host(c).tobytes() == want
        assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


def test_forced_picks_decode(glc, ctx, cuda):
    """what the writer never makes and the reader takes: byte words with lag 16, the strides 65536, 2 and 16, a stride larger than
    the frame; a byte frame next to a grid frame, lag, delta and shuffle frames beside them"""
    n, rows = 8192, 4
    x = BFI.mixed_stream()[BFI.FRAME - 2 * n * rows:BFI.FRAME + 3 * n * rows + 77]
    with _plan(glc, ctx, n=n, rows=rows) as plan:
        for picks in ([(1, 1, 16, 0, 0), (1, 1, 1, 0, 65536), (1, 1, 3, 0, 2), (2, 1, 1, 1, 640), (1, 1, 4, 0, 16), (1, 0, 1, 0, 0)],
                      [(2, 1, 1, 0, 640), (1, 1, 16, 0, 65536), (8, 1, 16, 1, 0), (1, 1, 1, 0, 721), (4, 0, 1, 0, 0), (1, 1, 7, 0, 1281)]):
            c = B.write(x, n, rows, picks=picks)
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
            assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(c, np.uint8)), x)


# --- 2. the other plans, and the older versions -----------------------------------------------------------------------------
def test_the_setting_off_writes_the_version_14_fixture(glc, ctx, cuda):
    x = QI.mixed_stream()
    want = open(GOLD14, "rb").read()
    with _plan(glc, ctx, on=False, n=QI.N, rows=QI.ROWS) as plan:
        assert glc.container_get_filter_byte(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
        assert glc.container_last_byte_filters(plan) == (0, 0, 0)
    with _plan(glc, ctx, n=QI.N, rows=QI.ROWS) as plan:            # and the plan with it on reads that fixture
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(want, np.uint8)))), x)


def test_the_plan_with_the_setting_on_reads_the_older_fixtures_and_refuses_version_15(glc, ctx, cuda):
    names = ("container_v1.bin", "container_v2_f32.bin", "container_v3_mixed.bin", "container_v4_series.bin", "container_v5_sparse.bin",
             "container_v7_ans.bin", "container_v8_auto.bin", "filter_auto_v10_container.bin", "filter_lag_v13_container.bin",
             "filter_grid_v14_container.bin")
    y = BI.grey8(40000, 300)
    c15 = BD.write(y, 8192, 4, 1, 300)
    with _plan(glc, ctx, rows=8, n=1 << 16) as plan:
        for name in names:
            g = np.fromfile(os.path.join(GOLDEN, name), np.uint8)
            want = B.read(g.tobytes())
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), want), name
            assert glc.container_last_error(plan) == (0, -1, -1)
        with pytest.raises(glc.CudppError):
            glc.container_decompress(plan, _gpu(np.frombuffer(c15, np.uint8)))
        assert glc.container_last_error(plan) == (M.STREAM_HEADER, -1, -1)
    with _byte_plan(glc, ctx, 1, 300, n=8192) as plan:             # (the byte-delta plan reads it)
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c15, np.uint8)))), y)


# --- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_of_version_16(glc, ctx, cuda, tmp_path, mixed):
    import torch
    x, c16, _ = mixed
    cases, _ = B.refusal_cases(c16)
    assert len(cases) >= 30
    path = tmp_path / "bad.glcb"
    with _plan(glc, ctx) as on_plan, _plan(glc, ctx, on=False) as v14_plan, _plan(glc, ctx, grid=False) as v13_plan, \
            _plan(glc, ctx, lag=False) as v10_plan, _byte_plan(glc, ctx, 1, 721) as v15_plan, \
            glc.Plan(ctx, glc.CUDPP_COMPRESS, BFI.N, rows=BFI.ROWS) as plain_plan:
        for name, cont, want, reads in cases:
            plan = (on_plan if "filter_byte" in reads else v14_plan if "filter_grid" in reads else v13_plan if "filter_lag" in reads else
                    v10_plan if "filter" in reads else v15_plan if "byte" in reads else plain_plan)
            out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN, name
            assert glc.container_last_error(plan) == want, name
            assert bool((out[x.size:] == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want, name
            if want[0] in (M.STREAM_HEADER, M.TRUNCATED) or (want[0] == M.FRAME_TABLE and want[2] == -1 and "CRC not" not in name):
                path.write_bytes(cont)
                with pytest.raises(glc.CudppError):
                    glc.container_decompress_file(plan, str(path), str(tmp_path / "back.bin"))
                assert glc.container_last_error(plan) == want, name
                with pytest.raises(glc.CudppError):                # what the headers alone show, the index walks refuse alike
                    glc.container_index(plan, _gpu(np.frombuffer(cont, np.uint8)))
                assert glc.container_last_error(plan) == want, name
                with pytest.raises(glc.CudppError):
                    glc.container_index_host(plan, np.frombuffer(cont, np.uint8))
                assert glc.container_last_error(plan) == want, name
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c16, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


# --- 4. index and range reads --------------------------------------------------------------------------------------------------
def test_range_reads(glc, ctx, cuda, tmp_path, mixed):
    x, want, _ = mixed
    Fr = BFI.FRAME
    frames = [(BFI.ROWS, BFI.N)] * 6 + [(1, BFI.TAIL)]
    words = F.frame_words(want)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    # grey8's band is 2048 * 12 = 24576 bytes, rgb8's 2048 * 21 = 43008 bytes, stereo8 has runs of 2048 bytes
    assert BD.step(721) == 24576 and BD.step(1281) == 43008 and BD.step(0) == 2048
    ranges = [(3000, 100), (30000, 3000), (2 * Fr + 50000, 100),   # inside a byte frame: in its first band; starting mid-band
              (2 * 24576 - 1, 2), (2 * Fr + 3 * 43008 - 3, 43014),  # across a band's edge; a whole band and a bit on both sides
              (4 * Fr + 5000, 10), (4 * Fr + 2047, 2),             # the stereo frame: mid-run; across a run's edge
              (Fr - 10, 20), (2 * Fr - 100, 300), (3 * Fr - 7, 30), (4 * Fr - 9, 20), (5 * Fr - 5000, 10000),   # across frames of different filters
              (6 * Fr - 5, BFI.TAIL), (6 * Fr + BFI.TAIL - 1, 1), (77, 1), (0, x.size), (x.size, 0)]
    with _plan(glc, ctx) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, BFI.N, 7, 16, 0, 0)       # what the stream header says
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                assert glc.container_last_range_stats(plan)[:2] == B.range_stats(frames, words, off, cnt), (off, cnt)
        assert B.range_stats(frames, words, 30000, 3000) == (1, 1) and B.range_stats(frames, words, 2 * Fr + 50000, 100) == (1, 1)
        assert B.range_stats(frames, words, 2 * Fr + 3 * 43008 - 3, 43014) == (1, 2)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            for off, cnt in ranges[:9]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
                assert glc.container_last_range_stats(plan)[:2] == B.range_stats(frames, words, off, cnt), (off, cnt)
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[1], ranges[11]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_filter_byte(plan, 0)                 # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)


# --- 5. the setter -------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, BFI.N, rows=BFI.ROWS) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        def on():
            glc.container_set_codec(plan, 1)
            glc.container_set_auto(plan, 1)
            glc.container_set_filter_auto(plan, 1)
            glc.container_set_filter_lag(plan, 1)
            glc.container_set_filter_grid(plan, 1)
            glc.container_set_filter_byte(plan, 1)

        get = lambda: glc.container_get_filter_byte(plan)
        assert get() == 0
        assert refused(glc.container_set_filter_byte, 1) and get() == 0            # no filter-grid: the BWT codec
        glc.container_set_filter_byte(plan, 0)                                    # off is always legal
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        glc.container_set_filter_lag(plan, 1)
        assert refused(glc.container_set_filter_byte, 1) and get() == 0            # filter-lag alone is not filter-grid
        glc.container_set_filter_grid(plan, 1)
        for bad in (2, 3, 1 << 31):
            assert refused(glc.container_set_filter_byte, bad) and get() == 0
        glc.container_set_filter_byte(plan, 1)
        assert get() == 1 and glc.container_get_filter_grid(plan) == 1 and glc.container_get_filter_lag(plan) == 1
        assert refused(glc.container_set_filter_byte, 2) and get() == 1            # unchanged
        assert refused(glc.container_set_byte_delta, 1, 721) and get() == 1        # the byte-delta setting stays exclusive with filter-auto
        assert glc.container_get_byte_delta(plan) == (0, 0)
        glc.container_set_filter_grid(plan, 0)                                    # filter-grid off: off with it
        assert get() == 0
        glc.container_set_filter_grid(plan, 1)
        assert get() == 0                                                         # and it stays off
        for off in (lambda: glc.container_set_filter_lag(plan, 0), lambda: glc.container_set_filter_auto(plan, 0),
                    lambda: glc.container_set_auto(plan, 0), lambda: glc.container_set_codec(plan, 0),
                    lambda: glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)):
            on()
            assert get() == 1
            off()
            assert get() == 0 and glc.container_get_filter_grid(plan) == 0
