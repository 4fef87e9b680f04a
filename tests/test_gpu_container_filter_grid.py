"""Filter-grid of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points write the bytes of
the Python model of format version 14 (tests/filter_grid_model.py), pipelining off and on, for the mixed stream of
tests/filter_grid_inputs.py (an image 640 wide, text, an int32 walk 300 wide, an 8-channel ADC dump, int64 timestamps and a ragged
tail; frames of 4 x 64 KiB), which is the golden fixture -- the model needs a minute for its rule, so the expected bytes and picks
are the fixture's -- and read them back; the three reports agree with the model; small and misaligned inputs equal the model's
rule; the model's forced-pick containers (fold 0 and the largest width among them) decode; every refusal case answers the model's
triple; version 14 is refused by every plan without the setting; index and range reads, one starting mid-band in a grid frame; with
the setting off the bytes are the version-13 fixture's; the setter's rules."""
import os
import struct

import numpy as np
import pytest

import container_model as M
import filter_auto_model as F
import filter_grid_inputs as QI
import filter_grid_model as Q
import filter_lag_inputs as FI
import grid_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GOLDEN, "filter_grid_v14_container.bin")
GOLD13 = os.path.join(GOLDEN, "filter_lag_v13_container.bin")
UNKNOWN = 9999


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


@pytest.fixture(scope="module")
def mixed():
    """(the stream, the fixture, the picks its frame words name)"""
    x = QI.mixed_stream()
    want = open(GOLD, "rb").read()
    picks = [Q.word_format(w) for w in F.frame_words(want)]
    assert picks == [p for _, p in QI.FRAMES] + [QI.TAIL_PICK] and np.array_equal(Q.read(want), x)
    return x, want, picks


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


def _plan(glc, ctx, pipelined=False, rows=QI.ROWS, on=True, n=QI.N, lag=True):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_filter_auto(plan, 1)
    if lag:
        glc.container_set_filter_lag(plan, 1)
    if on:
        glc.container_set_filter_grid(plan, 1)
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
    assert struct.unpack("<HHII", want[4:16]) == (14, 0, QI.N, 0)
    with _plan(glc, ctx, pipelined) as plan:
        assert glc.container_get_filter_grid(plan) == 1 and glc.container_last_grid_filters(plan) == (0,) * 4
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert glc.container_last_filters(plan) == Q.last_filters(picks) == (1, 0, 0, 0, 0, 0, 0, 6)
        assert glc.container_last_lag_filters(plan) == Q.last_lag_filters(picks) == (1, 1, 1, 3)
        assert glc.container_last_grid_filters(plan) == Q.last_grid_filters(picks) == (1, 1, 0, 2)
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
    """lengths around the first byte the probes count and the first element size with a grid candidate; then the frame is probed
    where it lies: an input 3 bytes off a 16-byte boundary in frames of 3 * 4099 bytes, each about 30 rows of a walk 100 wide"""
    x = QI.mixed_stream()
    with _plan(glc, ctx) as plan:
        for L in (0, 1, 7, 8, 9, 31, 2047, 2048, 4103):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == Q.write(y, QI.N, QI.ROWS), L
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
    y = grid_inputs.grid_bytes("walk32", 5 * 3 * 4099 + 50, 100)
    want = Q.write(y, 4099, 3)
    assert sum(1 for w in F.frame_words(want) if w & Q.WORD_GRID) >= 4
    buf = _gpu(np.concatenate([np.zeros(3, np.uint8), y]))
    with _plan(glc, ctx, rows=3, n=4099) as plan:
        c = glc.container_compress(plan, buf[3:])
        assert _host(c).tobytes() == want
        assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


def test_forced_picks_decode(glc, ctx, cuda):
    """what the writer never makes and the reader takes: grid words with fold 0, the widths 2 and 65536, a width larger than the
    frame; lag, delta and shuffle frames beside them"""
    n, rows = FI.N, FI.ROWS
    x = QI.mixed_stream()[:4 * n * rows + 77]
    with _plan(glc, ctx, n=n, rows=rows) as plan:
        for picks in ([(2, 1, 1, 0, 640), (4, 1, 1, 1, 65536), (8, 1, 1, 0, 2), (1, 0, 1, 0, 0), (2, 1, 1, 1, 2)],
                      [(8, 1, 1, 1, 100), (2, 1, 5, 0, 0), (4, 1, 1, 0, 63), (4, 0, 1, 0, 0), (8, 1, 16, 1, 0)]):
            c = Q.write(x, n, rows, picks=picks)
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
            assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(c, np.uint8)), x)


# --- 2. the other plans, and the older versions -----------------------------------------------------------------------------
def test_the_setting_off_writes_the_version_13_fixture(glc, ctx, cuda):
    x = FI.mixed_stream()
    want = open(GOLD13, "rb").read()
    with _plan(glc, ctx, on=False, n=FI.N, rows=FI.ROWS) as plan:
        assert glc.container_get_filter_grid(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
        assert glc.container_last_grid_filters(plan) == (0, 0, 0, 0)
    with _plan(glc, ctx, n=FI.N, rows=FI.ROWS) as plan:            # and the plan with it on reads that fixture
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(want, np.uint8)))), x)


def test_the_plan_with_the_setting_on_reads_the_older_fixtures(glc, ctx, cuda):
    names = ("container_v1.bin", "container_v2_f32.bin", "container_v3_mixed.bin", "container_v4_series.bin", "container_v5_sparse.bin",
             "container_v7_ans.bin", "container_v8_auto.bin", "filter_auto_v10_container.bin", "filter_lag_v13_container.bin")
    with _plan(glc, ctx, rows=8, n=1 << 16) as plan:
        for name in names:
            g = np.fromfile(os.path.join(GOLDEN, name), np.uint8)
            want = Q.read(g.tobytes())
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), want), name
            assert glc.container_last_error(plan) == (0, -1, -1)


# --- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_of_version_14(glc, ctx, cuda, tmp_path, mixed):
    import torch
    x, c14, _ = mixed
    cases, _ = Q.refusal_cases(c14)
    assert len(cases) >= 30
    path = tmp_path / "bad.glcb"

    def grid12(plan):
        glc.container_set_filter_auto(plan, 0)
        glc.container_set_shuffle(plan, 4)
        glc.container_set_delta(plan, 1)
        glc.container_set_delta_grid(plan, 64, 1)

    with _plan(glc, ctx) as on_plan, _plan(glc, ctx, on=False) as v13_plan, _plan(glc, ctx, on=False, lag=False) as v10_plan, \
            _plan(glc, ctx, on=False, lag=False) as v12_plan, glc.Plan(ctx, glc.CUDPP_COMPRESS, QI.N, rows=QI.ROWS) as plain_plan:
        grid12(v12_plan)
        for name, cont, want, reads in cases:
            plan = (on_plan if "filter_grid" in reads else v13_plan if "filter_lag" in reads else v10_plan if "filter" in reads else
                    v12_plan if "grid" in reads else plain_plan)
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
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c14, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


# --- 4. index and range reads --------------------------------------------------------------------------------------------------
def test_range_reads(glc, ctx, cuda, tmp_path, mixed):
    x, want, _ = mixed
    Fr = QI.FRAME
    frames = [(QI.ROWS, QI.N)] * 5 + [(1, QI.TAIL)]
    words = F.frame_words(want)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    # the image's band is 2048 * 10 elements = 40960 bytes, the walk's 2048 * 5 elements = 40960 bytes
    ranges = [(3000, 100), (50000, 3000), (2 * Fr + 45000, 100),   # inside a grid frame: in its first band; starting mid-band
              (2 * 40960 - 1, 2), (2 * Fr + 3 * 40960 - 3, 40966),  # across a band's edge; a whole band and a bit on both sides
              (Fr - 10, 20), (2 * Fr - 100, 300), (3 * Fr - 7, 30),  # across a grid frame and text, text and a grid frame, a grid and a lag frame
              (4 * Fr - 5000, 10000), (5 * Fr - 5, QI.TAIL), (5 * Fr + QI.TAIL - 1, 1), (77, 1),
              (0, x.size), (x.size, 0)]
    with _plan(glc, ctx) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, QI.N, 6, 14, 0, 0)        # what the stream header says
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                assert glc.container_last_range_stats(plan)[:2] == Q.range_stats(frames, words, off, cnt), (off, cnt)
        assert Q.range_stats(frames, words, 50000, 3000) == (1, 2) and Q.range_stats(frames, words, 2 * Fr + 45000, 100) == (1, 4)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            for off, cnt in ranges[:8]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
                assert glc.container_last_range_stats(plan)[:2] == Q.range_stats(frames, words, off, cnt), (off, cnt)
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[1], ranges[9]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_filter_grid(plan, 0)                 # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)


# --- 5. the setter -------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, QI.N, rows=QI.ROWS) as plan:
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

        get = lambda: glc.container_get_filter_grid(plan)
        assert get() == 0
        assert refused(glc.container_set_filter_grid, 1) and get() == 0            # no filter-lag: the BWT codec
        glc.container_set_filter_grid(plan, 0)                                    # off is always legal
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        assert refused(glc.container_set_filter_grid, 1) and get() == 0            # filter-auto alone is not filter-lag
        glc.container_set_filter_lag(plan, 1)
        for bad in (2, 3, 1 << 31):
            assert refused(glc.container_set_filter_grid, bad) and get() == 0
        glc.container_set_filter_grid(plan, 1)
        assert get() == 1 and glc.container_get_filter_lag(plan) == 1 and glc.container_get_filter_auto(plan) == 1
        assert refused(glc.container_set_filter_grid, 2) and get() == 1            # unchanged
        glc.container_set_filter_lag(plan, 0)                                     # filter-lag off: off with it
        assert get() == 0
        glc.container_set_filter_lag(plan, 1)
        assert get() == 0                                                         # and it stays off
        for off in (lambda: glc.container_set_filter_auto(plan, 0), lambda: glc.container_set_auto(plan, 0), lambda: glc.container_set_codec(plan, 0),
                    lambda: glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)):
            on()
            assert get() == 1
            off()
            assert get() == 0 and glc.container_get_filter_lag(plan) == 0
