"""Filter-lag of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points write the bytes of
the Python model of format version 13 (tests/filter_lag_model.py), pipelining off and on, for the mixed stream of
tests/filter_lag_inputs.py (stereo audio, text, an 8-channel ADC dump, int64 timestamps, xyz points, float32 and a ragged tail), which
is the golden fixture, and read them back; glcContainerLastFilters and glcContainerLastLagFilters agree with the model; the model's
forced-pick containers decode; every refusal case answers the model's triple; version 13 is refused by every plan without the
setting; the plan with it on reads the older fixtures; index and range reads inside and across lag frames; the setter's rules."""
import os
import struct

import numpy as np
import pytest

import container_model as M
import filter_auto_model as F
import filter_lag_inputs as FI
import filter_lag_model as FL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GOLDEN, "filter_lag_v13_container.bin")
UNKNOWN = 9999


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


@pytest.fixture(scope="module")
def mixed():
    x = FI.mixed_stream()
    return x, FL.write(x, FI.N, FI.ROWS), FL.picks_of(x, FI.N, FI.ROWS)


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


def _plan(glc, ctx, pipelined=False, rows=FI.ROWS, on=True, n=FI.N):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_filter_auto(plan, 1)
    if on:
        glc.container_set_filter_lag(plan, 1)
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
    assert want == open(GOLD, "rb").read() and picks[:6] == [p for _, p in FI.FRAMES]
    assert struct.unpack("<HHII", want[4:16]) == (13, 0, FI.N, 0)
    with _plan(glc, ctx, pipelined) as plan:
        assert glc.container_get_filter_lag(plan) == 1 and glc.container_last_lag_filters(plan) == (0,) * 4
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert glc.container_last_filters(plan) == FL.last_filters(picks) == (1, 0, 0, 1, 0, 0, 0, 7)
        assert glc.container_last_lag_filters(plan) == FL.last_lag_filters(picks) == (2, 2, 1, 5)
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
        for L in (0, 1, 7, 8, 9, 31, FI.N + 9):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == FL.write(y, FI.N, FI.ROWS), L
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused


def test_misaligned_input(glc, ctx, cuda):
    """the frame is probed where it lies: an input 3 bytes off a 16-byte boundary, and frames of 3 * 4099 bytes behind it"""
    x = FI.mixed_stream()[:7 * 4099 + 50]
    want = FL.write(x, 4099, 3)
    buf = _gpu(np.concatenate([np.zeros(3, np.uint8), x]))
    with _plan(glc, ctx, rows=3, n=4099) as plan:
        c = glc.container_compress(plan, buf[3:])
        assert _host(c).tobytes() == want
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)


def test_forced_picks_decode(glc, ctx, cuda):
    """what the writer never makes and the reader takes: (8, lag 16, fold 0), (4, lag 3, fold 0), and (2, lag 16, fold 1), a plain
    delta and a plain shuffle beside them; a frame shorter than `lag` elements"""
    x = FI.mixed_stream()[:3 * FI.FRAME + 77]
    with _plan(glc, ctx) as plan:
        for picks in ([(8, 1, 16, 0), (2, 1, 16, 1), (4, 1, 3, 0), (1, 0, 1, 0)], [(4, 1, 1, 0), (8, 0, 1, 0), (2, 1, 5, 0), (8, 1, 16, 1)]):
            c = FL.write(x, FI.N, FI.ROWS, picks=picks)
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
            assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(c, np.uint8)), x)
        y = x[:31]
        c = FL.write(y, FI.N, FI.ROWS, picks=[(8, 1, 16, 1)])
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), y)


# --- 2. the other plans, and the older versions -----------------------------------------------------------------------------
def test_version_13_is_refused_without_the_setting(glc, ctx, cuda, tmp_path, mixed):
    import torch
    x, c13, _ = mixed
    src = tmp_path / "c13.glcb"
    src.write_bytes(c13)

    def default(plan):
        pass

    def v10(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)

    def v11(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_shuffle(plan, 2)
        glc.container_set_delta(plan, 1)
        glc.container_set_delta_lag(plan, 2, 1)

    def v12(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_shuffle(plan, 4)
        glc.container_set_delta(plan, 1)
        glc.container_set_delta_grid(plan, 64, 1)

    for setup in (default, v10, v11, v12):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, FI.N, rows=FI.ROWS) as plan:
            setup(plan)
            assert glc.container_get_filter_lag(plan) == 0
            out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, c13, out, x.size)
            assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
            assert bool((out == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(c13, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_file(plan, str(src), str(tmp_path / "back.bin"))
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_index(plan, _gpu(np.frombuffer(c13, np.uint8)))
            assert glc.container_last_error(plan) == (1, -1, -1)


def test_the_plan_with_the_setting_on_reads_the_older_fixtures(glc, ctx, cuda):
    names = ("container_v1.bin", "container_v2_f32.bin", "container_v3_mixed.bin", "container_v4_series.bin", "container_v5_sparse.bin",
             "container_v7_ans.bin", "container_v8_auto.bin", "filter_auto_v10_container.bin")
    with _plan(glc, ctx, rows=8, n=1 << 16) as plan:
        for name in names:
            g = np.fromfile(os.path.join(GOLDEN, name), np.uint8)
            want = FL.read(g.tobytes())
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), want), name
            assert glc.container_last_error(plan) == (0, -1, -1)


# --- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_of_version_13(glc, ctx, cuda, tmp_path, mixed):
    import torch
    x, c13, _ = mixed
    cases, _ = FL.refusal_cases(c13)
    assert len(cases) >= 24
    path = tmp_path / "bad.glcb"

    def lag11(plan):
        glc.container_set_filter_auto(plan, 0)
        glc.container_set_shuffle(plan, 2)
        glc.container_set_delta(plan, 1)
        glc.container_set_delta_lag(plan, 2, 1)

    with _plan(glc, ctx) as on_plan, _plan(glc, ctx, on=False) as v10_plan, _plan(glc, ctx, on=False) as v11_plan, \
            _plan(glc, ctx, on=False) as auto_plan, glc.Plan(ctx, glc.CUDPP_COMPRESS, FI.N, rows=FI.ROWS) as plain_plan:
        lag11(v11_plan)
        glc.container_set_filter_auto(auto_plan, 0)
        for name, cont, want, reads in cases:
            plan = (on_plan if "filter_lag" in reads else v10_plan if "filter" in reads else v11_plan if "lag" in reads else
                    auto_plan if "auto" in reads else plain_plan)
            out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN, name
            assert glc.container_last_error(plan) == want, name
            assert bool((out[x.size:] == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want, name
            path.write_bytes(cont)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_file(plan, str(path), str(tmp_path / "back.bin"))
            assert glc.container_last_error(plan) == want, name
            if want[0] in (M.STREAM_HEADER, M.TRUNCATED) or (want[0] == M.FRAME_TABLE and want[2] == -1 and "CRC not" not in name):
                with pytest.raises(glc.CudppError):                # what the headers alone show, the index walks refuse alike
                    glc.container_index(plan, _gpu(np.frombuffer(cont, np.uint8)))
                assert glc.container_last_error(plan) == want, name
                with pytest.raises(glc.CudppError):
                    glc.container_index_host(plan, np.frombuffer(cont, np.uint8))
                assert glc.container_last_error(plan) == want, name
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c13, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


# --- 4. index and range reads --------------------------------------------------------------------------------------------------
def test_range_reads(glc, ctx, cuda, tmp_path, mixed):
    x, want, _ = mixed
    Fr = FI.FRAME
    frames = [(FI.ROWS, FI.N)] * 6 + [(1, FI.TAIL)]
    words = F.frame_words(want)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(3000, 100), (2 * Fr + 5000, 2000),                  # inside one lag frame (lag 2; lag 8)
              (2 * Fr + 2 * 2048 + 6, 50), (4 * Fr + 4 * 2049 + 1, 9),   # starting off a 2048-element boundary
              (3 * Fr - 100, 300), (4 * Fr - 7, 30),               # across two frames of different lag (8 and 1; 1 and 3)
              (Fr - 10, 20), (5 * Fr - 5000, 10000),               # a lag frame and an unfiltered or shuffled one
              (6 * Fr - 5, FI.TAIL), (6 * Fr + FI.TAIL - 1, 1), (77, 1),      # into the tail; 1 byte
              (0, x.size), (x.size, 0)]
    with _plan(glc, ctx) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, FI.N, 7, 13, 0, 0)        # what the stream header says
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                assert glc.container_last_range_stats(plan)[:2] == FL.range_stats(frames, words, off, cnt), (off, cnt)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            for off, cnt in ranges[:8]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
                assert glc.container_last_range_stats(plan)[:2] == FL.range_stats(frames, words, off, cnt), (off, cnt)
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[4], ranges[8]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_filter_lag(plan, 0)                  # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)


# --- 5. the setter -------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda, mixed):
    x, want13, _ = mixed
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, FI.N, rows=FI.ROWS) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        def on():
            glc.container_set_codec(plan, 1)
            glc.container_set_auto(plan, 1)
            glc.container_set_filter_auto(plan, 1)
            glc.container_set_filter_lag(plan, 1)

        get = lambda: glc.container_get_filter_lag(plan)
        assert get() == 0
        assert refused(glc.container_set_filter_lag, 1) and get() == 0             # no filter-auto: the BWT codec
        glc.container_set_filter_lag(plan, 0)                                     # off is always legal
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        assert refused(glc.container_set_filter_lag, 1) and get() == 0             # the auto mode alone is not filter-auto
        glc.container_set_filter_auto(plan, 1)
        for bad in (2, 3, 1 << 31):
            assert refused(glc.container_set_filter_lag, bad) and get() == 0
        glc.container_set_filter_lag(plan, 1)
        assert get() == 1 and glc.container_get_filter_auto(plan) == 1
        assert refused(glc.container_set_filter_lag, 2) and get() == 1             # unchanged
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want13
        glc.container_set_filter_auto(plan, 0)                                    # filter-auto off: off with it
        assert get() == 0
        glc.container_set_filter_auto(plan, 1)
        assert get() == 0                                                         # and it stays off
        on()
        glc.container_set_auto(plan, 0)
        assert get() == 0 and glc.container_get_filter_auto(plan) == 0
        on()
        glc.container_set_codec(plan, 0)                                          # a codec change
        assert get() == 0
        on()
        glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)
        assert get() == 0
        on()
        glc.container_set_filter_lag(plan, 0)                                     # with it off: version 10's bytes for the same input
        assert get() == 0 and glc.container_get_filter_auto(plan) == 1
        c10 = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c10 == F.write(x, FI.N, FI.ROWS) and glc.container_last_lag_filters(plan) == (0, 0, 0, 0)
        assert struct.unpack("<H", c10[4:6])[0] == 10
