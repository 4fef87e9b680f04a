"""The delta-lag setting of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points write the
bytes of the Python model of format version 11 (tests/lag_model.py) and read them back; the golden fixture decodes; every refusal
case comes back with the model's class and frame; (1, 0) and a plan that never touched the setting write the older versions byte for
byte; the setter's rules; the index reports the version and flags and range reads give the input's slices; the ratio conditions."""
import os
import struct
import sys

import numpy as np
import pytest

import auto_model as U
import container_model as M
import filter_auto_inputs as FI
import filter_auto_model as F
import lag_inputs as LI
import lag_model as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lag_v11_container.bin")
ILLEGAL, UNKNOWN = 2, 9999
N, ROWS = 16384, 4
LENGTH = 5 * N * ROWS // 2                                        # 2.5 frames
TRIPLES = (("stereo16", 2, 2, 1), ("xyz32", 4, 3, 0), ("i32x4", 4, 4, 1))     # (input, elem, lag, fold)

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_lag_v11_gold as gold  # noqa: E402


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


def _plan(glc, ctx, elem=2, lag=1, fold=0, n=N, rows=ROWS, pipelined=False):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_delta(plan, 1)
    glc.container_set_delta_lag(plan, lag, fold)
    return plan


def _decodes_everywhere(glc, plan, cont, x, tmp_path):
    g = np.frombuffer(cont, np.uint8)
    assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
    assert glc.container_last_error(plan) == (0, -1, -1)
    assert np.array_equal(glc.container_decompress_host(plan, g), x)
    src, back = tmp_path / "c.glcb", tmp_path / "back.bin"
    src.write_bytes(cont)
    glc.container_decompress_file(plan, str(src), str(back))
    assert back.read_bytes() == x.tobytes()


# --- 1. small frames: the model's bytes, and read back ------------------------------------------------------------------------
@pytest.mark.parametrize("kind,elem,lag,fold", TRIPLES)
def test_gpu_container_equals_the_models(glc, ctx, cuda, tmp_path, kind, elem, lag, fold):
    x = LI.lag_bytes(kind, LENGTH)
    want = G.write(x, N, ROWS, elem, lag, fold)
    assert struct.unpack("<HHII", want[4:16]) == (11, G.flags_of(lag, fold), N, elem)
    for pipelined in (False, True):
        with _plan(glc, ctx, elem, lag, fold, pipelined=pipelined) as plan:
            assert glc.container_get_delta_lag(plan) == (lag, fold)
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want
            assert glc.container_compress_host(plan, x).tobytes() == want
            src, dst = tmp_path / "in.bin", tmp_path / "out.glcb"
            x.tofile(src)
            glc.container_compress_file(plan, str(src), str(dst))
            assert dst.read_bytes() == want
            _decodes_everywhere(glc, plan, want, x, tmp_path)
            for L in (0, 1, elem * lag - 1, N + 9):
                y = x[:L]
                c = glc.container_compress(plan, _gpu(y))
                assert _host(c).tobytes() == G.write(y, N, ROWS, elem, lag, fold)
                assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


def test_lag_and_fold_come_from_the_stream_header_not_the_plan(glc, ctx, cuda, tmp_path):
    """the golden fixture (elem 2, lag 3, fold 1) and a model container, read by plans whose own setting says something else"""
    g = open(GOLD, "rb").read()
    x = gold.gold_input()
    assert np.array_equal(G.read(g), x)
    y = LI.lag_bytes("adc16x8", LENGTH)
    c = G.write(y, N, ROWS, 2, 8, 1)
    for elem, lag, fold, n, rows in ((2, 3, 1, N, ROWS), (8, 16, 0, N, 1), (4, 1, 1, 70000, 2)):
        with _plan(glc, ctx, elem, lag, fold, n=n, rows=rows) as plan:
            _decodes_everywhere(glc, plan, g, x, tmp_path)
            _decodes_everywhere(glc, plan, c, y, tmp_path)


# --- 2. refusals -----------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_refusals_of_version_11(glc, ctx, cuda, tmp_path):
    import torch
    c11 = open(GOLD, "rb").read()
    x = gold.gold_input()
    cases, _ = G.refusal_cases(c11)
    assert len(cases) >= 20
    guard = 64
    path = tmp_path / "bad.glcb"

    def filter_auto_plan():
        plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS)
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        return plan

    with _plan(glc, ctx, 2, 3, 1) as on_plan, _plan(glc, ctx, 2, 1, 0) as auto_plan, filter_auto_plan() as fa_plan, \
            glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plain_plan:
        assert glc.container_get_delta_lag(auto_plan) == (1, 0) and glc.container_get_filter_auto(fa_plan) == 1
        for name, cont, want, reads in cases:
            plan = on_plan if "lag" in reads else fa_plan if "filter" in reads else auto_plan if "auto" in reads else plain_plan
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN, name
            assert glc.container_last_error(plan) == want, name
            assert bool((out[x.size:] == 0xAB).all())
            if want[0] == M.STREAM_HEADER:
                assert bool((out == 0xAB).all()), name
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want, name
            path.write_bytes(cont)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_file(plan, str(path), str(tmp_path / "back.bin"))
            assert glc.container_last_error(plan) == want, name
            if want[0] in (M.STREAM_HEADER, M.TRUNCATED) or (want[0] == M.FRAME_TABLE and want[2] == -1):
                with pytest.raises(glc.CudppError):                # what the headers alone show, the index walks refuse alike
                    glc.container_index(plan, _gpu(np.frombuffer(cont, np.uint8)))
                assert glc.container_last_error(plan) == want, name
                with pytest.raises(glc.CudppError):
                    glc.container_index_host(plan, np.frombuffer(cont, np.uint8))
                assert glc.container_last_error(plan) == want, name
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c11, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


# --- 3. byte-for-byte compatibility ---------------------------------------------------------------------------------------------
def test_one_zero_writes_version_8(glc, ctx, cuda):
    x = LI.lag_bytes("stereo16", LENGTH)
    want8 = U.write(x, N, ROWS, 2, True)
    assert struct.unpack("<HH", want8[4:8]) == (8, 1)
    with _plan(glc, ctx, 2, 2, 1) as plan:
        glc.container_set_delta_lag(plan, 1, 0)                    # on, then off again
        assert glc.container_get_delta_lag(plan) == (1, 0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want8
        with pytest.raises(glc.CudppError):                        # and it no longer speaks version 11
            glc.container_decompress(plan, _gpu(np.frombuffer(G.write(x, N, ROWS, 2, 2, 1), np.uint8)))
        assert glc.container_last_error(plan) == (1, -1, -1)


def test_with_the_setting_never_touched_versions_4_8_and_10_are_the_models(glc, ctx, cuda):
    x = FI.four_frames()
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, FI.N, rows=FI.ROWS) as plan:
        glc.container_set_shuffle(plan, 4)
        glc.container_set_delta(plan, 1)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, FI.N, FI.ROWS, 4, 0, delta=True)      # version 4
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        c8 = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c8 == U.write(x, FI.N, FI.ROWS, 4, True) and struct.unpack("<HH", c8[4:8]) == (8, 1)
        glc.container_set_shuffle(plan, 0)
        glc.container_set_filter_auto(plan, 1)
        c10 = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c10 == F.write(x, FI.N, FI.ROWS) and struct.unpack("<HH", c10[4:8]) == (10, 0)
        assert glc.container_get_delta_lag(plan) == (1, 0)


# --- 4. the setter ---------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        get = lambda: glc.container_get_delta_lag(plan)
        on = lambda: glc.container_set_delta_lag(plan, 3, 1)

        def ready():
            glc.container_set_codec(plan, 1)
            glc.container_set_auto(plan, 1)
            glc.container_set_shuffle(plan, 4)
            glc.container_set_delta(plan, 1)

        assert get() == (1, 0)
        glc.container_set_delta_lag(plan, 1, 0)                                     # off is always legal
        # each prerequisite missing in turn: refused and unchanged
        glc.container_set_shuffle(plan, 4)
        glc.container_set_delta(plan, 1)
        assert refused(glc.container_set_delta_lag, 3, 1) and get() == (1, 0)      # the BWT codec
        glc.container_set_codec(plan, 1)
        assert refused(glc.container_set_delta_lag, 3, 1) and get() == (1, 0)      # the auto mode is off
        for mode in (glc.container_set_sparse, glc.container_set_ans, glc.container_set_dedup):
            mode(plan, 1)
            assert refused(glc.container_set_delta_lag, 2, 0) and get() == (1, 0)  # another mode is no substitute
            mode(plan, 0)
        glc.container_set_auto(plan, 1)
        glc.container_set_delta(plan, 0)
        assert refused(glc.container_set_delta_lag, 3, 1) and get() == (1, 0)      # the delta is off
        glc.container_set_shuffle(plan, 0)
        assert refused(glc.container_set_delta_lag, 3, 1) and get() == (1, 0)      # the shuffle is off
        glc.container_set_filter_auto(plan, 1)
        assert refused(glc.container_set_delta_lag, 1, 1) and get() == (1, 0)      # filter-auto is on
        glc.container_set_filter_auto(plan, 0)
        ready()
        for lag, fold in ((0, 0), (17, 0), (3, 2), (1 << 31, 1), (0, 1)):
            assert refused(glc.container_set_delta_lag, lag, fold) and get() == (1, 0)
        on()
        assert get() == (3, 1)
        for lag, fold in ((0, 0), (17, 1), (3, 2)):
            assert refused(glc.container_set_delta_lag, lag, fold) and get() == (3, 1)   # unchanged
        assert refused(glc.container_set_filter_auto, 1) and get() == (3, 1)       # (it wants the shuffle off)
        assert refused(glc.container_set_sparse, 1) and refused(glc.container_set_shuffle, 3) and get() == (3, 1)
        for elem in (2, 8, 4):
            glc.container_set_shuffle(plan, elem)                                  # a change among 2, 4 and 8 keeps it
            assert get() == (3, 1) and glc.container_get_delta(plan) == 1
        glc.container_set_delta_lag(plan, 16, 0)
        assert get() == (16, 0)
        # each way of ending a prerequisite puts it back to (1, 0), and it stays there
        on(); glc.container_set_delta(plan, 0)
        assert get() == (1, 0)
        glc.container_set_delta(plan, 1)
        assert get() == (1, 0)
        on(); glc.container_set_shuffle(plan, 0)
        assert get() == (1, 0)
        ready(); on(); glc.container_set_shuffle(plan, 1)
        assert get() == (1, 0)
        ready(); on(); glc.container_set_auto(plan, 0)
        assert get() == (1, 0)
        ready(); on(); glc.container_set_codec(plan, 0)
        assert get() == (1, 0) and glc.container_get_auto(plan) == 0
        ready(); on(); glc.container_set_codec(plan, 1)                            # the same codec again: no change
        assert get() == (3, 1)
        glc.container_set_delta_lag(plan, 1, 0)
        assert get() == (1, 0) and glc.container_get_delta(plan) == 1 and glc.container_get_auto(plan) == 1


# --- 5. index and range ----------------------------------------------------------------------------------------------------------
def test_index_and_range_reads(glc, ctx, cuda, tmp_path):
    elem, lag, fold = 2, 8, 1
    x = LI.lag_bytes("adc16x8", LENGTH)
    want = G.write(x, N, ROWS, elem, lag, fold)
    Fr = N * ROWS
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(5000, 100), (2048 * 2 * 3 - 3, 9), (N - 5, 10), (N - 1, 2), (Fr + 3 * N - 7, 30),       # inside a block, across block edges
              (Fr - 10, 20), (Fr - 5000, 10000), (2 * Fr - 1, N),                                   # across frame edges
              (2 * Fr + 2 * N - 9, 9), (0, x.size), (x.size, 0), (1, 1)]
    with _plan(glc, ctx, 4, 2, 0) as plan:                          # (the plan's own lag and fold are not the stream's)
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, N, 3, 11, G.flags_of(lag, fold), elem)
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            assert ix.info()[3:] == (11, G.flags_of(lag, fold), elem)
            for off, cnt in ranges[:8]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[1], ranges[5], ranges[7]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_delta_lag(plan, 1, 0)                # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)
    g = open(GOLD, "rb").read()                                     # lag 3: RUN % lag != 0, and a ragged tail frame
    y = gold.gold_input()
    with _plan(glc, ctx, 2, 3, 1, n=gold.BLOCK, rows=gold.ROWS) as plan:
        dg = _gpu(np.frombuffer(g, np.uint8))
        with glc.container_index(plan, dg) as ix:
            assert ix.info() == (y.size, gold.BLOCK, 3, 11, G.flags_of(3, 1), 2)
            for off, cnt in ((4090, 20), (3 * gold.BLOCK - 3, 7), (6 * gold.BLOCK - 100, 1335), (6 * gold.BLOCK + 1230, 5), (0, y.size)):
                assert np.array_equal(_host(glc.container_read_range(plan, ix, dg, off, cnt)), y[off:off + cnt]), (off, cnt)


# --- 6. the ratio conditions -----------------------------------------------------------------------------------------------------
def _size(glc, plan, x):
    return glc.container_compress(plan, _gpu(x)).numel()


@pytest.mark.parametrize("kind", sorted(LI.KINDS))
def test_lag_equal_to_the_channels_beats_both_version_8_filters(glc, ctx, cuda, kind):
    elem, ch = LI.KINDS[kind]
    x = LI.lag_bytes(kind, LENGTH)
    with _plan(glc, ctx, elem, ch, 1) as plan:
        v11 = _size(glc, plan, x)
        assert v11 == len(G.write(x, N, ROWS, elem, ch, 1))
        glc.container_set_delta_lag(plan, 1, 0)
        delta = _size(glc, plan, x)
        glc.container_set_delta(plan, 0)
        shuffle_only = _size(glc, plan, x)
    assert v11 < min(delta, shuffle_only), (v11, delta, shuffle_only)


@pytest.mark.parametrize("kind", sorted(LI.FOLD_ONLY))
def test_the_fold_alone_beats_the_plain_delta(glc, ctx, cuda, kind):
    elem = LI.FOLD_ONLY[kind]
    x = LI.fold_bytes(kind, LENGTH)
    with _plan(glc, ctx, elem, 1, 1) as plan:
        folded = _size(glc, plan, x)
        glc.container_set_delta_lag(plan, 1, 0)
        delta = _size(glc, plan, x)
    assert folded < delta, (folded, delta)
