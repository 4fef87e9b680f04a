"""The grid setting of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points, pipelined
and not, write the bytes of the Python model of format version 12 (tests/grid_model.py) and read them back; the golden fixture
decodes; width and fold come from the stream header; every refusal case comes back with the model's class and frame; with the
setting off the bytes are those of a plan that never touched it; the setter's prerequisite and reset rules; the index reports word 3
as it stands and range reads around a band edge give the input's slices."""
import os
import struct
import sys

import numpy as np
import pytest

import auto_model as U
import container_model as M
import grid_inputs as GI
import grid_model as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "grid_v12_container.bin")
ILLEGAL, UNKNOWN = 2, 9999
N, ROWS = 4096, 4
LENGTH = 3 * N * ROWS + N + 777                                   # 54025 bytes: three frames and a ragged fourth of two blocks
CASES = (("img16", 2, 100, 1), ("field32", 4, 64, 0), ("walk32", 4, 65, 1))      # (input, elem, width, fold): two bands, two, one a frame

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_grid_v12_gold as gold  # noqa: E402
import make_lag_v11_gold as gold11  # noqa: E402


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


def _plan(glc, ctx, elem=2, width=0, fold=0, n=N, rows=ROWS, pipelined=False, lag=(1, 0)):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_delta(plan, 1)
    glc.container_set_delta_lag(plan, *lag)
    glc.container_set_delta_grid(plan, width, fold)
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


# --- 1. small frames: the model's bytes from all six entry points, and read back -------------------------------------------------
@pytest.mark.parametrize("kind,elem,width,fold", CASES)
def test_gpu_container_equals_the_models(glc, ctx, cuda, tmp_path, kind, elem, width, fold):
    x = GI.grid_bytes(kind, LENGTH, width)
    want = G.write(x, N, ROWS, elem, width, fold)
    assert struct.unpack("<HHII", want[4:16]) == (12, 5 | fold << 1, N, elem | width << 8)
    assert [(f["nb"], f["blk_len"]) for f in M.layout(want)["frames"]] == [(ROWS, N)] * 3 + [(1, N), (1, 777)]
    for pipelined in (False, True):
        with _plan(glc, ctx, elem, width, fold, pipelined=pipelined) as plan:
            assert glc.container_get_delta_grid(plan) == (width, fold)
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want
            assert glc.container_compress_host(plan, x).tobytes() == want
            src, dst = tmp_path / "in.bin", tmp_path / "out.glcb"
            x.tofile(src)
            glc.container_compress_file(plan, str(src), str(dst))
            assert dst.read_bytes() == want
            _decodes_everywhere(glc, plan, want, x, tmp_path)
            for n in (0, 1, elem * width - 1, N + 9):
                y = x[:n]
                c = glc.container_compress(plan, _gpu(y))
                assert _host(c).tobytes() == G.write(y, N, ROWS, elem, width, fold)
                assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


def test_width_and_fold_come_from_the_stream_header_not_the_plan(glc, ctx, cuda, tmp_path):
    """the golden fixture (elem 2, width 100, fold 1) and a model container, read by plans whose own setting says something else"""
    g = open(GOLD, "rb").read()
    x = gold.gold_input()
    assert np.array_equal(G.read(g), x)
    y = GI.grid_bytes("field32", LENGTH, 1000)
    c = G.write(y, N, ROWS, 4, 1000, 1)
    for elem, width, fold, n, rows in ((2, 100, 1, gold.BLOCK, gold.ROWS), (8, 65536, 0, gold.BLOCK, 1), (4, 7, 1, 70000, 2)):
        with _plan(glc, ctx, elem, width, fold, n=n, rows=rows) as plan:
            _decodes_everywhere(glc, plan, g, x, tmp_path)
            _decodes_everywhere(glc, plan, c, y, tmp_path)


# --- 2. refusals -----------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_refusals_of_version_12(glc, ctx, cuda, tmp_path):
    import torch
    c12 = open(GOLD, "rb").read()
    x = gold.gold_input()
    cases, _ = G.refusal_cases(c12, gold11.make())
    assert len(cases) >= 20
    guard = 64
    path = tmp_path / "bad.glcb"

    def filter_auto_plan():
        plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, gold.BLOCK, rows=gold.ROWS)
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        return plan

    kw = dict(n=gold.BLOCK, rows=gold.ROWS)
    with _plan(glc, ctx, 2, 100, 1, **kw) as on_plan, _plan(glc, ctx, 2, lag=(3, 1), **kw) as lag_plan, _plan(glc, ctx, 2, **kw) as auto_plan, \
            filter_auto_plan() as fa_plan, glc.Plan(ctx, glc.CUDPP_COMPRESS, gold.BLOCK, rows=gold.ROWS) as plain_plan:
        assert glc.container_get_delta_grid(lag_plan) == (0, 0) and glc.container_get_delta_lag(lag_plan) == (3, 1)
        assert glc.container_get_delta_grid(auto_plan) == (0, 0) and glc.container_get_filter_auto(fa_plan) == 1
        for name, cont, want, reads in cases:
            plan = on_plan if "grid" in reads else lag_plan if "lag" in reads else fa_plan if "filter" in reads else \
                auto_plan if "auto" in reads else plain_plan
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
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c12, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


# --- 3. byte-for-byte compatibility ---------------------------------------------------------------------------------------------
def test_with_the_setting_off_the_bytes_are_those_of_a_plan_that_never_touched_it(glc, ctx, cuda):
    x = GI.grid_bytes("img16", LENGTH, 100)
    want8 = U.write(x, N, ROWS, 2, True)
    assert struct.unpack("<HH", want8[4:8]) == (8, 1)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as never:
        glc.container_set_codec(never, 1)
        glc.container_set_auto(never, 1)
        glc.container_set_shuffle(never, 2)
        glc.container_set_delta(never, 1)
        c_never = _host(glc.container_compress(never, _gpu(x))).tobytes()
    with _plan(glc, ctx, 2, 100, 1) as plan:
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == G.write(x, N, ROWS, 2, 100, 1)
        glc.container_set_delta_grid(plan, 0, 0)                   # on, then off again
        assert glc.container_get_delta_grid(plan) == (0, 0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == c_never == want8
        with pytest.raises(glc.CudppError):                        # and it no longer speaks version 12
            glc.container_decompress(plan, _gpu(np.frombuffer(G.write(x, N, ROWS, 2, 100, 1), np.uint8)))
        assert glc.container_last_error(plan) == (1, -1, -1)


# --- 4. the setter ---------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        get = lambda: glc.container_get_delta_grid(plan)
        on = lambda: glc.container_set_delta_grid(plan, 1024, 1)

        def ready():
            glc.container_set_codec(plan, 1)
            glc.container_set_auto(plan, 1)
            glc.container_set_shuffle(plan, 4)
            glc.container_set_delta(plan, 1)

        assert get() == (0, 0)
        glc.container_set_delta_grid(plan, 0, 0)                                    # off is always legal
        # each prerequisite missing in turn: refused and unchanged
        glc.container_set_shuffle(plan, 4)
        glc.container_set_delta(plan, 1)
        assert refused(glc.container_set_delta_grid, 1024, 1) and get() == (0, 0)   # the BWT codec
        glc.container_set_codec(plan, 1)
        assert refused(glc.container_set_delta_grid, 1024, 1) and get() == (0, 0)   # the auto mode is off
        for mode in (glc.container_set_sparse, glc.container_set_ans, glc.container_set_dedup):
            mode(plan, 1)
            assert refused(glc.container_set_delta_grid, 64, 0) and get() == (0, 0)  # another mode is no substitute
            mode(plan, 0)
        glc.container_set_auto(plan, 1)
        glc.container_set_delta(plan, 0)
        assert refused(glc.container_set_delta_grid, 1024, 1) and get() == (0, 0)   # the delta is off
        glc.container_set_shuffle(plan, 0)
        assert refused(glc.container_set_delta_grid, 1024, 1) and get() == (0, 0)   # the shuffle is off
        glc.container_set_filter_auto(plan, 1)
        assert refused(glc.container_set_delta_grid, 1024, 0) and get() == (0, 0)   # filter-auto is on
        glc.container_set_filter_auto(plan, 0)
        ready()
        glc.container_set_delta_lag(plan, 3, 1)
        assert refused(glc.container_set_delta_grid, 1024, 1) and get() == (0, 0)   # the lag is not (1, 0)
        glc.container_set_delta_lag(plan, 1, 0)
        for width, fold in ((1, 0), (65537, 0), (1024, 2), (1 << 31, 1), (0, 2)):
            assert refused(glc.container_set_delta_grid, width, fold) and get() == (0, 0)
        for width in (2, 65536):
            glc.container_set_delta_grid(plan, width, 0)
            assert get() == (width, 0)
        on()
        assert get() == (1024, 1)
        for width, fold in ((1, 0), (65537, 1), (1024, 2)):
            assert refused(glc.container_set_delta_grid, width, fold) and get() == (1024, 1)   # unchanged
        for lag, fold in ((3, 1), (1, 1), (2, 0)):                                  # while the grid is on the lag stays (1, 0)
            assert refused(glc.container_set_delta_lag, lag, fold) and get() == (1024, 1) and glc.container_get_delta_lag(plan) == (1, 0)
        glc.container_set_delta_lag(plan, 1, 0)
        assert get() == (1024, 1)
        assert refused(glc.container_set_filter_auto, 1) and get() == (1024, 1)     # (it wants the shuffle off)
        assert refused(glc.container_set_sparse, 1) and refused(glc.container_set_shuffle, 3) and get() == (1024, 1)
        for elem in (2, 8, 4):
            glc.container_set_shuffle(plan, elem)                                   # a change among 2, 4 and 8 keeps it
            assert get() == (1024, 1) and glc.container_get_delta(plan) == 1
        # each way of ending a prerequisite puts it back to off, and it stays there
        on(); glc.container_set_delta(plan, 0)
        assert get() == (0, 0)
        glc.container_set_delta(plan, 1)
        assert get() == (0, 0)
        on(); glc.container_set_shuffle(plan, 0)
        assert get() == (0, 0)
        ready(); on(); glc.container_set_shuffle(plan, 1)
        assert get() == (0, 0)
        ready(); on(); glc.container_set_auto(plan, 0)
        assert get() == (0, 0)
        ready(); on(); glc.container_set_codec(plan, 0)
        assert get() == (0, 0) and glc.container_get_auto(plan) == 0
        ready(); on(); glc.container_set_codec(plan, 1)                             # the same codec again: no change
        assert get() == (1024, 1)
        glc.container_set_delta_grid(plan, 0, 1)                                    # off takes its fold along
        assert get() == (0, 0) and glc.container_get_delta(plan) == 1 and glc.container_get_auto(plan) == 1
        glc.container_set_delta_lag(plan, 3, 1)                                     # and the lag is free again
        assert glc.container_get_delta_lag(plan) == (3, 1)


# --- 5. index and range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,elem,width,fold", CASES)
def test_index_and_range_reads(glc, ctx, cuda, tmp_path, kind, elem, width, fold):
    x = GI.grid_bytes(kind, LENGTH, width)
    want = G.write(x, N, ROWS, elem, width, fold)
    Fr, B = N * ROWS, G.period(width) * elem                       # a frame's bytes, a band's (8192, 8192 or 16384: the frame)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(B - 1, 2), (B, 1), (B + width * elem - 3, 7), (B - 5, 10), (Fr + B - 1, 1), (Fr + B, elem), (B + width * elem, 5),   # a band edge
              (5000, 100), (N - 5, 10), (Fr + 3 * N - 7, 30), (Fr - 10, 20), (Fr - 3000, 6000), (2 * Fr - 1, N),     # block and frame edges
              (3 * Fr + N - 9, 9), (3 * Fr + N - 1, 778), (x.size - 3, 3), (0, x.size), (x.size, 0), (1, 1)]
    with _plan(glc, ctx, 8, 7, fold ^ 1) as plan:                  # (the plan's own width and fold are not the stream's)
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, N, 5, 12, 5 | fold << 1, elem | width << 8)
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            assert ix.info()[3:] == (12, 5 | fold << 1, elem | width << 8)
            for off, cnt in ranges[:10]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[0], ranges[3], ranges[11]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_delta_grid(plan, 0, 0)               # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)


def test_range_reads_of_the_golden(glc, ctx, cuda):
    g = open(GOLD, "rb").read()                                     # three bands a frame, and a ragged tail frame
    y = gold.gold_input()
    with _plan(glc, ctx, 2, 100, 1, n=gold.BLOCK, rows=gold.ROWS) as plan:
        dg = _gpu(np.frombuffer(g, np.uint8))
        with glc.container_index(plan, dg) as ix:
            assert ix.info() == (y.size, gold.BLOCK, 3, 12, 7, 2 | 100 << 8)
            for off, cnt in ((8190, 20), (16384 + 199, 3), (3 * gold.BLOCK - 3, 7), (6 * gold.BLOCK - 100, 1335), (6 * gold.BLOCK + 1230, 5), (0, y.size)):
                assert np.array_equal(_host(glc.container_read_range(plan, ix, dg, off, cnt)), y[off:off + cnt]), (off, cnt)
