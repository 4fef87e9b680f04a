"""The byte-delta setting of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points write
the bytes of the Python model of format version 15 (tests/byte_delta_model.py), pipelined or not, and read them back; every refusal
case comes back with the model's class, frame and block; a plan without the setting refuses version 15; with the setting off the
bytes are the auto mode's; the setter's prerequisites and exclusions; the index reports the header's words, range reads give the
input's slices and decode the blocks the rounding rule says."""
import struct

import numpy as np
import pytest

import auto_model as U
import byte_delta_inputs as BI
import byte_delta_model as B
import container_model as M

pytestmark = pytest.mark.gpu

ILLEGAL, UNKNOWN = 2, 9999
N, ROWS = 16384, 4
LENGTH = 5 * N * ROWS // 2                                        # 2.5 frames
PAIRS = ((1, 0), (3, 0), (1, 600), (3, 1281), (16, 65536))        # (lag, stride)


def _input(lag, stride, n=LENGTH):
    if lag == 3:
        return BI.rgb8(n, 427)
    return BI.grey8(n, stride if 2 <= stride <= 4096 else 721)


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


def _auto_plan(glc, ctx, n=N, rows=ROWS, pipelined=False):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    return plan


def _plan(glc, ctx, lag, stride, n=N, rows=ROWS, pipelined=False):
    plan = _auto_plan(glc, ctx, n, rows, pipelined)
    glc.container_set_byte_delta(plan, lag, stride)
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


# --- 1. the model's bytes, and read back ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag,stride", PAIRS)
def test_gpu_container_equals_the_models(glc, ctx, cuda, tmp_path, lag, stride):
    x = _input(lag, stride)
    want = B.write(x, N, ROWS, lag, stride)
    assert struct.unpack("<HHII", want[4:16]) == (15, 1 | (4 if stride else 0) | (lag - 1) << 8, N, 1 | stride << 8)
    assert [(f["nb"], f["blk_len"]) for f in M.layout(want)["frames"]] == [(ROWS, N)] * 2 + [(2, N)]
    for pipelined in (False, True):
        with _plan(glc, ctx, lag, stride, pipelined=pipelined) as plan:
            assert glc.container_get_byte_delta(plan) == (lag, stride)
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want
            assert glc.container_compress_host(plan, x).tobytes() == want
            src, dst = tmp_path / "in.bin", tmp_path / "out.glcb"
            x.tofile(src)
            glc.container_compress_file(plan, str(src), str(dst))
            assert dst.read_bytes() == want
            _decodes_everywhere(glc, plan, want, x, tmp_path)
            for L in (0, 1, lag, N + 9, N * ROWS + 2049):         # (the last: a full frame and a ragged one)
                y = x[:L]
                c = glc.container_compress(plan, _gpu(y))
                assert _host(c).tobytes() == B.write(y, N, ROWS, lag, stride)
                assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


def test_lag_and_stride_come_from_the_stream_header_not_the_plan(glc, ctx, cuda, tmp_path):
    x = BI.rgb8(LENGTH, 427)
    c = B.write(x, N, ROWS, 3, 1281)
    for lag, stride, n, rows in ((1, 0, N, ROWS), (16, 2, N, 1), (3, 1281, 70000, 2)):
        with _plan(glc, ctx, lag, stride, n=n, rows=rows) as plan:
            _decodes_everywhere(glc, plan, c, x, tmp_path)


def test_a_byte_delta_plan_reads_the_older_versions(glc, ctx, cuda, tmp_path):
    x = BI.stereo8(2 * N + 5)
    older = [M.write(x, N, 2), M.write(x, N, 2, 4), M.write(x, N, 2, 4, 1), U.write(x, N, 2, 4, True), U.write(x, N, 2)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 8, 8]
    with _plan(glc, ctx, 2, 0, rows=2) as plan:
        for c in older:
            _decodes_everywhere(glc, plan, c, x, tmp_path)


# --- 2. refusals -----------------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_refusals_of_version_15(glc, ctx, cuda, tmp_path):
    import torch
    x = BI.rgb8(LENGTH, 427)
    c15 = B.write(x, N, ROWS, 3, 1281)
    cases, _ = B.refusal_cases(c15)
    assert len(cases) >= 25
    guard = 64
    path = tmp_path / "bad.glcb"

    def other_plan(kind):
        plan = _auto_plan(glc, ctx)
        if kind == "filter":
            glc.container_set_filter_auto(plan, 1)
        else:
            glc.container_set_shuffle(plan, 2)
            glc.container_set_delta(plan, 1)
            if kind == "lag":
                glc.container_set_delta_lag(plan, 3, 1)
            else:
                glc.container_set_delta_grid(plan, 100, 1)
        return plan

    with _plan(glc, ctx, 3, 1281) as on_plan, _auto_plan(glc, ctx) as auto_plan, other_plan("filter") as fa_plan, other_plan("lag") as lag_plan, \
            other_plan("grid") as grid_plan, glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plain_plan:
        for name, cont, want, reads in cases:
            plan = (on_plan if "byte" in reads else fa_plan if "filter" in reads else lag_plan if "lag" in reads else grid_plan if "grid" in reads
                    else auto_plan if "auto" in reads else plain_plan)
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
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c15, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


def test_a_plan_without_the_setting_refuses_version_15(glc, ctx, cuda):
    x = BI.grey8(N + 9, 721)
    for lag, stride in ((1, 0), (3, 1281)):
        c = _gpu(np.frombuffer(B.write(x, N, ROWS, lag, stride), np.uint8))
        with _plan(glc, ctx, 2, 64) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            glc.container_set_byte_delta(plan, 0, 0)               # on, then off again: it no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_decompress(plan, c)
            assert glc.container_last_error(plan) == (1, -1, -1)
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plan:
            with pytest.raises(glc.CudppError):
                glc.container_decompress(plan, c)
            assert glc.container_last_error(plan) == (1, -1, -1)


# --- 3. byte-for-byte compatibility ---------------------------------------------------------------------------------------------
def test_with_the_setting_off_the_bytes_are_the_auto_modes(glc, ctx, cuda):
    x = BI.rgb8(LENGTH, 427)
    want8 = U.write(x, N, ROWS)
    assert struct.unpack("<HHII", want8[4:16]) == (8, 0, N, 0) and want8 == B.write(x, N, ROWS, 0, 0)
    with _auto_plan(glc, ctx) as plan:                              # never touched
        assert glc.container_get_byte_delta(plan) == (0, 0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want8
    for pipelined in (False, True):
        with _plan(glc, ctx, 3, 1281, pipelined=pipelined) as plan:  # on, then off again
            assert len(_host(glc.container_compress(plan, _gpu(x))).tobytes()) < len(want8) // 2
            glc.container_set_byte_delta(plan, 0, 0)
            assert glc.container_get_byte_delta(plan) == (0, 0)
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want8


# --- 4. the setter -----------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        get = lambda: glc.container_get_byte_delta(plan)
        on = lambda: glc.container_set_byte_delta(plan, 3, 1281)

        def ready():
            glc.container_set_shuffle(plan, 0)
            glc.container_set_codec(plan, 1)
            glc.container_set_auto(plan, 1)

        assert get() == (0, 0)
        glc.container_set_byte_delta(plan, 0, 0)                                   # off is always legal
        # each prerequisite missing in turn: refused and unchanged
        assert refused(glc.container_set_byte_delta, 3, 1281) and get() == (0, 0)  # the BWT codec
        glc.container_set_codec(plan, 1)
        assert refused(glc.container_set_byte_delta, 3, 1281) and get() == (0, 0)  # the auto mode is off
        for mode in (glc.container_set_sparse, glc.container_set_ans, glc.container_set_dedup):
            mode(plan, 1)
            assert refused(glc.container_set_byte_delta, 2, 0) and get() == (0, 0)  # another mode is no substitute
            mode(plan, 0)
        glc.container_set_auto(plan, 1)
        for elem in (2, 4, 8):
            glc.container_set_shuffle(plan, elem)
            assert refused(glc.container_set_byte_delta, 1, 0) and get() == (0, 0)  # the shuffle is on
            glc.container_set_delta(plan, 1)
            assert refused(glc.container_set_byte_delta, 1, 0) and get() == (0, 0)  # and the delta
        glc.container_set_shuffle(plan, 0)
        glc.container_set_filter_auto(plan, 1)
        assert refused(glc.container_set_byte_delta, 1, 0) and get() == (0, 0)     # filter-auto is on
        glc.container_set_filter_auto(plan, 0)
        glc.container_set_codec(plan, 4)
        assert refused(glc.container_set_byte_delta, 1, 0) and get() == (0, 0)     # the CHOOSE codec
        ready()
        for lag, stride in ((17, 0), (1, 1), (3, 65537), (1 << 31, 0), (3, 1 << 31)):
            assert refused(glc.container_set_byte_delta, lag, stride) and get() == (0, 0)
        on()
        assert get() == (3, 1281)
        for lag, stride in ((17, 0), (3, 1), (3, 65537)):
            assert refused(glc.container_set_byte_delta, lag, stride) and get() == (3, 1281)    # unchanged
        # while it is on: the shuffle at 2, 4 or 8 and filter-auto are refused, and with the shuffle what needs it
        for elem in (2, 4, 8, 3):
            assert refused(glc.container_set_shuffle, elem) and get() == (3, 1281)
        assert refused(glc.container_set_filter_auto, 1) and get() == (3, 1281)
        assert refused(glc.container_set_delta, 1) and refused(glc.container_set_delta_lag, 3, 1) and refused(glc.container_set_delta_grid, 100, 1)
        assert refused(glc.container_set_sparse, 1) and get() == (3, 1281)         # (another mode while the auto mode is on)
        glc.container_set_shuffle(plan, 0)                                         # "off" in both spellings keeps it
        glc.container_set_shuffle(plan, 1)
        glc.container_set_filter_auto(plan, 0)
        assert get() == (3, 1281) and glc.container_get_shuffle(plan) == 0
        glc.container_set_byte_delta(plan, 16, 0)
        assert get() == (16, 0)
        glc.container_set_byte_delta(plan, 1, 65536)
        assert get() == (1, 65536)
        # each way of ending a prerequisite switches it off, and it stays off
        on(); glc.container_set_auto(plan, 0)
        assert get() == (0, 0)
        glc.container_set_auto(plan, 1)
        assert get() == (0, 0)
        on(); glc.container_set_codec(plan, 0)
        assert get() == (0, 0) and glc.container_get_auto(plan) == 0
        ready(); on(); glc.container_set_codec(plan, 4)
        assert get() == (0, 0)
        ready(); on(); glc.container_set_codec(plan, 1)                            # the same codec again: no change
        assert get() == (3, 1281)
        glc.container_set_byte_delta(plan, 0, 77)                                  # off, whatever the stride says
        assert get() == (0, 0) and glc.container_get_auto(plan) == 1
        glc.container_set_shuffle(plan, 4)                                         # and the shuffle is free again


# --- 5. index and range ----------------------------------------------------------------------------------------------------------
def _blocks_of(off, cnt, total, stride):
    """the blocks a range read of bytes [off, off + cnt) decodes, by the rounding rule, frame by frame"""
    Fr, blocks = N * ROWS, 0
    for pos in range(0, total, Fr):
        nb = -(-min(Fr, total - pos) // N)
        a, b = max(off, pos) - pos, min(off + cnt, pos + nb * N, total) - pos
        if a < b:
            blocks += len(B.range_blocks(a, b, stride, nb, N))
    return blocks


@pytest.mark.parametrize("lag,stride", [(3, 1281), (3, 0)])
def test_index_and_range_reads(glc, ctx, cuda, tmp_path, lag, stride):
    x = BI.rgb8(LENGTH, 427)
    want = B.write(x, N, ROWS, lag, stride)
    Fr, step = N * ROWS, B.step(stride)
    assert step == (43008 if stride else 2048) and 2 * N < 43008 < 3 * N       # the first band edge lies in block 2
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(5000, 100), (2048 * 3 + 5, 9),                                   # inside a run
              (3 * N + 100, 50), (43008 - 4, 8), (Fr + 43008 + 7000, 30),       # behind a band edge that lies in another block; across it
              (N - 5, 10), (Fr - 10, 20), (Fr - 5000, 10000), (2 * Fr - 1, N),  # across block and frame edges
              (2 * Fr + 2 * N - 9, 9), (0, x.size), (x.size, 0), (1, 1)]
    with _plan(glc, ctx, 1, 64) as plan:                            # (the plan's own lag and stride are not the stream's)
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, N, 3, 15, B.flags_of(lag, stride), B.word3_of(stride))
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                if cnt:
                    assert glc.container_last_range_stats(plan)[1] == _blocks_of(off, cnt, x.size, stride), (off, cnt)
            if stride:                                              # the rule, spelt out once: bytes of block 3 need block 2, where their band starts
                glc.container_read_range(plan, ix, d, 3 * N + 100, 50)
                assert glc.container_last_range_stats(plan)[:2] == (1, 2)
                glc.container_read_range(plan, ix, d, 43008 - 4, 8)
                assert glc.container_last_range_stats(plan)[:2] == (1, 3)
            else:
                glc.container_read_range(plan, ix, d, 3 * N + 100, 50)
                assert glc.container_last_range_stats(plan)[:2] == (1, 1)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            assert ix.info()[3:] == (15, B.flags_of(lag, stride), B.word3_of(stride))
            for off, cnt in ranges[:9]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[2], ranges[3], ranges[7]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_byte_delta(plan, 0, 0)                # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)
