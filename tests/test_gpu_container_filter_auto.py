"""Filter-auto of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points write the bytes
of the Python model of format version 10 (tests/filter_auto_model.py), pipelining off and on, for the four-frame input (int64
timestamps, text, float32, a ragged tail) and for one 3-block input per candidate filter, and read them back;
glcContainerLastFilters agrees with the model; the golden fixture decodes; with the setting off a plan writes version 8 as ever and
refuses version 10; the setter's rules; refusals with their glcContainerLastError triples, equal on the device, host and file forms;
capacity; range reads give the input's slices and decode only the blocks the model says."""
import os
import struct

import numpy as np
import pytest

import auto_model as U
import container_model as M
import filter_auto_inputs as FI
import filter_auto_model as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "filter_auto_v10_container.bin")
ILLEGAL, UNKNOWN = 2, 9999


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


@pytest.fixture(scope="module")
def four():
    x = FI.four_frames()
    return x, F.write(x, FI.N, FI.ROWS)


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
    if on:
        glc.container_set_filter_auto(plan, 1)
    return plan


def _all_entry_points(glc, plan, x, want, tmp_path):
    c = glc.container_compress(plan, _gpu(x))
    assert _host(c).tobytes() == want
    assert c.numel() <= glc.container_bound(x.size, FI.N)
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


# --- 1. the setting on: byte-identical to the model, and read back ------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_four_frames_on_all_entry_points(glc, ctx, cuda, tmp_path, four, pipelined):
    x, want = four
    picks = F.picks_of(x, FI.N, FI.ROWS)
    assert len(set(picks)) >= 3 and struct.unpack("<HHII", want[4:16]) == (10, 0, FI.N, 0)
    with _plan(glc, ctx, pipelined) as plan:
        assert glc.container_get_filter_auto(plan) == 1 and glc.container_last_filters(plan) == (0,) * 8
        _all_entry_points(glc, plan, x, want, tmp_path)
        assert glc.container_last_filters(plan) == F.last_filters(picks)
        for L in (0, 1, 8, FI.N + 9):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == F.write(y, FI.N, FI.ROWS)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
            assert glc.container_last_filters(plan) == F.last_filters(F.picks_of(y, FI.N, FI.ROWS))
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused
    assert np.array_equal(F.read(want), x)


@pytest.mark.parametrize("cand", range(7))
def test_one_input_per_candidate(glc, ctx, cuda, tmp_path, cand):
    x = FI.for_candidate(cand)
    want = F.write(x, FI.N, 3)
    assert F.picks_of(x, FI.N, 3) == [cand] and F.frame_words(want) == [F.frame_word(cand)]
    for pipelined in (False, True):
        with _plan(glc, ctx, pipelined, rows=3) as plan:
            _all_entry_points(glc, plan, x, want, tmp_path)
            assert glc.container_last_filters(plan) == F.last_filters([cand])


def test_misaligned_input(glc, ctx, cuda):
    """the frame is probed where it lies: an input 3 bytes off a 16-byte boundary, and frames of 3 * 4099 bytes behind it"""
    x = FI.four_frames()[:7 * 4099 + 50]
    want = F.write(x, 4099, 3)
    buf = _gpu(np.concatenate([np.zeros(3, np.uint8), x]))
    with _plan(glc, ctx, rows=3, n=4099) as plan:
        c = glc.container_compress(plan, buf[3:])
        assert _host(c).tobytes() == want
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)


# --- 2. decoding, and the other plans ---------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_gpu_reads_the_golden_fixture(glc, ctx, cuda, four):
    gold = open(GOLD, "rb").read()
    x = F.read(gold)
    assert np.array_equal(x, four[0])
    g = np.frombuffer(gold, np.uint8)
    for n, rows, pipelined in ((FI.N, FI.ROWS, False), (FI.N, 1, True), (70000, 2, False)):
        with _plan(glc, ctx, pipelined, rows=rows, n=n) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert np.array_equal(glc.container_decompress_host(plan, g), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


def test_with_the_setting_off_a_plan_writes_version_8_and_refuses_version_10(glc, ctx, cuda, tmp_path, four):
    import torch
    x, c10 = four
    src = tmp_path / "c10.glcb"
    src.write_bytes(c10)
    want8 = U.write(x, FI.N, FI.ROWS)

    def auto(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)

    def default(plan):
        pass

    def sparse(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_sparse(plan, 1)

    def dedup(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_dedup(plan, 1)

    for setup in (auto, default, sparse, dedup):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, FI.N, rows=FI.ROWS) as plan:
            setup(plan)
            assert glc.container_get_filter_auto(plan) == 0
            if setup is auto:
                assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want8
                assert glc.container_last_filters(plan) == (4, 0, 0, 0, 0, 0, 0, 4)
            out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, c10, out, x.size)
            assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
            assert bool((out == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(c10, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_file(plan, str(src), str(tmp_path / "back.bin"))
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_index(plan, _gpu(np.frombuffer(c10, np.uint8)))
            assert glc.container_last_error(plan) == (1, -1, -1)
    with _plan(glc, ctx) as plan:                                  # on: version 10 and everything the auto reader reads
        for c in (c10, want8, M.write(x, FI.N, FI.ROWS, 4, 1, delta=True)):
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
        glc.container_set_filter_auto(plan, 0)                     # off again: version 8 again
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want8
        glc.container_set_shuffle(plan, 8)
        glc.container_set_delta(plan, 1)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == U.write(x, FI.N, FI.ROWS, 8, True)
        assert glc.container_last_filters(plan) == (0, 0, 0, 0, 0, 0, 4, 4)


# --- 3. the setter -------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        get = lambda: glc.container_get_filter_auto(plan)
        assert get() == 0
        assert refused(glc.container_set_filter_auto, 1) and get() == 0            # the BWT codec
        glc.container_set_filter_auto(plan, 0)                                    # off is always legal
        glc.container_set_codec(plan, 1)
        assert refused(glc.container_set_filter_auto, 1) and get() == 0            # the auto mode is off
        for mode in (glc.container_set_sparse, glc.container_set_ans, glc.container_set_dedup):
            mode(plan, 1)
            assert refused(glc.container_set_filter_auto, 1) and get() == 0        # another mode is no substitute
            mode(plan, 0)
        glc.container_set_auto(plan, 1)
        glc.container_set_shuffle(plan, 4)
        assert refused(glc.container_set_filter_auto, 1) and get() == 0            # the plan's shuffle is on
        glc.container_set_shuffle(plan, 0)
        for bad in (2, 3, 255, 1 << 31):
            assert refused(glc.container_set_filter_auto, bad) and get() == 0
        glc.container_set_filter_auto(plan, 1)
        assert get() == 1
        for bad in (2, 1 << 31):
            assert refused(glc.container_set_filter_auto, bad) and get() == 1      # unchanged
        for elem in (2, 4, 8):
            assert refused(glc.container_set_shuffle, elem) and get() == 1 and glc.container_get_shuffle(plan) == 0
        assert refused(glc.container_set_shuffle, 3)
        glc.container_set_shuffle(plan, 0)
        glc.container_set_shuffle(plan, 1)                                        # (off, either way)
        assert refused(glc.container_set_delta, 1) and get() == 1                  # (no delta without the shuffle, as ever)
        assert refused(glc.container_set_sparse, 1) and refused(glc.container_set_codec, 7) and get() == 1
        glc.container_set_codec(plan, 1)                                          # the same codec again: no change
        assert get() == 1 and glc.container_get_auto(plan) == 1
        glc.container_set_auto(plan, 0)                                           # the auto mode off: off with it
        assert get() == 0
        glc.container_set_auto(plan, 1)
        assert get() == 0                                                         # and it stays off
        glc.container_set_filter_auto(plan, 1)
        glc.container_set_codec(plan, 0)                                          # a codec change: off, with the auto mode
        assert get() == 0 and glc.container_get_auto(plan) == 0
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        glc.container_set_codec(plan, glc.CONTAINER_CODEC_CHOOSE)
        assert get() == 0
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        glc.container_set_filter_auto(plan, 0)
        assert get() == 0 and glc.container_get_auto(plan) == 1
        glc.container_set_shuffle(plan, 8)                                        # and the shuffle is free again
        assert glc.container_get_shuffle(plan) == 8


# --- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_of_version_10(glc, ctx, cuda, tmp_path, four):
    import torch
    x, c10 = four
    cases, _ = F.refusal_cases(c10)
    assert len(cases) >= 20
    guard = 64
    path = tmp_path / "bad.glcb"
    with _plan(glc, ctx) as plan, _plan(glc, ctx, on=False) as auto_plan, glc.Plan(ctx, glc.CUDPP_COMPRESS, FI.N, rows=FI.ROWS) as plain_plan:
        on_plan = plan
        for name, cont, want, reads in cases:
            plan = on_plan if "filter" in reads else auto_plan if "auto" in reads else plain_plan
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
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
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c10, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


def test_capacity(glc, ctx, cuda, four):
    import torch
    x, want = four
    need = len(want)
    with _plan(glc, ctx) as plan:
        for cap in (need - 1, need // 2, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need and _host(c).tobytes() == want
        out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
        with pytest.raises(glc.CudppError) as e:
            _decompress_into(glc, plan, want, out, x.size - 1)
        assert e.value.code == ILLEGAL and bool((out == 0xAB).all())


# --- 5. range reads ----------------------------------------------------------------------------------------------------------
def test_range_reads(glc, ctx, cuda, tmp_path, four):
    x, want = four
    Fr = FI.N * FI.ROWS
    frames = [(FI.ROWS, FI.N)] * 3 + [(1, 4999)]
    words = F.frame_words(want)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(40000, 100), (2049 * 8 - 3, 9), (Fr + 20000, 100), (Fr + FI.N - 1, 2), (2 * Fr + 30001, FI.N),      # inside each frame
              (Fr - 10, 20), (Fr - 5000, 10000),                                                                # the delta frame and the unfiltered one
              (2 * Fr - 7, 30), (3 * Fr - 5, 4999), (3 * Fr + 4990, 9), (3 * Fr + 4996, 3),                       # ... into the tail, and its len % 4 bytes
              (0, x.size), (x.size, 0)]
    with _plan(glc, ctx) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, FI.N, 4, 10, 0, 0)        # what the stream header says
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                assert glc.container_last_range_stats(plan)[:2] == F.range_stats(frames, words, off, cnt), (off, cnt)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            for off, cnt in ranges[:9]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
                assert glc.container_last_range_stats(plan)[:2] == F.range_stats(frames, words, off, cnt), (off, cnt)
        with glc.container_index_file(plan, str(path)) as ix:
            for off, cnt in (ranges[5], ranges[8]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            # the frame's word is part of what the index holds: a container whose word changed behind it is refused at that frame
            other = F.with_frame_word(want, 3, 4)
            with pytest.raises(glc.CudppError):
                glc.container_read_range_host(plan, ix, np.frombuffer(other, np.uint8), 3 * Fr + 10, 100)
            assert glc.container_last_error(plan) == (2, 3, -1)
            glc.container_set_filter_auto(plan, 0)                 # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)
