"""The runs mode of the container's BWT codec on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points
write the bytes of the Python model of format version 6 (tests/runs_model.py) and read them back, with pipelining off and on, with
and without the filters; every corrupted container of the CPU test is refused with the same triple; a plan with the mode off
refuses version 6 and writes what a plan that never heard of the mode writes; the setters' rules; the golden fixture; range
reads."""
import os
import struct

import numpy as np
import pytest

import container_model as M
import range_model as RM
import runs_inputs as I
import runs_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v6_runs.bin")
ILLEGAL, UNKNOWN = 2, 9999
ROWS = 4
FILTERS = {"plain": (0, False), "shuffle4": (4, False), "delta8": (8, True)}
NAMES = ("text", "log", "page", "zeros", "tail1", "empty")


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


_INPUTS, _WANT = {}, {}


def _input(block_len, name):
    if block_len not in _INPUTS:
        _INPUTS[block_len] = I.container_inputs(block_len, ROWS)
    return _INPUTS[block_len][name]


def _want(block_len, name, filt):
    key = (block_len, name, filt)
    if key not in _WANT:
        _WANT[key] = R.write(_input(block_len, name), block_len, ROWS, *FILTERS[filt])
    return _WANT[key]


def _plan(glc, ctx, n, filt="plain", pipelined=False, runs=True, rows=ROWS):
    elem, delta = FILTERS[filt]
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    if delta:
        glc.container_set_delta(plan, 1)
    if runs:
        glc.container_set_runs(plan, 1)
    return plan


# --- 1. runs on: byte-identical to the model, and read back -----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("block_len", (1000, 4096, 65536))
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, block_len, filt, name):
    x, want = _input(block_len, name), _want(block_len, name, filt)
    elem, delta = FILTERS[filt]
    assert struct.unpack("<HHII", want[4:16]) == (6, 1 if delta else 0, block_len, elem)
    kinds = {k for f in M.layout(want)["frames"] for _, _, k in f["records"]}
    assert kinds <= {M.RAW, R.RUNS} and (R.RUNS in kinds or name == "empty")
    src, dst, back = tmp_path / "in.bin", tmp_path / "out.glcb", tmp_path / "back.bin"
    x.tofile(src)
    for pipelined in (False, True):
        with _plan(glc, ctx, block_len, filt, pipelined) as plan:
            assert glc.container_get_runs(plan) == 1
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want, pipelined
            assert c.numel() <= glc.container_bound(x.size, block_len)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            assert glc.container_last_error(plan) == (0, -1, -1)
            ch = glc.container_compress_host(plan, x)
            assert ch.tobytes() == want
            assert np.array_equal(glc.container_decompress_host(plan, ch), x)
            glc.container_compress_file(plan, str(src), str(dst))
            assert dst.read_bytes() == want
            glc.container_decompress_file(plan, str(dst), str(back))
            assert back.read_bytes() == x.tobytes()
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused
    if block_len <= 4096:
        assert np.array_equal(R.read(want), x)                 # (equal bytes: the model reads the GPU's)


def test_mixed_kinds_and_a_reader_of_another_shape(glc, ctx, cuda):
    """kinds 0, 1, 2 and 4 in one version-6 stream (no GPU writer makes it), read by plans of other n, rows and settings"""
    gold = open(GOLD, "rb").read()
    x, kinds = R.read(gold, with_kinds=True)
    assert set(kinds) == {0, 1, 2, 4}
    g = np.frombuffer(gold, np.uint8)
    for n, rows, filt, pipelined in ((1024, 4, "plain", False), (1024, 1, "delta8", True), (70000, 2, "shuffle4", False), (5000, 3, "plain", True)):
        with _plan(glc, ctx, n, filt, pipelined, rows=rows) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert np.array_equal(glc.container_decompress_host(plan, g), x)
            assert glc.container_last_error(plan) == (0, -1, -1)
    y = _input(4096, "text")
    c = R.write(y, 4096, ROWS, kinds=(4, 0, 4, 4, 2, 4, 1, 0, 0, 4))
    with _plan(glc, ctx, 4096, rows=2) as plan:                  # (decoder chunks of two blocks: runs of kind 4 cut at their edges)
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), y)


# --- 2. the mode off ---------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_a_plan_with_the_mode_off_refuses_version_6_and_writes_as_ever(glc, ctx, cuda, tmp_path):
    import torch
    x, c6 = _input(4096, "text"), _want(4096, "text", "plain")
    src = tmp_path / "c6.glcb"
    src.write_bytes(c6)
    with pytest.raises(M.ContainerError) as merr:
        R.read(c6, runs=False)
    assert (merr.value.what, merr.value.frame, merr.value.block) == (1, -1, -1)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 4096, rows=ROWS) as never:           # a plan that never heard of the mode
        before = _host(glc.container_compress(never, _gpu(x))).tobytes()
    assert before == M.write(x, 4096, ROWS)
    for codec, sparse in ((0, 0), (1, 0), (1, 1)):
        with _plan(glc, ctx, 4096, runs=False) as plan:
            glc.container_set_codec(plan, codec)
            glc.container_set_sparse(plan, sparse)
            out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, c6, out, x.size)
            assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
            assert bool((out == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(c6, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_file(plan, str(src), str(tmp_path / "back.bin"))
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_index(plan, _gpu(np.frombuffer(c6, np.uint8)))
            assert glc.container_last_error(plan) == (1, -1, -1)
    with _plan(glc, ctx, 4096) as plan:                           # on, then off again: the old bytes again; on: older versions read
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == c6
        for older in (before, M.write(x, 4096, ROWS, 4), M.write(x, 4096, ROWS, 0, 1), M.write(x, 4096, ROWS, 2, 0, True)):
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(older, np.uint8)))), x)
        glc.container_set_runs(plan, 0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == before
        import sparse_model as S
        c5 = S.write(x, 4096, ROWS)
        glc.container_set_runs(plan, 1)
        with pytest.raises(glc.CudppError):                       # no single plan reads both 5 and 6
            glc.container_decompress(plan, _gpu(np.frombuffer(c5, np.uint8)))
        assert glc.container_last_error(plan) == (1, -1, -1)


# --- 3. the setters ----------------------------------------------------------------------------------------------------------
def test_setters(glc, ctx, cuda):
    x = _input(4096, "log")
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 4096, rows=ROWS) as plan:
        assert glc.container_get_runs(plan) == 0
        for bad in (2, 3, 255, 1 << 31):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_runs(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_runs(plan) == 0
        glc.container_set_runs(plan, 1)
        for bad in (2, 1 << 31):
            with pytest.raises(glc.CudppError):
                glc.container_set_runs(plan, bad)
            assert glc.container_get_runs(plan) == 1            # unchanged
        for codec in (2, 7):                                    # a refused codec changes nothing
            with pytest.raises(glc.CudppError):
                glc.container_set_codec(plan, codec)
        assert glc.container_get_runs(plan) == 1 and glc.container_get_codec(plan) == 0
        with pytest.raises(glc.CudppError):                     # the sparse mode needs the other codec
            glc.container_set_sparse(plan, 1)
        glc.container_set_shuffle(plan, 4)                      # the filter settings leave it alone
        glc.container_set_delta(plan, 1)
        glc.container_set_delta(plan, 0)
        glc.container_set_shuffle(plan, 0)
        assert glc.container_get_runs(plan) == 1
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(4096, "log", "plain")
        glc.container_set_codec(plan, 0)                        # the same codec again: still on
        assert glc.container_get_runs(plan) == 1
        glc.container_set_codec(plan, 1)                        # the order-0 codec: runs off, and it stays off
        assert glc.container_get_runs(plan) == 0
        with pytest.raises(glc.CudppError) as e:
            glc.container_set_runs(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_runs(plan) == 0
        glc.container_set_runs(plan, 0)                         # off is always legal
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, 4096, ROWS, 0, 1)
        glc.container_set_codec(plan, 0)
        assert glc.container_get_runs(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, 4096, ROWS)


# --- 4. refusals -------------------------------------------------------------------------------------------------------------
def _refusal_input(n):
    import datagen
    return np.concatenate([datagen.text_bytes(n // 2, seed=31), np.zeros(n // 8, np.uint8), datagen.log_bytes(n - n // 2 - n // 8, seed=32)])


@pytest.mark.parametrize("block_len,filt", ((4096, "plain"), (1000, "plain"), (4096, "delta8")))
def test_refusals_of_version_6(glc, ctx, cuda, block_len, filt):
    import torch
    elem, delta = FILTERS[filt]
    x = _refusal_input(2 * 3 * block_len + 321)
    c6 = R.write(x, block_len, 3, elem, delta)
    cases, _ = R.refusal_cases(c6, elem)
    assert all("%d:" % k in " ".join(name for name, _, _ in cases) for k in range(1, 10))
    guard = 64
    with _plan(glc, ctx, block_len, filt, rows=3) as plan:
        for name, cont, want in cases:
            with pytest.raises(M.ContainerError) as merr:          # the model
                R.read(cont)
            assert (merr.value.what, merr.value.frame, merr.value.block) == want, name
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN, name
            assert glc.container_last_error(plan) == want, name
            assert bool((out[x.size:] == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want, name
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c6, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_mode_on(glc, ctx, cuda):
    import torch
    x, want = _input(4096, "text"), _want(4096, "text", "plain")
    need = len(want)
    with _plan(glc, ctx, 4096) as plan:
        for cap in (need - 1, need // 2, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need and _host(c).tobytes() == want


# --- 5. range reads ----------------------------------------------------------------------------------------------------------
def _want_stats(c, a, n, flags, elem):
    frames = [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]]
    return RM.stats_of(frames, a, n, 5, flags, elem)             # (version 6 has version 5's triples and filters)


@pytest.mark.parametrize("filt", list(FILTERS))
def test_range_reads_of_a_version_6_container(glc, ctx, cuda, tmp_path, filt):
    import torch
    n = 4096
    elem, delta = FILTERS[filt]
    x, c = _input(n, "text"), _want(n, "text", filt)
    F = ROWS * n
    assert x.size > 2 * F
    d_c = _gpu(np.frombuffer(c, np.uint8))
    path = tmp_path / "c.glcb"
    path.write_bytes(c)
    ranges = [(100, 50), (n + 7, 1), (n - 3, 7), (2 * n - 1, n + 2), (F - 5, 11), (2 * F - 300, 301), (0, x.size), (x.size - 1, 1), (5, 0)]
    with _plan(glc, ctx, n, filt) as plan:
        with glc.container_index(plan, d_c) as ix:
            assert ix.info() == (x.size, n, 3, 6, 1 if delta else 0, elem)
            for a, k in ranges:
                buf = torch.full((k + 64,), 0xCD, dtype=torch.uint8, device=cuda)
                out = glc.container_read_range(plan, ix, d_c, a, k, out=buf[3:3 + max(k, 1)])
                assert out.numel() == k and np.array_equal(_host(buf[3:3 + k]), x[a:a + k]), (a, k)
                assert bool((buf[:3] == 0xCD).all()) and bool((buf[3 + k:] == 0xCD).all())
                assert glc.container_last_error(plan) == (0, -1, -1)
                st = glc.container_last_range_stats(plan)
                assert tuple(st[:2]) == (_want_stats(c, a, k, 1 if delta else 0, elem) if k else (0, 0)), (a, k, st)
            if filt == "plain":                                 # blocks decoded as predicted: one, two, and two across the frame edge
                for (a, k), blocks in (((100, 50), 1), ((n - 3, 7), 2), ((F - 5, 11), 2)):
                    glc.container_read_range(plan, ix, d_c, a, k)
                    assert glc.container_last_range_stats(plan)[1] == blocks
        hc = np.frombuffer(c, np.uint8)
        with glc.container_index_host(plan, hc) as ixh, glc.container_index_file(plan, str(path)) as ixf:
            for a, k in ((F - 5, 11), (x.size - 500, 300)):
                out = np.full(k + 16, 0xCD, np.uint8)
                glc.container_read_range_host(plan, ixh, hc, a, k, out=out[8:])
                assert np.array_equal(out[8:8 + k], x[a:a + k]) and (out[:8] == 0xCD).all() and (out[8 + k:] == 0xCD).all()
                out = np.full(k + 16, 0xCD, np.uint8)
                glc.container_read_range_file(plan, ixf, str(path), a, k, out=out[8:])
                assert np.array_equal(out[8:8 + k], x[a:a + k]) and (out[:8] == 0xCD).all() and (out[8 + k:] == 0xCD).all()
        assert np.array_equal(_host(glc.container_decompress(plan, d_c)), x)
