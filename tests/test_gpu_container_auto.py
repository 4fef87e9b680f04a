"""The auto mode of the container's order-0 codec on the MI355X (-m gpu): with it on, the device, host-pointer and file entry
points write the bytes of the Python model of format version 8 (tests/auto_model.py) for every element size, delta off and on and
pipelining off and on, at n = 70000 and n = 8192 over ans_inputs.container_input and at n = 4099 (misaligned blocks with a short
last chunk), and read them back; range reads give the input's slices and decode only the blocks range_model says; the golden
fixture decodes; every other plan refuses version 8 as it refuses an unknown version and the mode-on plan reads versions 1 to 5
and 7 and refuses 6; mode on then off gives the old bytes again; the setters' rules; refusals with their glcContainerLastError
triples; capacity."""
import os
import struct

import numpy as np
import pytest

import ans_inputs as I
import ans_model as A
import auto_inputs as AI
import auto_model as U
import container_model as M
import range_model
import sparse_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL, UNKNOWN = 2, 9999
N = 70000
CASES = [(0, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)]


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


def _input(elem, delta, n):
    return AI.odd_input(elem, delta) if n == AI.ODD else I.container_input(elem, delta, n=n)


def _want(elem, delta, n=N):
    if (elem, delta, n) not in _WANT:
        _WANT[elem, delta, n] = U.write(_input(elem, delta, n), n, I.rows_of(elem), elem, delta)
    return _WANT[elem, delta, n]


def _plan(glc, ctx, elem, delta=False, pipelined=False, auto=True, n=N, rows=None, codec=1):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows or I.rows_of(elem))
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if delta:
        glc.container_set_delta(plan, 1)
    if auto:
        glc.container_set_auto(plan, 1)
    return plan


# --- 1. the mode on: byte-identical to the model, and read back -----------------------------------------------------------
@pytest.mark.parametrize("n", [N, 8192])
@pytest.mark.parametrize("elem,delta", CASES)
@pytest.mark.parametrize("pipelined", [False, True])
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, elem, delta, pipelined, n):
    x, want = _input(elem, delta, n), _want(elem, delta, n)
    rows = I.rows_of(elem)
    assert struct.unpack("<HHII", want[4:16]) == (8, 1 if delta else 0, n, elem)
    frames = M.layout(want)["frames"]
    assert [f["nb"] for f in frames] == [rows, rows, 1] and frames[-1]["blk_len"] == 1235
    assert {k for f in frames for _, _, k in f["records"]} == {M.RAW, M.HUFF0, S.SPARSE, A.ANS}
    with _plan(glc, ctx, elem, delta, pipelined, n=n) as plan:
        assert glc.container_get_auto(plan) == 1
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert c.numel() <= glc.container_bound(x.size, n)
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
        for L in (0, 1):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == U.write(y, n, rows, elem, delta)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused
    assert np.array_equal(U.read(want), x)


@pytest.mark.parametrize("elem,delta", CASES)
def test_misaligned_blocks_with_a_short_last_chunk(glc, ctx, cuda, elem, delta):
    """n = 4099: every block but the first starts off a 16-byte boundary, and chunk 64 of a block holds 3 bytes"""
    x, want = _input(elem, delta, AI.ODD), _want(elem, delta, AI.ODD)
    assert {M.HUFF0, S.SPARSE, A.ANS} <= {k for f in M.layout(want)["frames"] for _, _, k in f["records"]}
    for pipelined in (False, True):
        with _plan(glc, ctx, elem, delta, pipelined, n=AI.ODD) as plan:
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            assert glc.container_compress_host(plan, x).tobytes() == want
            assert np.array_equal(glc.container_decompress_host(plan, _host(c)), x)


# --- 2. range reads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", [(0, False), (4, False), (8, True)])
def test_range_reads(glc, ctx, cuda, tmp_path, elem, delta):
    x, want = _input(elem, delta, N), _want(elem, delta)
    rows = I.rows_of(elem)
    F = rows * N
    shape = [(rows, N), (rows, N), (1, 1235)]
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(40000, 100), (N + 30000, N), (F - 5000, 10000), (2 * F - 10, 500), (0, x.size), (x.size, 0), (F + 3 * N - 1, 2)]
    with _plan(glc, ctx, elem, delta) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, N, 3, 8, 1 if delta else 0, elem)
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                stats = glc.container_last_range_stats(plan)
                assert stats[:2] == range_model.stats_of(shape, off, cnt, 5, 1 if delta else 0, elem), (off, cnt)   # (version 5's triples are version 8's)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            for off, cnt in ranges[:4]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
        with glc.container_index_file(plan, str(path)) as ix:
            off, cnt = ranges[2]
            assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_auto(plan, 0)                     # the index outlives the setting; the plan no longer speaks the version
            glc.container_set_ans(plan, 1)
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), off, cnt)
            assert glc.container_last_error(plan) == (1, -1, -1)
    with _plan(glc, ctx, elem, delta, auto=False) as plan:         # a plan without the mode cannot index the stream either
        with pytest.raises(glc.CudppError):
            glc.container_index(plan, d)
        assert glc.container_last_error(plan) == (1, -1, -1)


# --- 3. decoding -----------------------------------------------------------------------------------------------------------
def test_gpu_reads_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "container_v8_auto.bin"), "rb").read()
    x, kinds = U.read(gold, with_kinds=True)
    assert {0, 1, 2, 3, 5} == set(kinds)
    g = np.frombuffer(gold, np.uint8)
    for n, rows, elem, delta, pipelined in ((8192, 3, 8, True, False), (8192, 1, 0, False, True), (70000, 2, 4, True, False)):
        with _plan(glc, ctx, elem, delta, pipelined, n=n, rows=rows) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert np.array_equal(glc.container_decompress_host(plan, g), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_every_other_plan_refuses_version_8(glc, ctx, cuda, tmp_path):
    """the setting is the version a plan speaks: a default plan, a sparse plan, an rANS plan, a runs plan and a plain order-0
    plan refuse a version-8 stream as a stream-header failure with nothing written -- exactly how they answer a version no plan
    knows; with the mode on the same plan reads it"""
    import torch
    gold = open(os.path.join(GOLDEN, "container_v8_auto.bin"), "rb").read()
    unknown = M.with_header(gold, 9, 1, 8)
    x = U.read(gold)
    src = tmp_path / "gold.glcb"
    src.write_bytes(gold)

    def default(plan):
        pass

    def sparse(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_sparse(plan, 1)

    def ans(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_ans(plan, 1)

    def runs(plan):
        glc.container_set_runs(plan, 1)

    def order0(plan):
        glc.container_set_codec(plan, 1)

    for setup in (default, sparse, ans, runs, order0):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=3) as plan:
            setup(plan)
            for cont in (gold, unknown):
                out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
                with pytest.raises(glc.CudppError) as err:
                    _decompress_into(glc, plan, cont, out, x.size)
                assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
                assert bool((out == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(gold, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_file(plan, str(src), str(tmp_path / "back.bin"))
            assert glc.container_last_error(plan) == (1, -1, -1)
            glc.container_set_codec(plan, 1)
            glc.container_set_sparse(plan, 0)
            glc.container_set_ans(plan, 0)
            glc.container_set_auto(plan, 1)
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(gold, np.uint8)))), x)
            assert glc.container_last_error(plan) == (0, -1, -1)
            with pytest.raises(glc.CudppError):                 # and a version no plan knows stays one
                glc.container_decompress_host(plan, np.frombuffer(unknown, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == (1, -1, -1)


def test_the_mode_on_plan_reads_versions_1_to_5_and_7_and_refuses_6(glc, ctx, cuda):
    x = AI.odd_input(8, True)[:3 * 8192 + 77]
    older = [M.write(x, 8192, 3), M.write(x, 8192, 3, 8), M.write(x, 8192, 3, 8, 1), M.write(x, 8192, 3, 8, 1, delta=True),
             S.write(x, 8192, 3, 8, True), A.write(x, 8192, 3, 8, True)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4, 5, 7]
    with _plan(glc, ctx, 8, True, n=8192, rows=3) as plan:
        for c in older:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
            assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(c, np.uint8)), x)
        for name, model in (("container_v5_sparse.bin", S), ("container_v7_ans.bin", A)):
            g = open(os.path.join(GOLDEN, name), "rb").read()
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(g, np.uint8)))), model.read(g))
        g = np.frombuffer(open(os.path.join(GOLDEN, "container_v6_runs.bin"), "rb").read(), np.uint8)
        with pytest.raises(glc.CudppError) as err:
            glc.container_decompress(plan, _gpu(g))
        assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
        with pytest.raises(glc.CudppError):
            glc.container_decompress_host(plan, g)
        assert glc.container_last_error(plan) == (1, -1, -1)


def test_mode_on_then_off_gives_the_old_bytes_again(glc, ctx, cuda):
    for elem, delta in ((0, False), (4, False), (8, True)):
        x = _input(elem, delta, 8192)
        rows = I.rows_of(elem)
        want = M.write(x, 8192, rows, elem, 1, delta=delta)
        with _plan(glc, ctx, elem, delta, auto=False, n=8192) as plan:
            assert glc.container_get_auto(plan) == 0
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want and struct.unpack("<H", want[4:6])[0] == (4 if delta else 3)
            glc.container_set_auto(plan, 1)                     # on: version 8
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(elem, delta, 8192)
            for older in (_want(elem, delta, 8192), want):      # with the mode on a plan reads the older versions too
                assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(older, np.uint8)))), x)
            glc.container_set_auto(plan, 0)                     # off again: the old bytes again
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
            glc.container_set_sparse(plan, 1)                   # and the other modes write what they always wrote
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == S.write(x, 8192, rows, elem, delta)
            glc.container_set_sparse(plan, 0)
            glc.container_set_ans(plan, 1)
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == A.write(x, 8192, rows, elem, delta)


# --- 4. the setters --------------------------------------------------------------------------------------------------------
def test_setters(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        _setter_rules(glc, plan)


def _setter_rules(glc, plan):
    ILLEGAL = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

    def refused(call, *a):
        with pytest.raises(glc.CudppError) as e:
            call(plan, *a)
        return e.value.code == ILLEGAL

    assert glc.container_get_auto(plan) == 0
    assert refused(glc.container_set_auto, 1) and glc.container_get_auto(plan) == 0          # the codec is the BWT one
    glc.container_set_auto(plan, 0)                                                         # off is always legal
    glc.container_set_codec(plan, 1)
    for bad in (2, 3, 255, 1 << 31):
        assert refused(glc.container_set_auto, bad) and glc.container_get_auto(plan) == 0
    for other_set, other_get in ((glc.container_set_sparse, glc.container_get_sparse), (glc.container_set_ans, glc.container_get_ans)):
        other_set(plan, 1)                                                                  # the modes exclude each other, both ways
        assert refused(glc.container_set_auto, 1) and glc.container_get_auto(plan) == 0 and other_get(plan) == 1
        other_set(plan, 0)
        glc.container_set_auto(plan, 1)
        assert refused(other_set, 1) and glc.container_get_auto(plan) == 1 and other_get(plan) == 0
        other_set(plan, 0)
        assert glc.container_get_auto(plan) == 1
        glc.container_set_auto(plan, 0)
    glc.container_set_auto(plan, 1)
    assert refused(glc.container_set_runs, 1) and glc.container_get_auto(plan) == 1          # the runs mode needs the BWT codec
    for bad in (2, 1 << 31):
        assert refused(glc.container_set_auto, bad) and glc.container_get_auto(plan) == 1    # unchanged
    assert refused(glc.container_set_codec, 7) and glc.container_get_auto(plan) == 1 and glc.container_get_codec(plan) == 1
    glc.container_set_shuffle(plan, 4)                                                      # the filter settings leave it alone
    glc.container_set_delta(plan, 1)
    glc.container_set_delta(plan, 0)
    assert glc.container_get_auto(plan) == 1
    glc.container_set_codec(plan, 0)                                                        # back to the BWT codec: off, and it stays off
    assert glc.container_get_auto(plan) == 0
    glc.container_set_runs(plan, 1)
    assert refused(glc.container_set_auto, 1)
    glc.container_set_codec(plan, 1)
    assert glc.container_get_auto(plan) == 0 and glc.container_get_runs(plan) == 0
    glc.container_set_auto(plan, 1)
    assert glc.container_get_auto(plan) == 1


# --- 5. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", [(0, False), (8, True), (4, False)])
def test_refusals_of_version_8(glc, ctx, cuda, elem, delta):
    import torch
    n = AI.ODD
    x, c8 = _input(elem, delta, n), _want(elem, delta, n)
    cases, lay = U.refusal_cases(c8, elem)
    assert len(cases) >= 30
    guard = 64
    with _plan(glc, ctx, elem, delta, n=n) as plan:
        for name, cont, want in cases:
            with pytest.raises(M.ContainerError) as merr:          # the model
                U.read(cont)
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
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c8, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_mode_on(glc, ctx, cuda):
    import torch
    elem, delta = 8, True
    x, need = _input(elem, delta, N), len(_want(elem, delta))
    with _plan(glc, ctx, elem, delta) as plan:
        for cap in (need - 1, need // 2, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need and _host(c).tobytes() == _want(elem, delta)
        out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
        with pytest.raises(glc.CudppError) as e:
            _decompress_into(glc, plan, _host(c).tobytes(), out, x.size - 1)
        assert e.value.code == ILLEGAL and bool((out == 0xAB).all())
