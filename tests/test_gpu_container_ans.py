"""The rANS mode of the container's order-0 codec on the MI355X (-m gpu): with it on, the device, host-pointer and file entry
points write the bytes of the Python model of format version 7 (tests/ans_model.py) for every element size, delta off and on and
pipelining off and on, at n = 70000 (two whole chunks and a part per block) and n = 8192, and read them back; range reads give the
input's slices and decode only the blocks range_model says; the golden fixture decodes; every other plan refuses version 7 as
ever and the mode-on plan reads versions 1 to 4 and refuses 5 and 6; with the mode off a plan writes versions 3 and 4 as ever; the
setters' rules; refusals with their glcContainerLastError triples; capacity."""
import os
import struct

import numpy as np
import pytest

import ans_inputs as I
import ans_model as A
import container_model as M
import range_model
import sparse_inputs

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
    return I.container_input(elem, delta) if n == N else sparse_inputs.container_input(elem, delta)


def _want(elem, delta, n=N):
    if (elem, delta, n) not in _WANT:
        _WANT[elem, delta, n] = A.write(_input(elem, delta, n), n, I.rows_of(elem), elem, delta)
    return _WANT[elem, delta, n]


def _plan(glc, ctx, elem, delta=False, pipelined=False, ans=True, n=N, rows=None, codec=1):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows or I.rows_of(elem))
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if delta:
        glc.container_set_delta(plan, 1)
    if ans:
        glc.container_set_ans(plan, 1)
    return plan


# --- 1. the mode on: byte-identical to the model, and read back -----------------------------------------------------------
@pytest.mark.parametrize("elem,delta", CASES)
@pytest.mark.parametrize("pipelined", [False, True])
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, elem, delta, pipelined):
    x, want = I.container_input(elem, delta), _want(elem, delta)
    rows = I.rows_of(elem)
    assert struct.unpack("<HHII", want[4:16]) == (7, 1 if delta else 0, N, elem)
    frames = M.layout(want)["frames"]
    assert [f["nb"] for f in frames] == [rows, rows, 1] and frames[-1]["blk_len"] == 1235
    assert {k for f in frames for _, _, k in f["records"]} == {M.RAW, A.ANS}
    assert [k for _, _, k in frames[1]["records"]][:3] == [M.RAW, A.ANS, A.ANS]
    s, e, _ = frames[1]["records"][1]
    assert e - s == 4 * (3 + 3 * 64)                             # the constant block: three counts of 0 and three chunks' states
    with _plan(glc, ctx, elem, delta, pipelined) as plan:
        assert glc.container_get_ans(plan) == 1
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
        for L in (0, 1):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == A.write(y, N, rows, elem, delta)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused
    assert np.array_equal(A.read(want), x)


@pytest.mark.parametrize("elem,delta", CASES)
def test_blocks_of_one_short_chunk(glc, ctx, cuda, elem, delta):
    """n = 8192 over the sparse tests' input: constant, sparse and dense blocks, one chunk each"""
    x, want = _input(elem, delta, 8192), _want(elem, delta, 8192)
    with _plan(glc, ctx, elem, delta, n=8192) as plan:
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        assert np.array_equal(glc.container_decompress_host(plan, _host(c)), x)


# --- 2. range reads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", [(0, False), (4, False), (8, True)])
def test_range_reads(glc, ctx, cuda, tmp_path, elem, delta):
    x, want = I.container_input(elem, delta), _want(elem, delta)
    rows = I.rows_of(elem)
    F = rows * N
    shape = [(rows, N), (rows, N), (1, 1235)]
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    # inside a chunk; from inside one chunk to inside the next block's; across the frame edge; into the tail; everything
    ranges = [(40000, 100), (N + 30000, N), (F - 5000, 10000), (2 * F - 10, 500), (0, x.size), (x.size, 0), (F + 3 * N - 1, 2)]
    with _plan(glc, ctx, elem, delta) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, N, 3, 7, 1 if delta else 0, elem)
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
                stats = glc.container_last_range_stats(plan)
                assert stats[:2] == range_model.stats_of(shape, off, cnt, 5, 1 if delta else 0, elem), (off, cnt)   # (version 5's triples are version 7's)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            for off, cnt in ranges[:4]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
        with glc.container_index_file(plan, str(path)) as ix:
            off, cnt = ranges[2]
            assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
    with _plan(glc, ctx, elem, delta, ans=False) as plan:          # a plan without the mode cannot index the stream either
        with pytest.raises(glc.CudppError):
            glc.container_index(plan, d)
        assert glc.container_last_error(plan) == (1, -1, -1)


# --- 3. decoding -----------------------------------------------------------------------------------------------------------
def test_gpu_reads_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "container_v7_ans.bin"), "rb").read()
    x, kinds = A.read(gold, with_kinds=True)
    assert {0, 1, 2, 5} == set(kinds)
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


def test_every_other_plan_refuses_version_7_as_ever(glc, ctx, cuda, tmp_path):
    """the setting is the version a plan speaks: a default plan, a sparse-mode plan and a runs-mode plan refuse a version-7 stream
    as a stream-header failure with nothing written; with the mode on the same plan reads it"""
    import torch
    gold = open(os.path.join(GOLDEN, "container_v7_ans.bin"), "rb").read()
    x = A.read(gold)
    src = tmp_path / "gold.glcb"
    src.write_bytes(gold)

    def default(plan):
        pass

    def sparse(plan):
        glc.container_set_codec(plan, 1)
        glc.container_set_sparse(plan, 1)

    def runs(plan):
        glc.container_set_runs(plan, 1)

    def order0(plan):
        glc.container_set_codec(plan, 1)

    for setup in (default, sparse, runs, order0):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=3) as plan:
            setup(plan)
            out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, gold, out, x.size)
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
            glc.container_set_ans(plan, 1)
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(gold, np.uint8)))), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


def test_the_mode_on_plan_reads_versions_1_to_4_and_refuses_5_and_6(glc, ctx, cuda):
    x = sparse_inputs.container_input(8, True)[:3 * 8192 + 77]
    older = [M.write(x, 8192, 3), M.write(x, 8192, 3, 8), M.write(x, 8192, 3, 8, 1), M.write(x, 8192, 3, 8, 1, delta=True)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4]
    with _plan(glc, ctx, 8, True, n=8192, rows=3) as plan:
        for c in older:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
        for name in ("container_v5_sparse.bin", "container_v6_runs.bin"):
            g = np.frombuffer(open(os.path.join(GOLDEN, name), "rb").read(), np.uint8)
            with pytest.raises(glc.CudppError) as err:
                glc.container_decompress(plan, _gpu(g))
            assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, g)
            assert glc.container_last_error(plan) == (1, -1, -1)


def test_a_plan_with_the_mode_off_writes_versions_3_and_4_as_ever(glc, ctx, cuda):
    for elem, delta in ((0, False), (4, False), (8, True)):
        x = _input(elem, delta, 8192)
        rows = I.rows_of(elem)
        want = M.write(x, 8192, rows, elem, 1, delta=delta)
        with _plan(glc, ctx, elem, delta, ans=False, n=8192) as plan:
            assert glc.container_get_ans(plan) == 0
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want and struct.unpack("<H", want[4:6])[0] == (4 if delta else 3)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            glc.container_set_ans(plan, 1)                      # on: version 7; off again: the old bytes again
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(elem, delta, 8192)
            for older in (_want(elem, delta, 8192), want):      # with the mode on a plan reads the older versions too
                assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(older, np.uint8)))), x)
            glc.container_set_ans(plan, 0)
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want


# --- 4. the setters --------------------------------------------------------------------------------------------------------
def test_setters(glc, ctx, cuda):
    x = _input(4, False, 8192)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=4) as plan:
        assert glc.container_get_ans(plan) == 0
        with pytest.raises(glc.CudppError) as e:                # the codec is the BWT one
            glc.container_set_ans(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_ans(plan) == 0
        glc.container_set_ans(plan, 0)                          # off is always legal
        with pytest.raises(glc.CudppError) as e:                # there is no third codec
            glc.container_set_codec(plan, 2)
        assert e.value.code == ILLEGAL and glc.container_get_codec(plan) == 0
        glc.container_set_codec(plan, 1)
        for bad in (2, 3, 255, 1 << 31):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_ans(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_ans(plan) == 0
        glc.container_set_sparse(plan, 1)                       # the two modes exclude each other, either way round
        with pytest.raises(glc.CudppError) as e:
            glc.container_set_ans(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_ans(plan) == 0 and glc.container_get_sparse(plan) == 1
        glc.container_set_sparse(plan, 0)
        glc.container_set_ans(plan, 1)
        with pytest.raises(glc.CudppError) as e:
            glc.container_set_sparse(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_ans(plan) == 1 and glc.container_get_sparse(plan) == 0
        glc.container_set_sparse(plan, 0)
        with pytest.raises(glc.CudppError) as e:                # the runs mode needs the BWT codec
            glc.container_set_runs(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_ans(plan) == 1
        for bad in (2, 1 << 31):
            with pytest.raises(glc.CudppError):
                glc.container_set_ans(plan, bad)
            assert glc.container_get_ans(plan) == 1             # unchanged
        with pytest.raises(glc.CudppError):                     # a refused codec changes nothing
            glc.container_set_codec(plan, 7)
        assert glc.container_get_ans(plan) == 1 and glc.container_get_codec(plan) == 1
        glc.container_set_shuffle(plan, 4)                      # the filter settings leave it alone
        glc.container_set_delta(plan, 1)
        glc.container_set_delta(plan, 0)
        assert glc.container_get_ans(plan) == 1
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(4, False, 8192)
        glc.container_set_codec(plan, 0)                        # back to the BWT codec: the mode off, and it stays off
        assert glc.container_get_ans(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, 8192, 4, 4)
        glc.container_set_codec(plan, 1)
        assert glc.container_get_ans(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, 8192, 4, 4, 1)


# --- 5. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta,n", [(0, False, N), (8, True, N), (4, False, 8192)])
def test_refusals_of_version_7(glc, ctx, cuda, elem, delta, n):
    import torch
    x, c7 = _input(elem, delta, n), _want(elem, delta, n)
    cases, lay = A.refusal_cases(c7, elem)
    assert len(cases) >= 19
    guard = 64
    with _plan(glc, ctx, elem, delta, n=n) as plan:
        for name, cont, want in cases:
            with pytest.raises(M.ContainerError) as merr:          # the model
                A.read(cont)
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
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c7, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_mode_on(glc, ctx, cuda):
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
        out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
        with pytest.raises(glc.CudppError) as e:
            _decompress_into(glc, plan, _host(c).tobytes(), out, x.size - 1)
        assert e.value.code == ILLEGAL and bool((out == 0xAB).all())
