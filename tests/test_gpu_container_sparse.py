"""The sparse mode of the container's order-0 codec on the MI355X (-m gpu): with it on, the device, host-pointer and file entry
points write the bytes of the Python model of format version 5 (tests/sparse_model.py) for every element size, delta off and on and
pipelining off and on, and read them back; the golden fixture decodes; with it off a plan writes versions 3 and 4 as ever and
refuses version 5 as ever; the setters' rules; refusals with their glcContainerLastError triples; capacity."""
import os
import struct

import numpy as np
import pytest

import container_model as M
import sparse_inputs as I
import sparse_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL, UNKNOWN = 2, 9999
N = 8192
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


def _want(elem, delta):
    if (elem, delta) not in _WANT:
        _WANT[elem, delta] = S.write(I.container_input(elem, delta), N, I.rows_of(elem), elem, delta)
    return _WANT[elem, delta]


def _plan(glc, ctx, elem, delta=False, pipelined=False, sparse=True, n=N, rows=None, codec=1):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows or I.rows_of(elem))
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if delta:
        glc.container_set_delta(plan, 1)
    if sparse:
        glc.container_set_sparse(plan, 1)
    return plan


# --- 1. sparse on: byte-identical to the model, and read back ------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", CASES)
@pytest.mark.parametrize("pipelined", [False, True])
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, elem, delta, pipelined):
    x, want = I.container_input(elem, delta), _want(elem, delta)
    rows = I.rows_of(elem)
    assert struct.unpack("<HHII", want[4:16]) == (5, 1 if delta else 0, N, elem)
    frames = M.layout(want)["frames"]
    assert [f["nb"] for f in frames] == [rows, rows, rows, 2, 1] and frames[-1]["blk_len"] == 1235
    assert {k for f in frames for _, _, k in f["records"]} == {M.RAW, M.HUFF0, S.SPARSE}
    assert {k for _, _, k in frames[1]["records"]} == {M.RAW} and [k for _, _, k in frames[2]["records"]][:2] == [S.SPARSE, M.HUFF0]
    s, e, _ = frames[2]["records"][0]
    assert e - s == 4 * S.mask_words(N)                          # the constant block: the mask alone
    with _plan(glc, ctx, elem, delta, pipelined) as plan:
        assert glc.container_get_sparse(plan) == 1
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
            assert _host(c).tobytes() == S.write(y, N, rows, elem, delta)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # the plan's scratch reused
    assert np.array_equal(S.read(want), x)


# --- 2. decoding -----------------------------------------------------------------------------------------------------------
def test_gpu_reads_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "container_v5_sparse.bin"), "rb").read()
    x, kinds = S.read(gold, with_kinds=True)
    assert {0, 1, 2, 3} == set(kinds)
    g = np.frombuffer(gold, np.uint8)
    for n, rows, elem, delta, pipelined in ((4096, 8, 8, True, False), (4096, 1, 0, False, True), (70000, 2, 4, True, False),
                                            (5000, 3, 2, False, True)):
        with _plan(glc, ctx, elem, delta, pipelined, n=n, rows=rows) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert np.array_equal(glc.container_decompress_host(plan, g), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


def test_a_plan_with_sparse_off_is_the_version_4_reader_it_was(glc, ctx, cuda, tmp_path):
    """the setting is the version a plan speaks: off, a version-5 stream is a stream-header failure (as to the model's reader
    with max_version=4, and as before version 5 existed) with nothing written; on, the same plan reads it"""
    import torch
    gold = open(os.path.join(GOLDEN, "container_v5_sparse.bin"), "rb").read()
    x = S.read(gold)
    with pytest.raises(M.ContainerError) as merr:
        S.read(gold, max_version=4)
    assert (merr.value.what, merr.value.frame, merr.value.block) == (1, -1, -1)
    src = tmp_path / "gold.glcb"
    src.write_bytes(gold)
    for codec in (0, 1):
        with _plan(glc, ctx, 8, True, sparse=False, n=4096, rows=8, codec=codec) as plan:
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
            glc.container_set_sparse(plan, 1)
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(gold, np.uint8)))), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


def test_a_plan_with_sparse_off_writes_versions_3_and_4_as_ever(glc, ctx, cuda):
    for elem, delta in ((0, False), (4, False), (8, True)):
        x = I.container_input(elem, delta)
        rows = I.rows_of(elem)
        want = M.write(x, N, rows, elem, 1, delta=delta)
        with _plan(glc, ctx, elem, delta, sparse=False) as plan:
            assert glc.container_get_sparse(plan) == 0
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want and struct.unpack("<H", want[4:6])[0] == (4 if delta else 3)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            glc.container_set_sparse(plan, 1)                   # on: version 5; off again: the old bytes again
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(elem, delta)
            for older in (_want(elem, delta), want):            # with the mode on a plan reads the older versions too
                assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(older, np.uint8)))), x)
            glc.container_set_sparse(plan, 0)
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want


# --- 3. the setters --------------------------------------------------------------------------------------------------------
def test_setters(glc, ctx, cuda):
    x = I.container_input(4, False)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=4) as plan:
        assert glc.container_get_sparse(plan) == 0
        with pytest.raises(glc.CudppError) as e:                # the codec is the BWT one
            glc.container_set_sparse(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_sparse(plan) == 0
        glc.container_set_sparse(plan, 0)                       # off is always legal
        glc.container_set_codec(plan, 1)
        for bad in (2, 3, 255, 1 << 31):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_sparse(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_sparse(plan) == 0
        glc.container_set_sparse(plan, 1)
        for bad in (2, 1 << 31):
            with pytest.raises(glc.CudppError):
                glc.container_set_sparse(plan, bad)
            assert glc.container_get_sparse(plan) == 1          # unchanged
        with pytest.raises(glc.CudppError):                     # a refused codec changes nothing
            glc.container_set_codec(plan, 7)
        assert glc.container_get_sparse(plan) == 1 and glc.container_get_codec(plan) == 1
        glc.container_set_shuffle(plan, 4)                      # the filter settings leave it alone
        glc.container_set_delta(plan, 1)
        glc.container_set_delta(plan, 0)
        assert glc.container_get_sparse(plan) == 1
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(4, False)
        glc.container_set_codec(plan, 0)                        # back to the BWT codec: sparse off, and it stays off
        assert glc.container_get_sparse(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, N, 4, 4)
        glc.container_set_codec(plan, 1)
        assert glc.container_get_sparse(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, N, 4, 4, 1)


# --- 4. refusals ---------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


@pytest.mark.parametrize("elem,delta", [(0, False), (8, True)])
def test_refusals_of_version_5(glc, ctx, cuda, elem, delta):
    import torch
    x, c5 = I.container_input(elem, delta), _want(elem, delta)
    cases, lay = S.refusal_cases(c5, elem)
    assert len(cases) >= 13
    guard = 64
    with _plan(glc, ctx, elem, delta) as plan:
        for name, cont, want in cases:
            with pytest.raises(M.ContainerError) as merr:          # the model
                S.read(cont)
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
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c5, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_sparse_mode_on(glc, ctx, cuda):
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
