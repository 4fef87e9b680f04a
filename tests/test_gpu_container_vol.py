"""The volume setting of the container on the MI355X (-m gpu): with it on, the device, host-pointer and file entry points,
pipelined and not, write the bytes of the Python model of format version 17 (tests/vol_model.py) and read them back; the golden
fixture decodes; width, plane and fold come from the stream header; every refusal case comes back with the model's class and frame,
and a grid plan, a lag plan and a default plan refuse version 17; with the setting off the bytes are a grid plan's version-12
stream; the setter's state table; the index reports the plane and range reads that start inside a slab, on a slab boundary and in
the last ragged frame give the input's slices."""
import os
import struct
import sys

import numpy as np
import pytest

import container_model as M
import grid_model as G
import vol_inputs as VI
import vol_model as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vol_v17_container.bin")
ILLEGAL, UNKNOWN = 2, 9999

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_grid_v12_gold as gold12  # noqa: E402
import make_vol_v17_gold as gold  # noqa: E402

N, ROWS = gold.BLOCK, gold.ROWS                                   # 8192, 3: a frame is 24576 bytes
FIELD = ("smooth32", 4, 20, 143, 0)                               # a float32 field: slabs of 4096 elements, 1.5 a frame; two frames


def _cases():
    """(name, input, elem, width, plane, fold): the fixture's input (two frames of two slabs and a ragged third) and the field"""
    kind, e, w, s, fold = FIELD
    return [("fixture", gold.gold_input(), gold.ELEM, gold.WIDTH, gold.PLANE, gold.FOLD), ("field", VI.vol_bytes(kind, 2 * N * ROWS, w, s), e, w, s, fold)]


@pytest.fixture(scope="module")
def cases():
    return [c + (V.write(c[1], N, ROWS, *c[2:]),) for c in _cases()]


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


def _plan(glc, ctx, elem=2, width=0, plane=0, fold=0, n=N, rows=ROWS, pipelined=False, lag=(1, 0)):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_delta(plan, 1)
    glc.container_set_delta_lag(plan, *lag)
    glc.container_set_delta_grid(plan, width, fold)
    glc.container_set_delta_volume(plan, plane)
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


# --- 1. the model's bytes from all six entry points, and read back -------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_gpu_container_equals_the_models(glc, ctx, cuda, tmp_path, cases, which):
    name, x, elem, width, plane, fold, want = cases[which]
    assert struct.unpack("<HHII", want[4:16]) == (17, 13 | fold << 1, N, elem | width << 8) and struct.unpack("<I", want[28:32]) == (plane,)
    assert len(M.layout(want)["frames"]) == (3 if name == "fixture" else 2)
    for pipelined in (False, True):
        with _plan(glc, ctx, elem, width, plane, fold, pipelined=pipelined) as plan:
            assert glc.container_get_delta_grid(plan) == (width, fold) and glc.container_get_delta_volume(plan) == plane
            c = glc.container_compress(plan, _gpu(x))
            assert _host(c).tobytes() == want
            assert glc.container_compress_host(plan, x).tobytes() == want
            src, dst = tmp_path / "in.bin", tmp_path / "out.glcb"
            x.tofile(src)
            glc.container_compress_file(plan, str(src), str(dst))
            assert dst.read_bytes() == want
            _decodes_everywhere(glc, plan, want, x, tmp_path)
            for n in (0, 1, elem * plane - 1, N + 9):
                y = x[:n]
                c = glc.container_compress(plan, _gpu(y))
                assert _host(c).tobytes() == V.write(y, N, ROWS, elem, width, plane, fold)
                assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


def test_the_fixture_decodes_and_its_settings_come_from_the_stream_header(glc, ctx, cuda, tmp_path, cases):
    """the golden fixture (elem 2, width 20, plane 300, fold 1) and the field's container, read by plans whose own setting says
    something else; a volume plan also reads version 12"""
    g = open(GOLD, "rb").read()
    x = gold.gold_input()
    assert g == cases[0][6]
    y, c = cases[1][1], cases[1][6]
    c12, x12 = gold12.make(), gold12.gold_input()
    for elem, width, plane, fold, n, rows in ((2, 20, 300, 1, N, ROWS), (8, 65536, 1 << 24, 0, N, 1), (4, 7, 8, 1, 70000, 2)):
        with _plan(glc, ctx, elem, width, plane, fold, n=n, rows=rows) as plan:
            _decodes_everywhere(glc, plan, g, x, tmp_path)
            _decodes_everywhere(glc, plan, c, y, tmp_path)
            _decodes_everywhere(glc, plan, c12, x12, tmp_path)


# --- 2. refusals -----------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_refusals_of_version_17(glc, ctx, cuda, tmp_path):
    import torch
    c17 = open(GOLD, "rb").read()
    x = gold.gold_input()
    cases, _ = V.refusal_cases(c17, gold12.make())
    assert len(cases) >= 25
    guard = 64
    path = tmp_path / "bad.glcb"
    with _plan(glc, ctx, 2, 20, 300, 1) as on_plan, _plan(glc, ctx, 2, 20, 0, 1) as grid_plan, _plan(glc, ctx, 2, lag=(3, 1)) as lag_plan, \
            _plan(glc, ctx, 2) as auto_plan, glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plain_plan:
        assert glc.container_get_delta_volume(grid_plan) == 0 and glc.container_get_delta_grid(grid_plan) == (20, 1)
        assert glc.container_get_delta_volume(lag_plan) == 0 and glc.container_get_delta_lag(lag_plan) == (3, 1)
        for name, cont, want, reads in cases:
            plan = on_plan if "vol" in reads else grid_plan if "grid" in reads else lag_plan if "lag" in reads else \
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
        assert np.array_equal(_host(glc.container_decompress(on_plan, _gpu(np.frombuffer(c17, np.uint8)))), x)
        assert glc.container_last_error(on_plan) == (0, -1, -1)


# --- 3. byte-for-byte compatibility ---------------------------------------------------------------------------------------------
def test_with_the_setting_off_the_bytes_are_a_grid_plans(glc, ctx, cuda, cases):
    _, x, elem, width, plane, fold, want17 = cases[0]
    want12 = G.write(x, N, ROWS, elem, width, fold)
    assert struct.unpack("<HH", want12[4:8]) == (12, 5 | fold << 1) and struct.unpack("<I", want12[28:32]) == (0,)
    with _plan(glc, ctx, elem, width, 0, fold) as never:
        c_never = _host(glc.container_compress(never, _gpu(x))).tobytes()
    with _plan(glc, ctx, elem, width, plane, fold) as plan:
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want17
        glc.container_set_delta_volume(plan, 0)                    # on, then off again
        assert glc.container_get_delta_volume(plan) == 0 and glc.container_get_delta_grid(plan) == (width, fold)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == c_never == want12
        with pytest.raises(glc.CudppError):                        # and it no longer speaks version 17
            glc.container_decompress(plan, _gpu(np.frombuffer(want17, np.uint8)))
        assert glc.container_last_error(plan) == (1, -1, -1)


# --- 4. the setter ---------------------------------------------------------------------------------------------------------------
def test_the_setter(glc, ctx, cuda):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        def refused(call, *a):
            with pytest.raises(glc.CudppError) as e:
                call(plan, *a)
            return e.value.code == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION

        get = lambda: glc.container_get_delta_volume(plan)
        grid = lambda: glc.container_get_delta_grid(plan)

        def ready(width=20):
            glc.container_set_codec(plan, 1)
            glc.container_set_auto(plan, 1)
            glc.container_set_shuffle(plan, 4)
            glc.container_set_delta(plan, 1)
            glc.container_set_delta_grid(plan, width, 1)

        on = lambda: glc.container_set_delta_volume(plan, 300)

        assert get() == 0
        glc.container_set_delta_volume(plan, 0)                                     # off is always legal
        assert refused(glc.container_set_delta_volume, 300) and get() == 0          # a default plan: no grid
        ready(0)
        assert refused(glc.container_set_delta_volume, 300) and get() == 0          # every prerequisite of the grid, but the grid off
        ready()
        for p in (20, 19, 1, (1 << 24) + 1, 1 << 31):
            assert refused(glc.container_set_delta_volume, p) and get() == 0        # not above the width; above 2^24
        for p in (21, 1 << 24, 300):
            glc.container_set_delta_volume(plan, p)
            assert get() == p and grid() == (20, 1)
        for p in (20, (1 << 24) + 1):
            assert refused(glc.container_set_delta_volume, p) and get() == 300      # unchanged
        # while it is on: a grid width at or above the plane is refused, one below it is taken
        for w in (300, 301, 65536):
            assert refused(glc.container_set_delta_grid, w, 1) and grid() == (20, 1) and get() == 300
        glc.container_set_delta_grid(plan, 299, 0)
        assert grid() == (299, 0) and get() == 300
        glc.container_set_delta_grid(plan, 20, 1)
        assert refused(glc.container_set_delta_lag, 3, 1) and get() == 300
        for elem in (2, 8, 4):
            glc.container_set_shuffle(plan, elem)                                   # a change among 2, 4 and 8 keeps it
            assert get() == 300 and grid() == (20, 1)
        # whatever switches the grid off switches this off, and it stays off
        glc.container_set_delta_grid(plan, 0, 0)
        assert get() == 0 and grid() == (0, 0)
        glc.container_set_delta_grid(plan, 20, 1)
        assert get() == 0
        on(); glc.container_set_delta(plan, 0)
        assert get() == 0 and grid() == (0, 0)
        ready(); on(); glc.container_set_shuffle(plan, 0)
        assert get() == 0
        ready(); on(); glc.container_set_auto(plan, 0)
        assert get() == 0
        ready(); on(); glc.container_set_codec(plan, 0)
        assert get() == 0
        ready(); on(); glc.container_set_codec(plan, 1)                             # the same codec again: no change
        assert get() == 300 and grid() == (20, 1)
        glc.container_set_delta_volume(plan, 0)
        assert get() == 0 and grid() == (20, 1)                                     # off leaves the grid as it is


# --- 5. index and range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_index_and_range_reads(glc, ctx, cuda, tmp_path, cases, which):
    name, x, elem, width, plane, fold, want = cases[which]
    Fr, Qb = N * ROWS, V.slab(width, plane) * elem                 # a frame's bytes, a slab's (12288: half a frame; 16384: two thirds)
    assert Qb < Fr
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    d = _gpu(np.frombuffer(want, np.uint8))
    ranges = [(Qb + plane * elem + 5, 9), (Qb + 3 * plane * elem - 1, 2 * plane * elem), (5000, 100), (Fr + Qb + 777, 31),        # inside a slab
              (Qb, 1), (Qb, elem), (Qb - 1, 2), (Qb - 5, 10), (Fr + Qb, 64), (Fr + Qb - 3, 7),                                    # on a slab boundary
              (Fr - 10, 20), (Fr - 3000, 6000), (N - 5, 10), (x.size - 3, 3), (x.size - 1000, 1000), (0, x.size), (x.size, 0), (1, 1)]
    if name == "fixture":                                           # the last, ragged frame: 1235 bytes of one block
        ranges += [(2 * Fr, 1235), (2 * Fr + 1, 100), (2 * Fr + 1230, 5), (2 * Fr - 7, 20), (2 * Fr + 600, 635)]
    with _plan(glc, ctx, 8, 7, 9, fold ^ 1) as plan:               # (the plan's own width, plane and fold are not the stream's)
        with glc.container_index(plan, d) as ix:
            assert ix.info() == (x.size, N, len(M.layout(want)["frames"]), 17, 13 | fold << 1, elem | width << 8)
            assert ix.plane() == plane
            for off, cnt in ranges:
                got = _host(glc.container_read_range(plan, ix, d, off, cnt))
                assert np.array_equal(got, x[off:off + cnt]), (off, cnt)
        with glc.container_index_host(plan, np.frombuffer(want, np.uint8)) as ix:
            assert ix.info()[3:] == (17, 13 | fold << 1, elem | width << 8) and ix.plane() == plane
            for off, cnt in ranges[:10]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(want, np.uint8), off, cnt), x[off:off + cnt])
        with glc.container_index_file(plan, str(path)) as ix:
            assert ix.plane() == plane
            for off, cnt in (ranges[0], ranges[7], ranges[11]):
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
            glc.container_set_delta_volume(plan, 0)                # the index outlives the setting; the plan no longer speaks the version
            with pytest.raises(glc.CudppError):
                glc.container_read_range_file(plan, ix, str(path), 10, 10)
            assert glc.container_last_error(plan) == (1, -1, -1)
        c12 = gold12.make()
        with _plan(glc, ctx, 2, 20, 300, 1) as vplan, glc.container_index_host(vplan, np.frombuffer(c12, np.uint8)) as ix:
            assert ix.plane() == 0 and ix.info()[3] == 12           # a version-12 stream has no plane
