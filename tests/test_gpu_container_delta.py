"""The delta mode of the container's filter on the MI355X (-m gpu): delta on is byte-identical to the Python model of format
version 4 (tests/container_model.py) for every element size, both codecs and pipelining on and off, through the device,
host-pointer and file entry points, and from plain C; the golden fixture decodes; a plan's own delta setting does not matter to
its decoder; the setters' rules; refusals with their glcContainerLastError triples; capacity."""
import os
import struct
import subprocess

import numpy as np
import pytest

import container_model as M
import series_datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-lossless-compression_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL, UNKNOWN = 2, 9999
N = 8192
SERIES = {2: "adc16", 4: "ctr32", 8: "ts64"}


def _rows(elem):
    return 8 if elem == 8 else 4


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


_INPUT, _WANT = {}, {}


def _input(elem):
    """two full frames, two whole blocks and 1235 bytes of the element size's series; the second frame is noise (raw records)"""
    if elem not in _INPUT:
        L = (2 * _rows(elem) + 2) * N + 1235
        x = series_datagen.series_bytes(SERIES[elem], L + 8)[:L].copy()
        r = _rows(elem)
        x[r * N:2 * r * N] = np.random.default_rng(elem).integers(0, 256, r * N, dtype=np.uint8)
        x.setflags(write=False)
        _INPUT[elem] = x
    return _INPUT[elem]


def _want(elem, codec):
    if (elem, codec) not in _WANT:
        _WANT[elem, codec] = M.write(_input(elem), N, _rows(elem), elem, codec, delta=True)
    return _WANT[elem, codec]


def _plan(glc, ctx, elem, codec, pipelined=False, delta=True, n=N, rows=None):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows or _rows(max(elem, 2)))
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if delta:
        glc.container_set_delta(plan, 1)
    return plan


# --- 1. delta on: byte-identical to the model, and read back ---------------------------------------------------------------
@pytest.mark.parametrize("elem", [2, 4, 8])
@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("pipelined", [False, True])
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, elem, codec, pipelined):
    x, want = _input(elem), _want(elem, codec)
    assert struct.unpack("<I", want[4:8])[0] == 0x00010004 and struct.unpack("<II", want[8:16]) == (N, elem)
    frames = M.layout(want)["frames"]
    assert [f["nb"] for f in frames] == [_rows(elem), _rows(elem), 2, 1]
    assert {k for f in frames for _, _, k in f["records"]} == {M.RAW, M.HUFF0 if codec else M.HUFF}
    with _plan(glc, ctx, elem, codec, pipelined) as plan:
        assert glc.container_get_delta(plan) == 1
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
        for L in (0, elem - 1):                                 # nothing; less than an element
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == M.write(y, N, _rows(elem), elem, codec, delta=True)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


# --- 2. decoding -----------------------------------------------------------------------------------------------------------
def test_gpu_reads_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "container_v4_series.bin"), "rb").read()
    x, kinds = M.read(gold, with_kinds=True)
    assert {0, 1, 2} <= set(kinds)
    g = np.frombuffer(gold, np.uint8)
    for n, rows, elem, codec, delta in ((4096, 8, 8, 1, True), (4096, 1, 0, 0, False), (70000, 2, 4, 1, True)):
        with _plan(glc, ctx, elem, codec, delta=delta, n=n, rows=rows) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert np.array_equal(glc.container_decompress_host(plan, g), x)


def test_the_decoder_ignores_its_plans_delta_setting(glc, ctx, cuda):
    elem = 4
    x, v4 = _input(elem), _want(elem, 1)
    older = [M.write(x, N, 4), M.write(x, N, 4, elem), M.write(x, N, 4, elem, 1), M.write(x, N, 4, 0, 1)]
    with _plan(glc, ctx, 0, 0, delta=False) as off:            # delta (and shuffle) off: decodes version 4
        assert glc.container_get_delta(off) == 0
        assert np.array_equal(_host(glc.container_decompress(off, _gpu(np.frombuffer(v4, np.uint8)))), x)
        assert np.array_equal(glc.container_decompress_host(off, np.frombuffer(v4, np.uint8)), x)
    with _plan(glc, ctx, 8, 1, pipelined=True, n=3 * N + 5, rows=2) as on:        # delta on, another shape: versions 1 to 4
        for c in older + [v4, _want(2, 0)]:
            y = _input(2) if c is _want(2, 0) else x
            assert np.array_equal(_host(glc.container_decompress(on, _gpu(np.frombuffer(c, np.uint8)))), y)
        assert glc.container_get_delta(on) == 1 and glc.container_get_shuffle(on) == 8


# --- 3. the setters ------------------------------------------------------------------------------------------------------
def test_setters_and_what_a_cleared_shuffle_writes(glc, ctx, cuda):
    elem = 4
    x = _input(elem)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=4) as plan:
        assert glc.container_get_delta(plan) == 0
        with pytest.raises(glc.CudppError) as e:                # the shuffle is off
            glc.container_set_delta(plan, 1)
        assert e.value.code == ILLEGAL and glc.container_get_delta(plan) == 0
        glc.container_set_delta(plan, 0)                        # off is always legal
        glc.container_set_shuffle(plan, elem)
        for bad in (2, 3, 255, 1 << 31):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_delta(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_delta(plan) == 0
        glc.container_set_delta(plan, 1)
        for bad in (2, 1 << 31):
            with pytest.raises(glc.CudppError):
                glc.container_set_delta(plan, bad)
            assert glc.container_get_delta(plan) == 1           # unchanged
        for other in (2, 8, elem):                              # switching among 2, 4 and 8 keeps it
            glc.container_set_shuffle(plan, other)
            assert glc.container_get_delta(plan) == 1
        with pytest.raises(glc.CudppError):                     # a refused shuffle setting changes nothing
            glc.container_set_shuffle(plan, 3)
        assert glc.container_get_delta(plan) == 1 and glc.container_get_shuffle(plan) == elem
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _want(elem, 0)
        glc.container_set_delta(plan, 0)                        # delta off: version 2 byte for byte
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, N, 4, elem)
        for codec, clear in ((0, 0), (1, 1)):                   # delta set, then the shuffle cleared: version 1 or 3
            glc.container_set_codec(plan, codec)
            glc.container_set_shuffle(plan, elem)
            glc.container_set_delta(plan, 1)
            glc.container_set_shuffle(plan, clear)
            assert glc.container_get_delta(plan) == 0 and glc.container_get_shuffle(plan) == 0
            c = _host(glc.container_compress(plan, _gpu(x))).tobytes()
            assert c == M.write(x, N, 4, 0, codec) and struct.unpack("<HH", c[4:8]) == (3 if codec else 1, 0)
            glc.container_set_shuffle(plan, elem)               # ... and the shuffle back on does not bring it back
            assert glc.container_get_delta(plan) == 0
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, N, 4, elem, codec)


# --- 4. refusals ---------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


@pytest.mark.parametrize("codec", [0, 1])
def test_refusal_matrix_of_version_4(glc, ctx, cuda, codec):
    import torch
    elem = 4
    x = _input(elem)
    with _plan(glc, ctx, elem, codec) as plan:
        c4 = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c4 == _want(elem, codec)
        glc.container_set_delta(plan, 0)
        glc.container_set_codec(plan, 1)
        c3 = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c3 == M.write(x, N, 4, elem, 1)
        cases, lay = M.refusal_cases(c4, c3, elem)
        assert len(cases) >= 17 and (M.with_header(c4, 4, 0, elem), (1, -1, -1)) in cases
        guard = 64
        for cont, want in cases:
            with pytest.raises(M.ContainerError) as merr:          # the model
                M.read(cont)
            assert (merr.value.what, merr.value.frame, merr.value.block) == want
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN
            assert glc.container_last_error(plan) == want
            assert bool((out[x.size:] == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want
        for cut in (len(c4) - 1, lay["frames"][1]["start"] + 40):
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError):
                _decompress_into(glc, plan, c4[:cut], out, x.size)
            assert glc.container_last_error(plan)[0] == 5
            assert bool((out[x.size:] == 0xAB).all())
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c4, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


@pytest.mark.parametrize("codec", [0, 1])
def test_capacity_with_the_delta_on(glc, ctx, cuda, codec):
    import torch
    elem = 8
    x, need = _input(elem), len(_want(elem, codec))
    with _plan(glc, ctx, elem, codec) as plan:
        for cap in (need - 1, need // 2, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need
        out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
        with pytest.raises(glc.CudppError) as e:
            _decompress_into(glc, plan, _host(c).tobytes(), out, x.size - 1)
        assert e.value.code == ILLEGAL and bool((out == 0xAB).all())


# --- 5. plain C ------------------------------------------------------------------------------------------------------------
def test_plain_c_caller_of_the_delta_mode(glc, tmp_path):
    glc.lib()
    exe = str(tmp_path / "container_delta_rig")
    cmd = ["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "c_caller", "container_delta_rig.c"), "-o", exe, "-L", PKG, "-lglc_amd", "-L", "/opt/rocm/lib",
           "-lamdhip64", "-lm", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(kv.split("=") for kv in r.stdout.split())
    assert (out["version"], out["flags"], out["elem"], out["delta_on"], out["cleared"], out["refused"]) == ("4", "1", "8", "1", "0", "1")
    assert (out["equal"], out["planes"], out["restored"]) == ("1", "1", "1")
    assert int(out["decoded_len"]) == 8 * (9 * 65536 // 8 + 300) + 5
    assert 4 * int(out["on_len"]) < 3 * int(out["off_len"])    # int64 timestamps under the order-0 codec: what the mode is for
