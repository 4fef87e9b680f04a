"""The container's byte-plane shuffle filter on the MI355X (-m gpu): filter off is version 1 byte for byte; filter on is
byte-identical to the Python model of version 2 (tests/container_model.py) through the device, host-pointer and file
entry points, with pipelining on and off, and from plain C; decoding by plans of other shapes and settings, of the golden
fixture and of version-1 containers; refusals with their glcContainerLastError triples; the effect on float32 data; the
plan's timing and profile interfaces with the filter on."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import container_model as M
import datagen
import typed_datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-lossless-compression_amd")
ILLEGAL, UNKNOWN = 2, 9999
KIND_OF = {2: "quant16", 4: "smooth32", 8: "smooth64"}


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


def _typed(elem, n, seed):
    """typed data of the element size, with a stretch of text in the middle so that every record kind and sorter tier occurs"""
    if n == 0:
        return np.zeros(0, np.uint8)
    x = typed_datagen.typed_bytes(KIND_OF[elem] if seed % 3 else "float32", n, seed=seed)
    if n > 3000:
        x[n // 3:n // 3 + n // 5] = datagen.text_bytes(n // 5, seed=seed)
    return x


def _lengths(n, rows, elem):
    """nothing; less than an element; several frames, a last frame with fewer blocks and a ragged tail with len % elem != 0"""
    tail = 777 if n > 777 else 77
    assert tail % elem != 0
    return [0, elem - 1, (2 * rows + (1 if rows > 1 else 0)) * n + tail, rows * n]


# --- 1. filter off ---------------------------------------------------------------------------------------------------------
def test_filter_off_or_reset_is_version_1(glc, ctx, cuda):
    n, rows = 4096, 3
    x = _typed(4, 7 * n + 777, 1)
    want = M.write(x, n, rows)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        assert glc.container_get_shuffle(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
        glc.container_set_shuffle(plan, 4)
        assert glc.container_get_shuffle(plan) == 4
        c = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c != want and c == M.write(x, n, rows, 4)
        for bad in (3, 5, 16, 64):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_shuffle(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_shuffle(plan) == 4     # unchanged
        for off in (0, 1):
            glc.container_set_shuffle(plan, 8)
            glc.container_set_shuffle(plan, off)
            assert glc.container_get_shuffle(plan) == 0
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
            assert glc.container_compress_host(plan, x).tobytes() == want


# --- 2. filter on: byte-identical to the model, and read back ------------------------------------------------------------
CASES = [(1000, 1, 8), (1000, 3, 2), (1000, 4, 4), (4096, 1, 2), (4096, 3, 4), (4096, 4, 4), (4096, 8, 8), (65536, 3, 2),
         (65536, 4, 4), (65536, 8, 8), (65536, 8, 4), (1 << 20, 1, 8), (1 << 20, 4, 4), (1 << 20, 3, 2)]


@pytest.mark.parametrize("n,rows,elem", CASES)
@pytest.mark.parametrize("pipelined", [False, True])
def test_device_container_equals_the_model(glc, ctx, cuda, n, rows, elem, pipelined):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        plan.set_pipelining(pipelined)
        glc.container_set_shuffle(plan, elem)
        for i, L in enumerate(_lengths(n, rows, elem)):
            x = _typed(elem, L, 10 * rows + i + 1)
            c = glc.container_compress(plan, _gpu(x))
            want = M.write(x, n, rows, elem)
            assert _host(c).tobytes() == want, (n, rows, elem, L)
            assert c.numel() <= glc.container_bound(L, n)
            back = glc.container_decompress(plan, c)
            assert np.array_equal(_host(back), x), (n, rows, elem, L)
            assert glc.container_last_error(plan) == (0, -1, -1)


@pytest.mark.parametrize("n,rows,elem", [(1000, 3, 2), (4096, 4, 4), (65536, 8, 8), (65536, 3, 4)])
@pytest.mark.parametrize("pipelined", [False, True])
def test_host_and_file_forms_equal_the_model(glc, ctx, cuda, tmp_path, n, rows, elem, pipelined):
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        plan.set_pipelining(pipelined)
        glc.container_set_shuffle(plan, elem)
        for i, L in enumerate(_lengths(n, rows, elem)):
            x = _typed(elem, L, 50 + i)
            want = M.write(x, n, rows, elem)
            c = glc.container_compress_host(plan, x)
            assert c.tobytes() == want, (n, rows, elem, L)
            assert np.array_equal(glc.container_decompress_host(plan, c), x)
            src, dst, back = tmp_path / "in.bin", tmp_path / "out.glcb", tmp_path / "back.bin"
            x.tofile(src)
            glc.container_compress_file(plan, str(src), str(dst))
            assert dst.read_bytes() == want, (n, rows, elem, L)
            glc.container_decompress_file(plan, str(dst), str(back))
            assert back.read_bytes() == x.tobytes()


# --- 3. decoding ---------------------------------------------------------------------------------------------------------
def test_other_plans_decode_and_the_decoder_ignores_its_own_setting(glc, ctx, cuda):
    n, rows, elem = 8192, 8, 4
    x = _typed(elem, 19 * n + 1235, 7)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as w:
        glc.container_set_shuffle(w, elem)
        c = glc.container_compress(w, _gpu(x))
        v1 = M.write(x, n, rows)
        assert np.array_equal(_host(glc.container_decompress(w, _gpu(np.frombuffer(v1, np.uint8)))), x)   # version 1, filter on
    assert np.array_equal(M.read(_host(c).tobytes()), x)
    for m, r, own, pipe in ((n, 3, 0, False), (n, 1, 2, True), (3 * n + 5, 2, 8, False), (1 << 20, 2, 4, True)):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, m, rows=r) as p:
            p.set_pipelining(pipe)
            glc.container_set_shuffle(p, own)
            assert np.array_equal(_host(glc.container_decompress(p, c)), x), (m, r, own)
            assert np.array_equal(glc.container_decompress_host(p, _host(c)), x), (m, r, own)
            assert glc.container_get_shuffle(p) == own
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n - 1, rows=8) as small:
        with pytest.raises(glc.CudppError) as e:
            glc.container_decompress(small, c)
        assert e.value.code == ILLEGAL


def test_gpu_reads_the_golden_fixture_and_writes_it(glc, ctx, cuda):
    gold = open(os.path.join(ROOT, "tests", "golden", "container_v2_f32.bin"), "rb").read()
    x = M.read(gold)
    for n, rows in ((4096, 4), (4096, 1), (70000, 2)):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(gold, np.uint8)))), x)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 4096, rows=4) as plan:
        glc.container_set_shuffle(plan, 4)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == gold


# --- 4. refusals ---------------------------------------------------------------------------------------------------------
def _with_header(c, version, elem):
    h = c[:4] + struct.pack("<HHII", version, 0, struct.unpack("<I", c[8:12])[0], elem) + c[16:24]
    return h + struct.pack("<II", zlib.crc32(h), 0) + c[32:]


def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_corrupted_version_2_containers_are_refused(glc, ctx, cuda):
    import torch
    n, rows, elem = 4096, 2, 4
    x = _typed(elem, 5 * n + 123, 4)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        glc.container_set_shuffle(plan, elem)
        c = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c == M.write(x, n, rows, elem)
        v1 = M.write(x, n, rows)
        lay = M.layout(c)
        s, e, _ = lay["frames"][1]["records"][1]
        flipped = bytearray(c)
        flipped[(s + e) // 2] ^= 0x20
        cases = [(_with_header(c, 2, 3), (1, -1, -1)), (_with_header(c, 2, 16), (1, -1, -1)), (_with_header(c, 2, 0), (1, -1, -1)),
                 (_with_header(v1, 1, 4), (1, -1, -1)),                # version 1 with the word set
                 (_with_header(c, 2, 2), (4, -1, -1)),                 # a legal but wrong elem: only crc_all sees it
                 (bytes(flipped), (3, 1, 1))]
        guard = 64
        for cont, want in cases:
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as err:
                _decompress_into(glc, plan, cont, out, x.size)
            assert err.value.code == UNKNOWN
            assert glc.container_last_error(plan) == want
            with pytest.raises(M.ContainerError) as merr:          # the model agrees
                M.read(cont)
            assert (merr.value.what, merr.value.frame, merr.value.block) == want
            assert bool((out[x.size:] == 0xAB).all())
            with pytest.raises(glc.CudppError):
                glc.container_decompress_host(plan, np.frombuffer(cont, np.uint8), cap=x.size)
            assert glc.container_last_error(plan) == want
        for cut in (len(c) - 1, lay["frames"][1]["start"] + 40):
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError):
                _decompress_into(glc, plan, c[:cut], out, x.size)
            assert glc.container_last_error(plan)[0] == 5
            assert bool((out[x.size:] == 0xAB).all())
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_filter_on(glc, ctx, cuda):
    import torch
    n, rows, elem = 70000, 2, 8
    x = _typed(elem, 2 * n + 999, 9)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        glc.container_set_shuffle(plan, elem)
        need = len(M.write(x, n, rows, elem))
        for cap in (need - 1, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all())
        c = glc.container_compress(plan, _gpu(x), cap=need)
        out = torch.full((x.size + 64,), 0xAB, dtype=torch.uint8, device=cuda)
        with pytest.raises(glc.CudppError) as e:
            _decompress_into(glc, plan, _host(c).tobytes(), out, x.size - 1)
        assert e.value.code == ILLEGAL and bool((out == 0xAB).all())


# --- 5. what the filter is for ---------------------------------------------------------------------------------------------
def test_float32_is_smaller_with_the_filter(glc, ctx, cuda):
    import torch
    n, rows, L = 1 << 20, 8, 8 << 20
    x = datagen.float_philox_bytes(0, L)
    d = _gpu(x)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        plan.set_pipelining(True)
        off = glc.container_compress(plan, d).numel()
        glc.container_set_shuffle(plan, 4)
        c = glc.container_compress(plan, d)
        print("8 MiB float32 ~ N(0,1), n = 1 MiB, rows 8: filter off %d bytes (ratio %.3f), elem 4 %d bytes (ratio %.3f)"
              % (off, L / off, c.numel(), L / c.numel()))
        assert c.numel() < off
        assert torch.equal(glc.container_decompress(plan, c), d)


def test_decoder_staging_grows_and_is_kept(glc, ctx, cuda):
    """a one-row plan decodes a stream of one-block frames, then one of three-block frames (its staging, and the order-0
    codec's scratch, grow), then the first again (they stay)"""
    n, elem = 4096, 4
    x = _typed(elem, 3 * n + 5, 11)
    conts = {}
    for rows, codec in ((1, glc.CONTAINER_CODEC_BWT), (3, glc.CONTAINER_CODEC_HUFF0)):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as w:
            glc.container_set_shuffle(w, elem)
            glc.container_set_codec(w, codec)
            conts[rows] = glc.container_compress(w, _gpu(x))
            assert glc.container_last_error(w) == (0, -1, -1)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=1) as r:
        for rows in (1, 3, 1):
            assert np.array_equal(_host(glc.container_decompress(r, conts[rows])), x), rows
            assert glc.container_last_error(r) == (0, -1, -1)
            assert glc.CONTAINER_WHAT[glc.container_last_error(r)[0]] == "ok"


# --- 6. timing and profile interfaces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_timing_and_kernel_profile_with_the_filter_on(glc, ctx, cuda, pipelined):
    n, rows, elem = 65536, 4, 4
    x = _typed(elem, 9 * n + 777, 3)
    want = M.write(x, n, rows, elem)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        plan.set_pipelining(pipelined)
        glc.container_set_shuffle(plan, elem)
        for mode in (1, 3):
            plan.enable_timing(mode)
            c = glc.container_compress(plan, _gpu(x))
            plan.synchronize()
            assert _host(c).tobytes() == want
            ms = plan.last_timing()
            assert len(ms) == 4 and all(np.isfinite(v) and v >= 0 for v in ms) and sum(ms) > 0
            if mode == 3:
                prof = plan.kernel_profiles()
                assert prof and all(v["launches"] > 0 and v["ms"] >= 0 for v in prof.values())
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            plan.synchronize()
            if mode == 3:
                assert plan.kernel_profile()["launches"] > 0
        plan.enable_timing(0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want


# --- 7. plain C ------------------------------------------------------------------------------------------------------------
def test_plain_c_caller_of_the_filter(glc, tmp_path):
    glc.lib()
    exe = str(tmp_path / "container_filter_rig")
    cmd = ["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "c_caller", "container_filter_rig.c"), "-o", exe, "-L", PKG, "-lglc_amd", "-L", "/opt/rocm/lib",
           "-lamdhip64", "-lm", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the rig reads its input from a file written here (its own sinf and float accumulation are not reproduced bit for bit in
    # numpy), so that the model's containers of the same bytes can be held beside the rig's
    x, want_off, want_on = _rig_input_and_containers()
    src = tmp_path / "filter_rig_input.bin"
    x.tofile(src)
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120)
    # first the line the rig prints BEFORE it decodes, whatever became of the decode: both containers against the model's
    lines = r.stdout.splitlines()
    assert lines and lines[0].startswith("input_crc="), "the rig got no container to report: rc %d\n%s" % (r.returncode, r.stdout + r.stderr)
    pre = dict(kv.split("=") for kv in lines[0].split())
    model = dict(input_crc="%08x" % zlib.crc32(x.tobytes()), off_len=str(len(want_off)), off_crc="%08x" % zlib.crc32(want_off),
                 on_len=str(len(want_on)), on_crc="%08x" % zlib.crc32(want_on))
    assert pre == model, "the ENCODER wrote other bytes than the model (rig rc %d)\nrig:   %r\nmodel: %r\n%s" % (r.returncode, pre, model, r.stderr)
    assert r.returncode == 0, "both containers equal the model's byte for byte, so the DECODER failed on right bytes\n" + r.stdout + r.stderr
    out = dict(kv.split("=") for kv in r.stdout.split())
    assert (out["version"], out["elem"], out["equal"], out["planes"], out["unshuffled"]) == ("2", "4", "1", "1", "1")
    assert int(out["decoded_len"]) == 4 * (9 * 65536 // 4 + 300) + 3
    assert int(out["on_len"]) < int(out["off_len"])             # smooth float32: the high planes code well


def _rig_input_and_containers():
    """float32 samples of a smooth signal -- a sine plus a small random walk, as the rig makes for itself without an argument --
    and a ragged tail of three bytes; the model's containers of them with the filter off and with element size 4 (n 65536, rows 4)"""
    n, count = 65536, 9 * 65536 // 4 + 300
    rng = np.random.default_rng(11)
    walk = np.cumsum(rng.integers(-100, 101, count).astype(np.float32) * np.float32(1e-4), dtype=np.float32)
    v = (np.float32(100.0) * np.sin(np.arange(count, dtype=np.float32) * np.float32(0.00125)) + walk).astype(np.float32)
    x = np.concatenate([v.view(np.uint8), np.array([1, 2, 3], np.uint8)])
    return x, M.write(x, n, 4), M.write(x, n, 4, 4)
