"""The container's order-0 Huffman codec on the MI355X (-m gpu): codec BWT is version 1 / 2 byte for byte; codec HUFF0 is
byte-identical to the Python model of version 3 (tests/container_model.py) through the device, host-pointer and file
entry points, with pipelining on and off, and from plain C; decoding by plans of other shapes and settings, of the golden
fixture with all three kinds and of the version-1 / 2 fixtures; refusals with their glcContainerLastError triples; capacity;
the plan's timing and profile interfaces with the codec on."""
import os
import struct
import subprocess

import numpy as np
import pytest

import container_model as M
import datagen
import typed_datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-lossless-compression_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL, UNKNOWN = 2, 9999
NEW_KERNELS = {"k_hdb_hist", "k_hdb_table", "k_hdb_enc_count", "k_hdb_enc_scan", "k_hdb_enc_pack", "k_hdb_span_functions", "k_hdb_emit"}


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


def _mixed(elem, L, n, seed):
    """Zipf, text, typed and uniform stretches.  Without the filter: Zipf bytes with a stretch of uniform bytes that covers whole
    blocks (raw records), one of text and one of 16-bit codes.  With it: elements whose low half is noise and whose high half is
    Zipf bytes -- the shuffled frame's first planes are raw records, its last ones order-0 ones -- with a stretch of text."""
    if L == 0:
        return np.zeros(0, np.uint8)
    rng = np.random.default_rng(seed)
    if elem == 0:
        x = datagen.zipf_bytes(L, seed=seed).copy()
        a, b = min(L, n), min(L, 2 * n + n // 2)
        x[a:b] = rng.integers(0, 256, b - a, dtype=np.uint8)
        a = min(L, 3 * n)
        t = datagen.text_bytes_fast(min(L - a, n // 2, 50000), seed=seed)
        x[a:a + t.size] = t
        a = min(L, 4 * n + 7)
        q = typed_datagen.typed_bytes("quant16", min(L - a, n // 2, 50000), seed=seed)
        x[a:a + q.size] = q
        return x
    q = L // elem
    if q == 0:
        return rng.integers(0, 256, L, dtype=np.uint8)
    x = np.empty(L, np.uint8)
    e = x[:q * elem].reshape(q, elem)
    e[:, :elem // 2] = rng.integers(0, 256, (q, elem // 2), dtype=np.uint8)
    e[:, elem // 2:] = datagen.zipf_bytes(q * (elem - elem // 2), seed=seed).reshape(q, -1)
    x[q * elem:] = rng.integers(0, 256, L - q * elem, dtype=np.uint8)
    if L > 3000:
        t = datagen.text_bytes_fast(min(L // 7, 30000), seed=seed)
        x[L // 3:L // 3 + t.size] = t
    return x


def _lengths(n, rows, elem):
    """nothing; less than an element; several frames, a last frame with fewer blocks and a ragged tail; exactly one frame"""
    tail = 777 if n > 777 else 77
    assert elem == 0 or tail % elem != 0
    return [0, max(elem, 2) - 1, (2 * rows + (1 if rows > 1 else 2)) * n + tail, rows * n]


def _frames_with_both(c):
    return sum(1 for f in M.layout(c)["frames"] if {k for _, _, k in f["records"]} >= {M.RAW, M.HUFF0})


def _plan(glc, ctx, n, rows, elem=0, codec=1, pipelined=False):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    return plan


# --- 1. codec BWT ----------------------------------------------------------------------------------------------------------
def test_codec_bwt_default_and_after_a_reset_is_version_1_or_2(glc, ctx, cuda):
    n, rows = 4096, 3
    x = _mixed(4, 7 * n + 777, n, 1)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        assert glc.container_get_codec(plan) == glc.CONTAINER_CODEC_BWT
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == M.write(x, n, rows)
        glc.container_set_codec(plan, glc.CONTAINER_CODEC_HUFF0)
        assert glc.container_get_codec(plan) == 1
        c = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c == M.write(x, n, rows, 0, 1) and struct.unpack("<H", c[4:6])[0] == 3
        for bad in (2, 3, 255, 1 << 31):
            with pytest.raises(glc.CudppError) as e:
                glc.container_set_codec(plan, bad)
            assert e.value.code == ILLEGAL and glc.container_get_codec(plan) == 1        # unchanged
        glc.container_set_codec(plan, glc.CONTAINER_CODEC_BWT)
        for elem in (0, 4):
            glc.container_set_shuffle(plan, elem)
            want = M.write(x, n, rows, elem)
            assert struct.unpack("<H", want[4:6])[0] == (2 if elem else 1)
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
            assert glc.container_compress_host(plan, x).tobytes() == want


# --- 2. codec HUFF0: byte-identical to the model, and read back ---------------------------------------------------------------
CASES = [(1000, 1, 0), (1000, 3, 2), (1000, 4, 4), (4096, 1, 2), (4096, 3, 0), (4096, 8, 8), (65536, 3, 0), (65536, 4, 4),
         (65536, 8, 8), (65536, 8, 2), (70000, 3, 4), (70000, 4, 0), (1 << 20, 1, 8), (1 << 20, 4, 4), (1 << 20, 3, 0)]


@pytest.mark.parametrize("n,rows,elem", CASES)
@pytest.mark.parametrize("pipelined", [False, True])
def test_device_container_equals_the_model(glc, ctx, cuda, n, rows, elem, pipelined):
    with _plan(glc, ctx, n, rows, elem, 1, pipelined) as plan:
        for i, L in enumerate(_lengths(n, rows, elem)):
            x = _mixed(elem, L, n, 10 * rows + i + 1)
            c = glc.container_compress(plan, _gpu(x))
            want = M.write(x, n, rows, elem, 1)
            assert _host(c).tobytes() == want, (n, rows, elem, L)
            assert struct.unpack("<HHII", want[4:16]) == (3, 0, n, elem)
            assert c.numel() <= glc.container_bound(L, n)
            back = glc.container_decompress(plan, c)
            assert np.array_equal(_host(back), x), (n, rows, elem, L)
            assert glc.container_last_error(plan) == (0, -1, -1)
            if i == 2 and n >= 65536 and rows >= 3:             # (a block of noise is a raw record from 64 KiB on)
                assert _frames_with_both(want) > 0, (n, rows, elem)


@pytest.mark.parametrize("n,rows,elem", [(1000, 3, 2), (4096, 4, 0), (65536, 8, 8), (65536, 3, 4), (70000, 3, 0)])
@pytest.mark.parametrize("pipelined", [False, True])
def test_host_and_file_forms_equal_the_model(glc, ctx, cuda, tmp_path, n, rows, elem, pipelined):
    with _plan(glc, ctx, n, rows, elem, 1, pipelined) as plan:
        for i, L in enumerate(_lengths(n, rows, elem)):
            x = _mixed(elem, L, n, 50 + i)
            want = M.write(x, n, rows, elem, 1)
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
def test_other_plans_decode_and_the_decoder_ignores_its_own_settings(glc, ctx, cuda):
    n, rows, elem = 65536, 8, 4
    x = _mixed(elem, 19 * n + 1235, n, 7)
    with _plan(glc, ctx, n, rows, elem, 1) as w:
        c = glc.container_compress(w, _gpu(x))
    assert np.array_equal(M.read(_host(c).tobytes()), x)
    assert _frames_with_both(_host(c).tobytes()) > 0
    for m, r, own_codec, own_elem, pipe in ((n, 3, 0, 0, False), (n, 1, 1, 2, True), (3 * n + 5, 2, 0, 8, False), (1 << 20, 2, 1, 4, True)):
        with _plan(glc, ctx, m, r, own_elem, own_codec, pipe) as p:
            assert np.array_equal(_host(glc.container_decompress(p, c)), x), (m, r)
            assert np.array_equal(glc.container_decompress_host(p, _host(c)), x), (m, r)
            assert glc.container_get_codec(p) == own_codec and glc.container_get_shuffle(p) == own_elem
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n - 1, rows=8) as small:
        with pytest.raises(glc.CudppError) as e:
            glc.container_decompress(small, c)
        assert e.value.code == ILLEGAL


def test_gpu_reads_the_fixtures_of_all_three_versions(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "container_v3_mixed.bin"), "rb").read()
    x, kinds = M.read(gold, with_kinds=True)
    assert {0, 1, 2} <= set(kinds)
    for n, rows, codec in ((4096, 4, 1), (4096, 1, 0), (70000, 2, 1)):
        with _plan(glc, ctx, n, rows, 0, codec) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(gold, np.uint8)))), x)
            assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(gold, np.uint8)), x)
            for name in ("container_v1.bin", "container_v2_f32.bin"):    # ... and the older ones on a HUFF0 plan
                old = open(os.path.join(GOLDEN, name), "rb").read()
                assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(old, np.uint8)))), M.read(old))


# --- 4. refusals ---------------------------------------------------------------------------------------------------------
def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


def test_corrupted_version_3_containers_are_refused(glc, ctx, cuda):
    import torch
    n, rows, elem = 4096, 3, 4
    x = _mixed(elem, 7 * n + 123, n, 4)
    with _plan(glc, ctx, n, rows, elem, 1) as plan:
        c = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        assert c == M.write(x, n, rows, elem, 1)
        cases, lay = M.corrupted_cases(c, x, n, rows, elem)
        assert len(cases) >= 12
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
        for cut in (len(c) - 1, lay["frames"][1]["start"] + 40):
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError):
                _decompress_into(glc, plan, c[:cut], out, x.size)
            assert glc.container_last_error(plan)[0] == 5
            assert bool((out[x.size:] == 0xAB).all())
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)
        assert glc.container_last_error(plan) == (0, -1, -1)


def test_capacity_with_the_codec_on(glc, ctx, cuda):
    import torch
    n, rows, elem = 70000, 2, 8
    x = _mixed(elem, 2 * n + 999, n, 9)
    with _plan(glc, ctx, n, rows, elem, 1) as plan:
        need = len(M.write(x, n, rows, elem, 1))
        for cap in (need - 1, need - 20, need // 2, 100):
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


# --- 5. timing and profile interfaces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True])
def test_timing_and_kernel_profile_with_the_codec_on(glc, ctx, cuda, pipelined):
    n, rows, elem = 65536, 4, 4
    x = _mixed(elem, 9 * n + 777, n, 3)
    want = M.write(x, n, rows, elem, 1)
    with _plan(glc, ctx, n, rows, elem, 1, pipelined) as plan:
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
                assert {"k_hdb_hist", "k_hdb_table", "k_hdb_enc_count", "k_hdb_enc_scan", "k_hdb_enc_pack"} <= set(prof)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
            plan.synchronize()
            if mode == 3:
                prof = plan.kernel_profiles()
                assert NEW_KERNELS <= set(prof)
                assert plan.kernel_profile()["launches"] > 0
        plan.enable_timing(0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want


# --- 6. plain C ------------------------------------------------------------------------------------------------------------
def test_plain_c_caller_of_the_codec(glc, tmp_path):
    glc.lib()
    exe = str(tmp_path / "container_codec_rig")
    cmd = ["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "c_caller", "container_codec_rig.c"), "-o", exe, "-L", PKG, "-lglc_amd", "-L", "/opt/rocm/lib",
           "-lamdhip64", "-lm", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(kv.split("=") for kv in r.stdout.split())
    assert (out["default_codec"], out["bwt_version"], out["huff0_version"], out["equal"], out["bad_codec_refused"]) == ("0", "1", "3", "1", "1")
    assert int(out["decoded_len"]) == 9 * 65536 + 1235
    assert int(out["huff0_len"]) < int(out["bwt_len"]) < int(out["decoded_len"])      # skewed i.i.d. bytes: the order-0 codec's case
