"""The BWT container on the MI355X (-m gpu): the CRC kernel against zlib, device containers byte-identical to the Python
model's (tests/container_model.py) and read back, cross reading between plans of other shapes, the model and the golden
fixture, blocks that cannot be encoded stored raw, corrupted containers refused before anything is decoded, capacity, the
host-pointer and file forms, and a plain-C caller."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import container_model as M
import datagen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-lossless-compression_amd")
ILLEGAL, UNKNOWN = 2, 9999


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _kind_data(kind, n, seed):
    if n == 0:
        return np.zeros(0, np.uint8)
    if kind == "zipf":
        return datagen.zipf_bytes(n, seed=seed)
    if kind == "text":
        return datagen.text_bytes(n, seed=seed)
    if kind == "log":
        return datagen.log_bytes(n, seed=seed)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


# --- 1. the CRC kernel --------------------------------------------------------------------------------------------------
def test_crc32_segments_equals_zlib(glc, cuda):
    import torch
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, (1 << 20) + 64, dtype=np.uint8)
    d = _gpu(buf)
    offs, lens = [], []
    for L in (0, 1, 3, 15, 16, 17, 63, 64, 65, 4095, 4096, (1 << 20) - 1, 1 << 20, (1 << 20) + 1):
        for o in (0, 1, 3, 7):
            offs.append(o)
            lens.append(L)
    got = glc.crc32_segments(d, offs, lens)
    assert got == [zlib.crc32(buf[o:o + L].tobytes()) for o, L in zip(offs, lens)]
    one = glc.crc32_segments(d, [3], [(1 << 20) + 1])
    assert one == [zlib.crc32(buf[3:(1 << 20) + 4].tobytes())]
    # 5000 ragged segments in one call, overlapping, any alignment
    o = rng.integers(0, 1 << 19, 5000)
    L = rng.integers(0, 70000, 5000)
    L[::7] = rng.integers(0, 40, L[::7].size)
    got = glc.crc32_segments(d, o, L)
    assert got == [zlib.crc32(buf[a:a + b].tobytes()) for a, b in zip(o, L)]
    # one 64 MiB segment
    big = torch.randint(0, 256, (64 << 20,), dtype=torch.uint8, device=cuda)
    assert glc.crc32_segments(big, [0], [64 << 20]) == [zlib.crc32(_host(big).tobytes())]


# --- 2. round trip, byte-identical to the model -------------------------------------------------------------------------
KINDS = ["zipf", "text", "log", "zeros", "random"]


@pytest.mark.parametrize("n,rows", [(4096, 1), (4096, 4), (70000, 1), (70000, 4), (1 << 20, 1), (1 << 20, 4)])
@pytest.mark.parametrize("pipelined", [False, True])
def test_round_trip_and_byte_identity_with_the_model(glc, ctx, cuda, n, rows, pipelined):
    lengths = [0, 1, 2, 4095, 4096, 4097, n - 1, n, n + 1, 3 * n + 12345]
    if n == 1 << 20:
        lengths = [0, 1, 4097, n - 1, n + 1, 3 * n + 12345]            # (the model's oracle is the slow part)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        plan.set_pipelining(pipelined)
        for i, L in enumerate(lengths):
            kind = KINDS[(i + rows) % len(KINDS)]
            x = _kind_data(kind, L, 100 + i)
            c = glc.container_compress(plan, _gpu(x))
            want = M.write(x, n, rows)
            assert _host(c).tobytes() == want, (kind, L)
            back = glc.container_decompress(plan, c)
            assert np.array_equal(_host(back), x), (kind, L)
            assert glc.container_last_error(plan) == (0, -1, -1)


# --- 3. cross reading ---------------------------------------------------------------------------------------------------
def test_gpu_reads_the_model_and_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(ROOT, "tests", "golden", "container_v1.bin"), "rb").read()
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 4096, rows=1) as plan:
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(gold, np.uint8)))), M.read(gold))
    x = _kind_data("text", 5 * 70000 + 777, 3)
    c = M.write(x, 70000, 3)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 70000, rows=2) as plan:
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)


def test_other_plans_read_a_container_and_the_model_reads_the_gpu(glc, ctx, cuda):
    n = 8192
    x = np.concatenate([_kind_data(k, 4 * n, 7 + i) for i, k in enumerate(["text", "zipf", "random"])] + [_kind_data("log", 999, 1)])
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=8) as w:
        c = glc.container_compress(w, _gpu(x))
    assert np.array_equal(M.read(_host(c).tobytes()), x)
    for m, rows in ((n, 3), (3 * n + 5, 1), (1 << 20, 2)):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, m, rows=rows) as r:
            assert np.array_equal(_host(glc.container_decompress(r, c)), x), (m, rows)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n - 1, rows=8) as small:
        with pytest.raises(glc.CudppError) as e:
            glc.container_decompress(small, c)
        assert e.value.code == ILLEGAL


# --- 4. a block the format cannot hold ----------------------------------------------------------------------------------
def _piece(rng, n):   # tests/test_gpu_fuzz.py's generator, restated
    kind = int(rng.integers(0, 10))
    seed = int(rng.integers(1, 1 << 30))
    if kind == 0:
        return datagen.zipf_bytes(n, seed=seed, s=float(rng.uniform(0.5, 2.0)))
    if kind == 1:
        return datagen.text_bytes(n, seed=seed)
    if kind == 2:
        return datagen.log_bytes(n, seed=seed)
    if kind == 3:
        return datagen.float_bytes(n, seed=seed)
    if kind == 4:
        return np.full(n, int(rng.integers(0, 256)), dtype=np.uint8)
    if kind == 5:
        per = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)
        return np.tile(per, n // per.size + 1)[:n]
    if kind == 6:
        return rng.integers(0, int(rng.integers(2, 6)), n, dtype=np.uint8) + np.uint8(rng.integers(0, 250))
    if kind == 7:
        chunk = rng.integers(0, 256, max(1, n // int(rng.integers(2, 9))), dtype=np.uint8)
        return np.tile(chunk, n // chunk.size + 1)[:n]
    if kind == 8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    base = datagen.text_bytes(n, seed=seed)
    base[rng.integers(0, n, max(1, n // 50))] = rng.integers(0, 256, max(1, n // 50), dtype=np.uint8)
    return base


def _block(rng, n):
    parts, left = [], n
    while left > 0:
        m = left if rng.random() < 0.35 else int(rng.integers(1, left + 1))
        parts.append(_piece(rng, m))
        left -= m
    return np.concatenate(parts)[:n]


def test_overflowing_block_is_stored_raw(glc, ctx, cuda):
    """the input of test_gpu_fuzz.py::test_compress_reports_a_block_that_does_not_fit: its third block has a 4096-symbol
    sub-block that needs 1544 words.  The container stores that block raw; glcCompressBatch still reports it."""
    rng = np.random.default_rng(2000 + 5 + 400000)
    n = int(rng.choice([4096, 70000, 1 << 19, 1 << 20]))
    rows = int(rng.integers(1, 5))
    x = np.concatenate([_block(rng, n) for _ in range(rows)])
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        c = glc.container_compress(plan, _gpu(x))
        h = _host(c).tobytes()
        assert h == M.write(x, n, rows)
        data, kinds = M.read(h, with_kinds=True)
        assert kinds[2] == M.RAW
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        glc.compress_batch(plan, _gpu(x), n, rows)
        with pytest.raises(glc.CudppError) as e:
            plan.synchronize()
        assert e.value.code == UNKNOWN


# --- 5. incompressible data ---------------------------------------------------------------------------------------------
def test_random_bytes_are_raw_and_within_the_bound(glc, ctx, cuda):
    import torch
    n, L = 1 << 20, 16 << 20
    x = torch.randint(0, 256, (L,), dtype=torch.uint8, device=cuda)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=4) as plan:
        plan.set_pipelining(True)
        c = glc.container_compress(plan, x)
        assert c.numel() <= glc.container_bound(L, n)
        lay = M.layout(_host(c).tobytes())
        assert all(k == M.RAW for f in lay["frames"] for (_, _, k) in f["records"])
        assert torch.equal(glc.container_decompress(plan, c), x)


# --- 6. every sorter tier in one container ------------------------------------------------------------------------------
def test_mixed_tiers_round_trip(glc, ctx, cuda):
    n = 1 << 18
    per = np.tile(np.frombuffer(b"abcdefgh", np.uint8), n // 8)
    deep = np.tile(datagen.text_bytes(3000, seed=4), n // 3000 + 1)[:n]
    x = np.concatenate([per, datagen.text_bytes(n, seed=5), deep, datagen.zipf_bytes(n, seed=6)])
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=4) as plan:
        c = glc.container_compress(plan, _gpu(x))                       # one frame: the getters describe it
        flagged, general = plan.last_sort_stats()
        assert flagged >= 3 and general >= 1
        assert plan.last_sort_periodic() >= 1
        assert _host(c).tobytes() == M.write(x, n, 4)
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        y = np.concatenate([x, datagen.log_bytes(12345, seed=8)])
        c = glc.container_compress(plan, _gpu(y))
        assert np.array_equal(_host(glc.container_decompress(plan, c)), y)


# --- 7. corruption is refused before decoding ---------------------------------------------------------------------------
def test_corrupted_containers_are_refused(glc, ctx, cuda):
    import torch
    n = 4096
    x = np.concatenate([_kind_data("text", 3 * n, 2), _kind_data("random", 3, 1)])
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=2) as plan:
        c = _host(glc.container_compress(plan, _gpu(x))).tobytes()
        lay = M.layout(c)
        f0, f1, f2 = lay["frames"]
        s0, e0, k0 = f0["records"][1]
        s2, _, k2 = f2["records"][0]
        assert (k0, k2) == (M.HUFF, M.RAW)
        cases = [(5, (1, -1, -1)), (f1["tables"][0] + 700, (2, 1, -1)), ((s0 + e0) // 2, (3, 0, 1)), (s2 + 1, (3, 2, 0)),
                 (lay["trailer"] + 6, (1, 3, -1))]
        guard = 64
        for pos, want in cases:
            b = bytearray(c)
            b[pos] ^= 0x20
            out = torch.full((x.size + guard,), 0xAB, dtype=torch.uint8, device=cuda)
            with pytest.raises(glc.CudppError) as e:
                _decompress_into(glc, plan, bytes(b), out, x.size)
            assert e.value.code == UNKNOWN
            assert glc.container_last_error(plan) == want, pos
            assert bool((out[x.size:] == 0xAB).all())
        for cut in (len(c) - 1, f1["start"] + 40):
            with pytest.raises(glc.CudppError):
                _decompress_into(glc, plan, c[:cut], torch.empty(x.size, dtype=torch.uint8, device=cuda), x.size)
            assert glc.container_last_error(plan)[0] == 5
        assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), x)


def _decompress_into(glc, plan, cont, out, cap):
    import torch
    d = _gpu(np.frombuffer(cont, np.uint8))
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    glc._chk("glcContainerDecompressDevice", glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(),
                                                                                   out.data_ptr(), cap, d_len.data_ptr()))


# --- 7b. what a plan reports of its last calls lives and dies with it -------------------------------------------------------
def _refused_header(glc, plan, c, size):
    import torch
    b = bytearray(c)
    b[0] ^= 0x20                                                # the stream header's magic
    with pytest.raises(glc.CudppError) as e:
        _decompress_into(glc, plan, bytes(b), torch.empty(size, dtype=torch.uint8, device="cuda"), size)
    assert e.value.code == UNKNOWN
    assert glc.container_last_error(plan) == (1, -1, -1)


def test_reports_die_with_their_plan(glc, ctx, cuda):
    """A plan that has failed a decode and made a range read is closed; the next plans, which the allocator may put at its
    address, start with the reports no call has touched."""
    n, rows = 4096, 2
    x = np.concatenate([_kind_data("text", 3 * n, 2), _kind_data("random", 3, 1)])
    a = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    d_c = glc.container_compress(a, _gpu(x))
    c = _host(d_c).tobytes()
    _refused_header(glc, a, c, x.size)
    with glc.container_index(a, d_c) as ix:
        assert np.array_equal(_host(glc.container_read_range(a, ix, d_c, n + 5, n)), x[n + 5:2 * n + 5])
    stats = glc.container_last_range_stats(a)
    assert all(v > 0 for v in stats)
    _refused_header(glc, a, c, x.size)                          # (the range read has reset the triple: leave it non-zero again)
    assert glc.container_last_range_stats(a) == stats
    old = a.handle
    a.close()
    reused = 0
    for _ in range(8):
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as p:
            reused += p.handle == old
            assert glc.container_last_error(p) == (0, -1, -1)
            assert glc.container_last_range_stats(p) == (0, 0, 0)
    print("reports_die_with_their_plan: %d of 8 new plans took the closed plan's handle" % reused)   # (recorded, not asserted)


def test_two_live_plans_do_not_share_reports(glc, ctx, cuda):
    n, rows = 4096, 2
    x = _kind_data("text", 2 * n + 7, 5)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as a, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as b, \
            glc.Plan(ctx, glc.CUDPP_BWT, n) as other:
        c = _host(glc.container_compress(a, _gpu(x))).tobytes()
        _refused_header(glc, a, c, x.size)
        assert glc.container_last_error(b) == (0, -1, -1) and glc.container_last_range_stats(b) == (0, 0, 0)
        assert glc.container_last_error(other) == (0, -1, -1)   # not a COMPRESS plan: no container call behind it, and no error
        assert glc.container_last_range_stats(other) == (0, 0, 0)
        assert np.array_equal(_host(glc.container_decompress(b, _gpu(np.frombuffer(c, np.uint8)))), x)
        assert glc.container_last_error(a) == (1, -1, -1) and glc.container_last_error(b) == (0, -1, -1)


# --- 8. capacity --------------------------------------------------------------------------------------------------------
def test_capacity_is_checked_and_never_passed(glc, ctx, cuda):
    import torch
    n = 70000
    x = _kind_data("text", 2 * n + 999, 9)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=2) as plan:
        need = len(M.write(x, n, 2))
        guard = 256
        for cap in (need - 1, need - 8, 100, 40):
            out = torch.full((cap + guard,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6
            assert int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need
        c = glc.container_compress(plan, _gpu(x), cap=glc.container_bound(x.size, n))
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        with pytest.raises(glc.CudppError) as e:
            glc.container_decompress(plan, c, cap=x.size - 1)
        assert e.value.code == ILLEGAL


# --- 9. host pointers and files -----------------------------------------------------------------------------------------
def test_host_and_file_forms(glc, ctx, cuda, tmp_path):
    n, rows = 65536, 2
    x = np.concatenate([_kind_data(k, 2 * n, 20 + i) for i, k in enumerate(["zipf", "text", "random"])] + [_kind_data("log", 4321, 3)])
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        plan.set_pipelining(True)
        c = glc.container_compress_host(plan, x)
        want = M.write(x, n, rows)
        assert c.tobytes() == want
        assert np.array_equal(glc.container_decompress_host(plan, c), x)
        src, dst, back = tmp_path / "in.bin", tmp_path / "out.glcb", tmp_path / "back.bin"
        x.tofile(src)
        glc.container_compress_file(plan, str(src), str(dst))
        assert dst.read_bytes() == want
        glc.container_decompress_file(plan, str(dst), str(back))
        assert back.read_bytes() == x.tobytes()
        model = tmp_path / "model.glcb"
        y = _kind_data("text", 3 * 70000 + 5, 4)
        model.write_bytes(M.write(y, 70000, 3))
        with glc.Plan(ctx, glc.CUDPP_COMPRESS, 70000, rows=2) as p2:
            glc.container_decompress_file(p2, str(model), str(back))
        assert back.read_bytes() == y.tobytes()
        empty = tmp_path / "empty.bin"
        empty.write_bytes(b"")
        glc.container_compress_file(plan, str(empty), str(dst))
        assert dst.read_bytes() == M.write(b"", n, rows)
        glc.container_decompress_file(plan, str(dst), str(back))
        assert back.read_bytes() == b""


# --- 10. plain C ----------------------------------------------------------------------------------------------------------
def test_plain_c_caller_round_trip(glc, tmp_path):
    glc.lib()
    exe = str(tmp_path / "container_rig")
    cmd = ["gcc", "-O1", "-std=gnu99", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "c_caller", "container_rig.c"), "-o", exe, "-L", PKG, "-lglc_amd", "-L", "/opt/rocm/lib",
           "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    # first the line the rig prints BEFORE it decodes, whatever became of the decode: the container against the model's of
    # the same input (the rig's srand(7) stream, restated).  Only then the return code: a refused decode of a container that
    # equals the model's is the decoder's failure, one of a container that differs the encoder's
    x, want = _rig_input_and_container()
    lines = r.stdout.splitlines()
    assert lines and lines[0].startswith("container_len="), "the rig got no container to report: rc %d\n%s" % (r.returncode, r.stdout + r.stderr)
    pre = dict(kv.split("=") for kv in lines[0].split())
    model = dict(container_len=str(len(want)), container_crc="%08x" % zlib.crc32(want))
    assert pre == model, "the ENCODER wrote other bytes than the model (rig rc %d)\nrig:   %r\nmodel: %r\n%s" % (r.returncode, pre, model, r.stderr)
    assert r.returncode == 0, "the container equals the model's byte for byte, so the DECODER failed on right bytes\n" + r.stdout + r.stderr
    out = dict(kv.split("=") for kv in r.stdout.split())
    assert out["equal"] == "1" and out["input_crc"] == out["gpu_crc"]
    assert int(out["decoded_len"]) == 3 * 65536 + 12345
    assert out["input_crc"] == "%08x" % zlib.crc32(x.tobytes())


def _rig_input_and_container():
    import oracle_lib as O
    n, length = 65536, 3 * 65536 + 12345
    letters = np.frombuffer(b"abcabd, the cat sat on the mat. ", np.uint8)
    x = letters[O.glibc_rand_bytes(length, 32, 7).astype(np.int64) - 1] ^ (np.arange(length) % 977 == 0).astype(np.uint8)
    return x, M.write(x, n, 2)
