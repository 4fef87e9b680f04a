"""The BWT container without a GPU: the library exports include/glc_container.h, the CRC algebra the kernel uses equals
zlib.crc32, the Python model of the format (tests/container_model.py) round-trips, reads the golden fixture byte-exactly and
refuses corrupted containers with the right verdict, and a plain-C caller links against the header."""
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import container_model as M
import datagen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-lossless-compression_amd")
GOLD = os.path.join(ROOT, "tests", "golden", "container_v1.bin")


def test_library_exports_every_container_function(glc):
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    names = set(re.findall(r"\b(glc\w+)\s*\(", decl))
    assert names == set(glc.CONTAINER_SYMBOLS)
    L = glc.lib()
    assert [n for n in names if not hasattr(L, n)] == []


def test_bound_depends_on_its_arguments_only(glc):
    for n, bl in [(0, 4096), (1, 4096), (4097, 4096), (3 << 20, 1 << 20), (10 ** 9, 70000)]:
        assert glc.container_bound(n, bl) == M.bound(n, bl)
    assert glc.container_bound(100, 0) == 0 and glc.container_bound(100, (1 << 20) + 1) == 0
    assert M.bound(1 << 30, 1 << 20) - (1 << 30) < 0.003 * (1 << 30)         # (hist + enc_off: ~2 KiB per 1 MiB block)


# --- the CRC algebra ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1, 3, 7, 15])
@pytest.mark.parametrize("chunk", [64, 256, 1024])
def test_crc_rows_and_combine_model_equals_zlib(off, chunk):
    rng = np.random.default_rng(off * 7 + chunk)
    buf = rng.integers(0, 256, 8192 + 32, dtype=np.uint8).tobytes()
    for n in (0, 1, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192):
        assert M.crc_chunked(buf, off, n, chunk) == zlib.crc32(buf[off:off + n]), (off, chunk, n)


def test_crc_combine_over_large_lengths():
    """shifts by x^(8 n) for n up to 3 MiB, and the per-block CRCs folded into the whole input's, as the trailer's crc_all"""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, 3 << 20, dtype=np.uint8).tobytes()
    for cut in (0, 1, 4095, 1 << 20, (3 << 20) - 1, 3 << 20):
        assert M.combine(zlib.crc32(x[:cut]), zlib.crc32(x[cut:]), len(x) - cut) == zlib.crc32(x)
    for bl in (4096, 70000, 1 << 20):
        n = len(x) // bl
        crcs = [zlib.crc32(x[i * bl:(i + 1) * bl]) for i in range(n)]
        assert M.fold_block_crcs(crcs, bl) == zlib.crc32(x[:n * bl])
    assert M.raw_crc(b"") == 0 and M.crc_from_raw(0, 0) == 0


# --- the model writer and reader ---------------------------------------------------------------------------------------
def _data(n, seed):
    return datagen.text_bytes(n, seed=seed) if n else np.zeros(0, np.uint8)


@pytest.mark.parametrize("bl", [4096, 70000])
def test_model_round_trip(bl):
    for n in (0, 1, 2, 4095, 4096, 4097, bl - 1, bl, bl + 1, 3 * bl + 12345):
        x = _data(n, n)
        for rows in (1, 2):
            c = M.write(x, bl, rows)
            assert len(c) <= M.bound(n, bl) and len(c) % 8 == 0
            assert np.array_equal(M.read(c), x), (bl, n, rows)


def test_model_reads_the_golden_fixture_and_rewrites_it():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_container_gold", os.path.join(ROOT, "tests", "golden", "make_container_gold.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    gold = open(GOLD, "rb").read()
    x = g.gold_input()
    data, kinds = M.read(gold, with_kinds=True)
    assert np.array_equal(data, x)
    assert kinds == [M.HUFF, M.HUFF, M.HUFF, M.RAW]
    assert M.write(x, g.BLOCK, g.ROWS) == gold


def test_incompressible_blocks_are_raw_and_the_size_stays_in_the_bound():
    """(4096 random bytes still save a little -- 1023 words --; 70000 of them do not)"""
    bl = 70000
    x = np.random.default_rng(5).integers(0, 256, 3 * bl + 5, dtype=np.uint8)
    x[bl:2 * bl] = datagen.zipf_bytes(bl, seed=1)
    c = M.write(x, bl, 2)
    data, kinds = M.read(c, with_kinds=True)
    assert np.array_equal(data, x) and kinds == [M.RAW, M.HUFF, M.RAW, M.RAW]
    assert len(c) <= M.bound(x.size, bl)


def _flip(c, pos):
    b = bytearray(c)
    b[pos] ^= 0x20
    return bytes(b)


def _refused(c):
    with pytest.raises(M.ContainerError) as e:
        M.read(c)
    return e.value.what, e.value.frame, e.value.block


def test_model_refuses_every_kind_of_corruption():
    x = np.concatenate([datagen.text_bytes(3 * 4096, seed=2), np.random.default_rng(1).integers(0, 256, 3, dtype=np.uint8)])
    c = M.write(x, 4096, 2)
    lay = M.layout(c)
    f0, f1 = lay["frames"][0], lay["frames"][1]
    assert _refused(_flip(c, 5)) == (M.STREAM_HEADER, -1, -1)
    assert _refused(_flip(c, f0["start"] + 8)) == (M.FRAME_TABLE, 0, -1)           # blk_len in a frame header
    assert _refused(_flip(c, f1["tables"][0] + 700)) == (M.FRAME_TABLE, 1, -1)      # a histogram
    s, e, kind = f0["records"][1]
    assert kind == M.HUFF
    assert _refused(_flip(c, (s + e) // 2)) == (M.RECORD_CRC, 0, 1)
    s, e, kind = lay["frames"][2]["records"][0]
    assert kind == M.RAW
    assert _refused(_flip(c, s + 1)) == (M.RECORD_CRC, 2, 0)
    assert _refused(_flip(c, lay["trailer"] + 6)) == (M.STREAM_HEADER, 3, -1)
    assert _refused(c[:-1])[0] == M.TRUNCATED
    assert _refused(c[:f1["start"] + 40])[0] == M.TRUNCATED
    # every byte of the first frame's header and tables, one at a time
    for pos in range(f0["start"], f0["tables"][1], 97):
        assert _refused(_flip(c, pos))[:2] == (M.FRAME_TABLE, 0), pos


def test_plain_c_caller_compiles_and_links_with_gcc(glc, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    glc.lib()
    exe = str(tmp_path / "container_rig")
    cmd = ["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
           os.path.join(ROOT, "tests", "c_caller", "container_rig.c"), "-o", exe, "-L", PKG, "-lglc_amd", "-L", "/opt/rocm/lib",
           "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(exe)


def test_the_settings_checker_under_the_host_sanitizers(tmp_path):
    """tools/ct_settings_check.cpp: the setters' rule, format_of() and reader() of csrc/container_internal.h against a
    restatement of the rule they replaced, over every state setter calls can reach from the default; a host-only build with the
    address and undefined-behaviour sanitizers, run on the CPU"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "ct_settings_check")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tools", "ct_settings_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ct_settings_check: ok, 42 states, " in r.stdout, r.stdout + r.stderr
