"""The 3-D predictor of the container's filter (format version 17) without a GPU: the library exports the new entry points and
validates their arguments before touching a device; the model (tests/vol_model.py) round-trips over the kernel tests' grid of
shapes, follows the rule element by element, is grid_model's where no element has a plane behind it, reproduces the golden
fixture, reads the older versions, refuses what the format forbids (a non-zero word 7 under another version included), and meets
tools/vol_when.py's table as INTEGRATION.md prints it; the header rule, the slab arithmetic, the range rounding and the setters of
csrc/container_internal.h, run by tools/vol_format_check.cpp under the host sanitizers, agree with the model."""
import ctypes as C
import importlib.util
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import auto_model as U
import container_model as M
import filter_auto_model as F
import grid_model as G
import lag_model as L
import vol_inputs as VI
import vol_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "vol_v17_container.bin")
NEW = ["glcVolDeltaShuffleDevice", "glcUnvolDeltaUnshuffleDevice", "glcUnvolDeltaUnshuffleRangeDevice", "glcPlanSetContainerDeltaVolume",
       "glcPlanGetContainerDeltaVolume", "glcContainerIndexPlane"]
NONE = (M.STREAM_HEADER, -1, -1)
WIDTHS = (5, 64, 100)

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_grid_v12_gold as gold12  # noqa: E402
import make_vol_v17_gold as gold  # noqa: E402


def planes(W):
    return (W + 1, 1000, 1003, 7 * W + 3, 5000)


def lengths(e, W, S):
    Q = V.slab(W, S)
    return (0, e - 1, S * e - 1, 5 * Q * e // 2 + 3 * e + (e - 1))


def _refused(read, cont, **kw):
    with pytest.raises(M.ContainerError) as e:
        read(cont, **kw)
    return e.value.what, e.value.frame, e.value.block


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points(glc):
    Lb = glc.lib()
    assert [n for n in NEW if not hasattr(Lb, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("vol_delta_shuffle", "unvol_delta_unshuffle", "unvol_delta_unshuffle_range", "container_set_delta_volume", "container_get_delta_volume"):
        assert callable(getattr(glc, name))
    assert callable(glc.ContainerIndex.plane)
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)
    internal = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "container_internal.h")).read()
    assert "CT_VERSION_VOL = %d;" % V.VERSION in internal


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    Lb = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    a = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for plane in (0, 300, 1 << 24, (1 << 24) + 1):
            assert Lb.glcPlanSetContainerDeltaVolume(h, plane) == HANDLE
        assert Lb.glcPlanGetContainerDeltaVolume(h, C.byref(a)) == HANDLE
    assert a.value == 77
    assert Lb.glcContainerIndexPlane(None, C.byref(a)) == ILLEGAL and a.value == 77
    x, y = 0x100000, 0x200000
    for fn in (Lb.glcVolDeltaShuffleDevice, Lb.glcUnvolDeltaUnshuffleDevice):
        assert fn(None, None, 0, 4, 20, 300, 1, None) == glc.CUDPP_SUCCESS                # nothing to do
        for elem, width, plane, fold in ((3, 20, 300, 1), (0, 20, 300, 1), (16, 20, 300, 0), (4, 0, 300, 0), (4, 1, 300, 0), (4, 65537, 70000, 0),
                                         (4, 20, 300, 2), (4, 20, 20, 1), (4, 20, 19, 1), (4, 20, 0, 1), (4, 20, (1 << 24) + 1, 1), (4, 20, 1 << 31, 0),
                                         (4, 65536, 65536, 0)):
            assert fn(x, y, 4096, elem, width, plane, fold, None) == ILLEGAL
            assert fn(None, None, 0, elem, width, plane, fold, None) == ILLEGAL           # (refused before the length is looked at)
        assert fn(None, y, 4096, 4, 20, 300, 1, None) == ILLEGAL and fn(x, None, 4096, 4, 20, 300, 1, None) == ILLEGAL
        assert fn(x, x + 4095, 4096, 4, 20, 300, 1, None) == ILLEGAL and fn(x + 1, x, 4096, 4, 20, 300, 1, None) == ILLEGAL    # overlapping
    rng = Lb.glcUnvolDeltaUnshuffleRangeDevice
    assert V.slab(20, 300) == 6144
    assert rng(x, y, 1 << 20, 4, 20, 300, 1, 6144, 0, None) == glc.CUDPP_SUCCESS          # nothing to do
    for elem, width, plane, fold, first, count in ((4, 0, 300, 0, 0, 8), (4, 20, 20, 1, 0, 8), (4, 20, (1 << 24) + 1, 1, 0, 8), (4, 20, 300, 2, 0, 8),
                                                   (3, 20, 300, 1, 0, 8), (4, 20, 300, 1, 1, 8), (4, 20, 300, 1, 2048, 8), (4, 20, 300, 1, 4096, 8),
                                                   (4, 20, 300, 1, 6143, 8), (4, 20, 300, 1, 6144, 1 << 18), (4, 20, 300, 1, 43 * 6144, 0)):
        assert rng(x, y, 1 << 20, elem, width, plane, fold, first, count, None) == ILLEGAL
    assert rng(x, x + 100, 1 << 20, 4, 20, 300, 1, 0, 8, None) == ILLEGAL                 # overlapping


# --- the transform -----------------------------------------------------------------------------------------------------
def test_the_slab():
    assert [V.slab(w, s) for w, s in ((20, 300), (2, 3), (64, 4096), (50, 2057), (100, 1000), (65536, 1 << 24))] == [6144, 2048, 65536, 34816, 16384, 1 << 28]
    for w in (2, 5, 64, 65, 100, 1000, 65536):
        for s in (w + 1, 7 * w + 3, 131072, (1 << 24) - 1, 1 << 24):
            if s > w:
                q = V.slab(w, s)
                assert q % G.period(w) == 0 and q % V.RUN == 0 and 16 * s <= q < 16 * s + G.period(w) and q <= (1 << 28) + (1 << 21)


@pytest.mark.parametrize("e", [2, 4, 8])
def test_round_trips_over_the_grid_of_shapes(e):
    for W in WIDTHS:
        for S in planes(W):
            for fold in (0, 1):
                for i, n in enumerate(lengths(e, W, S)):
                    x = np.random.default_rng(1000 * e + 10 * W + S + i).integers(0, 256, n, dtype=np.uint8)
                    y = V.vol_delta_shuffle(x, e, W, S, fold)
                    assert y.size == n and np.array_equal(V.unvol_delta_unshuffle(y, e, W, S, fold), x), (e, W, S, fold, n)


def test_the_transform_by_its_definition():
    """element by element on Python integers: a stride that is no multiple of the width, two slabs and a ragged third"""
    e, W, S, B = 2, 20, 143, 16
    P, Q = G.period(W), V.slab(W, S)
    assert (P, Q) == (2048, 4096) and S % W
    x = np.random.default_rng(17).integers(0, 1 << B, 2 * Q + 300, dtype=np.uint16)
    xs = [int(t) for t in x]
    w = [t if i % Q < S else (t - xs[i - S]) % (1 << B) for i, t in enumerate(xs)]
    v = [t if i % P < W else (t - w[i - W]) % (1 << B) for i, t in enumerate(w)]
    d = [t if i % V.RUN == 0 else (t - v[i - 1]) % (1 << B) for i, t in enumerate(v)]
    for fold in (0, 1):
        f = [((t << 1) ^ (0 - (t >> (B - 1)))) % (1 << B) for t in d] if fold else d
        want = M.shuffle(np.asarray(f, "<u2").view(np.uint8), e)
        assert np.array_equal(V.vol_delta_shuffle(x.view(np.uint8), e, W, S, fold), want)
    # a trilinear ramp a + b x + c y + d z + products of two: the 3-D residual is 0 off the first row, column and plane
    z, y, xx = np.meshgrid(np.arange(3), np.arange(3), np.arange(4), indexing="ij")
    vol = (7 + 2 * xx + 3 * y + 5 * z + xx * y + 2 * y * z + xx * z).astype("<i2")
    out = V.vol_delta_shuffle(vol.view(np.uint8).reshape(-1), 2, 4, 12, 0)[:36].astype(np.int8).reshape(3, 3, 4)
    assert not out[1:, 1:, 1:].any() and out[1:, 1:, :].any()


@pytest.mark.parametrize("e", [2, 4, 8])
def test_no_plane_behind_is_the_grid(e):
    for W, fold in ((5, 1), (100, 0)):
        n = 3 * G.period(W) * e + 5 * e + 1
        x = np.random.default_rng(e + W).integers(0, 256, n, dtype=np.uint8)
        for S in (n // e, n // e + 1, 1 << 24):
            assert np.array_equal(V.vol_delta_shuffle(x, e, W, S, fold), G.grid_delta_shuffle(x, e, W, fold))
        assert not np.array_equal(V.vol_delta_shuffle(x, e, W, W + 1, fold), G.grid_delta_shuffle(x, e, W, fold))


@pytest.mark.parametrize("e", [2, 4, 8])
def test_range_inverse_of_the_model(e):
    for W, S, fold in ((5, 6, 1), (100, 1003, 0), (64, 451, 1)):
        Q = V.slab(W, S)
        n = 5 * Q * e // 2 + 3 * e + (e - 1)
        x = np.random.default_rng(e + W).integers(0, 256, n, dtype=np.uint8)
        y = V.vol_delta_shuffle(x, e, W, S, fold)
        for first in (0, Q, 2 * Q):
            for count in (1, Q - 1, n // e - first):
                if first + count <= n // e:
                    assert np.array_equal(V.unvol_delta_unshuffle_range(y, e, W, S, fold, first, count), x[first * e:(first + count) * e])
        assert V.range_first(Q + 17, W, S) == Q and V.range_first(Q - 1, W, S) == 0 and V.range_first(2 * Q, W, S) == 2 * Q


# --- format version 17 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c17():
    x = gold.gold_input()
    return x, gold.make()


def test_the_fixture_is_the_writers(c17):
    x, c = c17
    g = open(GOLD, "rb").read()
    assert g == c and 10 << 10 < len(g) < 100 << 10
    assert struct.unpack("<HHII", g[4:16]) == (17, 1 | 2 | 4 | 8, gold.BLOCK, 2 | 20 << 8)
    assert struct.unpack("<II", g[24:32]) == (zlib.crc32(g[:24] + g[28:32]), 300)
    frames = M.layout(g)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(3, gold.BLOCK)] * 2 + [(1, 1235)]
    assert V.slab(20, 300) * 2 < 3 * gold.BLOCK + 1                   # a full frame is longer than a slab
    assert tuple(L.kinds_of(g)) == gold.WANT and set(gold.WANT) == {1, 2, 3, 5}
    assert zlib.crc32(V.read(g).tobytes()) == gold.INPUT_CRC == zlib.crc32(x.tobytes())


def test_small_frames_round_trip():
    N, ROWS = 16384, 4
    for kind, e in VI.KINDS.items():
        for (W, S), fold in zip(VI.STRIDES, (1, 0)):
            x = VI.vol_bytes(kind, 5 * N * ROWS // 2, W, S)
            c = V.write(x, N, ROWS, e, W, S, fold)
            assert struct.unpack("<HHII", c[4:16]) == (17, 13 | fold << 1, N, e | W << 8) and struct.unpack("<I", c[28:32]) == (S,)
            assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(ROWS, N)] * 2 + [(2, N)]
            assert np.array_equal(V.read(c), x)
    for n in (0, 1, 3, 5, N + 9):
        y = VI.vol_bytes("smooth32", n, 20, 300)
        assert np.array_equal(V.read(V.write(y, N, ROWS, 4, 20, 300, 1)), y)


def test_the_reader_reads_the_older_versions():
    N = 16384
    x = VI.vol_bytes("ct16", 2 * N + 5, 64, 4096)
    older = [M.write(x, N, 2), M.write(x, N, 2, 4), M.write(x, N, 2, 4, 1), M.write(x, N, 2, 8, 1, delta=True), U.write(x, N, 2, 4, True),
             G.write(x, N, 2, 2, 64, 1)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4, 8, 12]
    for c in older:
        assert np.array_equal(V.read(c), x)
    for c in (F.write(x, N, 2), L.write(x, N, 2, 4, 3, 1)):       # versions 10 and 11 are other settings'
        assert _refused(V.read, c) == NONE


def test_refusal_cases(c17):
    x, c = c17
    cases, _ = V.refusal_cases(c, gold12.make())
    names = [k[0] for k in cases]
    for must in ("flags without bit 3", "plane 0", "plane == width", "plane 2^24 + 1", "word 7 changed under the old CRC", "word 6 over words 0..5 alone",
                 "version 12 with a non-zero word 7", "version 8 with a non-zero word 7", "version 17 to a grid plan", "version 17 to a lag plan",
                 "version 17 to an auto plan", "version 17 to a plain plan", "a legal but wrong plane: only crc_all sees it"):
        assert must in names
    for name, cont, want, reads in cases:
        assert _refused(V.read, cont, reads=reads) == want, name
    for reads in (G.READS, L.READS, U.READS_AUTO, F.READS, frozenset(), frozenset(("sparse",)), frozenset(("vol",)) - {"vol"}):
        assert _refused(V.read, c, reads=reads) == NONE
    assert _refused(U.read, c) == NONE and _refused(M.read, c) == NONE and _refused(F.read, c) == NONE and _refused(L.read, c) == NONE
    assert _refused(G.read, c) == NONE


def test_the_header_rule_of_the_model():
    for fold in (0, 1):
        for e in (2, 4, 8):
            assert V.format_legal(17, 13 | fold << 1, e | 20 << 8, 300) and V.format_legal(17, 13 | fold << 1, e | 65536 << 8, 1 << 24)
            assert not V.format_legal(17, 13 | fold << 1, e | 20 << 8, 20) and not V.format_legal(17, 5 | fold << 1, e | 20 << 8, 300)
            assert V.format_legal(12, 5 | fold << 1, e | 20 << 8, 0) and not V.format_legal(12, 5 | fold << 1, e | 20 << 8, 300)
            assert not V.format_legal(12, 13 | fold << 1, e | 20 << 8, 0)
    for v in range(1, 12):
        for f in (0, 1):
            for e in (0, 2, 4, 8):
                assert V.format_legal(v, f, e, 0) == L.format_legal(v, f, e) and not V.format_legal(v, f, e, 300)


# --- the claim of tools/vol_when.py --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def when():
    spec = importlib.util.spec_from_file_location("vol_when", os.path.join(ROOT, "tools", "vol_when.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, {(name, w, s): mod.sizes(x, e, w, s) for name, e, w, s, x in mod.inputs(mod.BLOCK * mod.ROWS)}


def test_the_volume_beats_the_grid_on_every_smooth_input_at_every_stride(when):
    _, sizes = when
    assert len(sizes) == len(VI.KINDS) * len(VI.STRIDES) == 12 and set(VI.SMOOTH) == {"smooth32", "smooth64", "round32", "ct16"}
    for kind in VI.SMOOTH:
        for w, s in VI.STRIDES:
            delta, fold, grid, vol = sizes[kind, w, s]
            assert vol < grid and vol < fold and vol < delta, (kind, w, s, sizes[kind, w, s])


def test_the_volume_loses_on_a_noisy_stack_and_on_a_series(when):
    _, sizes = when
    for kind in ("ct16n", "series"):
        for w, s in VI.STRIDES:
            delta, fold, grid, vol = sizes[kind, w, s]
            assert vol > grid, (kind, w, s)


def test_the_when_table_of_the_integration_guide_is_the_measured_one(when):
    _, sizes = when
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = {}
    for line in doc.splitlines():
        c = [t.strip() for t in line.strip().strip("|").split("|")]
        if len(c) == 9 and c[0] in VI.KINDS and c[1].isdigit():
            rows[c[0], int(c[2]), int(c[3])] = (int(c[1]),) + tuple(int(t) for t in c[4:8]) + (c[8],)
    assert set(rows) == set(sizes)
    for k, t in sizes.items():
        assert rows[k] == (VI.KINDS[k[0]],) + t + ("%.2f" % (t[2] / t[3]),), k


# --- the rule of container_internal.h ---------------------------------------------------------------------------------------
def test_header_rule_slab_and_setters_of_the_library_agree_with_the_model(tmp_path):
    """tools/vol_format_check.cpp: check_stream_header() by brute force over versions, flag words, words 3 and words 7 under both
    ways of counting word 6, the slab at its limits, the range rounding and the setter state machine; a host-only build with the
    address and undefined-behaviour sanitizers, run on the CPU.  The headers it accepts are the model's."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc for tools/vol_format_check.cpp")
    exe = str(tmp_path / "vol_format_check")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tools", "vol_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "vol_format_check: ok, " in r.stdout, r.stdout[-2000:] + r.stderr
    got = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("legal ")]
    assert len(got) == len(set(got))
    flags17 = list(range(32)) + [f | 1 << b for b in range(5, 16) for f in (13, 15)]
    words3 = [e | w << 8 for e in range(10) for w in (0, 1, 2, 20, 65535, 65536, 65537, 1 << 20)]
    words7 = [0, 1, 2, 3, 20, 21, 300, 65536, 65537, 65538, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 1 << 31, (1 << 32) - 1]
    want17 = {(17, f, w3, w7) for f in flags17 for w3 in words3 for w7 in words7 if V.format_legal(17, f, w3, w7)}
    assert {t for t in got if t[0] == 17} == want17 and len(want17) == 2 * 3 * (9 + 7 + 5 + 4)
    # the other versions: word 7 at 0 always, and what the models of versions 1 to 12 accept is accepted
    rest = {t for t in got if t[0] != 17}
    assert all(t[3] == 0 for t in rest)
    assert {t[:3] for t in rest if t[0] <= 12} == {(v, f, w3) for v in range(13) for f in flags17 for w3 in words3 if G.format_legal(v, f, w3)}
    assert {t[0] for t in rest} <= set(range(1, 17))
    assert int(r.stdout.rsplit("ok, ", 1)[1].split()[0]) == len(got)
