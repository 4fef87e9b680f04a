"""The 2-D predictor of the container's filter (format version 12) without a GPU: the library exports the new entry points and
validates their arguments before touching a device; the model (tests/grid_model.py) round-trips over the kernel tests' grid of
shapes, follows the rule element by element, reproduces the golden fixture, reads the older versions, refuses what the format
forbids, and meets tools/grid_when.py's claim on the inputs of tests/grid_inputs.py; format_legal(), the period, the writer's
packing and the setters of csrc/container_internal.h, run by tools/grid_format_check.cpp under the host sanitizers, agree with the
model."""
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
import grid_inputs as GI
import grid_model as G
import lag_model as L
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "grid_v12_container.bin")
NEW = ["glcGridDeltaShuffleDevice", "glcUngridDeltaUnshuffleDevice", "glcUngridDeltaUnshuffleRangeDevice", "glcPlanSetContainerDeltaGrid",
       "glcPlanGetContainerDeltaGrid"]
NONE = (M.STREAM_HEADER, -1, -1)
WIDTHS = (2, 3, 63, 64, 65, 1000, 4096)
N, ROWS = 16384, 4                                                # the small frames of the container tests: 2.5 frames
LENGTH = 5 * N * ROWS // 2

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_grid_v12_gold as gold  # noqa: E402
import make_lag_v11_gold as gold11  # noqa: E402


def lengths(e, W):
    P = G.period(W)
    return (0, e - 1, W * e - 1, P * e, 2 * P * e + 777 * e + (e - 1))


def _refused(read, cont, **kw):
    with pytest.raises(M.ContainerError) as e:
        read(cont, **kw)
    return e.value.what, e.value.frame, e.value.block


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points(glc):
    Lb = glc.lib()
    assert [n for n in NEW if not hasattr(Lb, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("grid_delta_shuffle", "ungrid_delta_unshuffle", "ungrid_delta_unshuffle_range", "container_set_delta_grid", "container_get_delta_grid"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)
    internal = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "container_internal.h")).read()
    assert "CT_VERSION_GRID = %d;" % G.VERSION in internal


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    Lb = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    a, b = C.c_uint(77), C.c_uint(78)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for width, fold in ((0, 0), (1024, 1), (1, 0), (65537, 2)):
            assert Lb.glcPlanSetContainerDeltaGrid(h, width, fold) == HANDLE
        assert Lb.glcPlanGetContainerDeltaGrid(h, C.byref(a), C.byref(b)) == HANDLE
    assert (a.value, b.value) == (77, 78)
    x, y = 0x100000, 0x200000
    for fn in (Lb.glcGridDeltaShuffleDevice, Lb.glcUngridDeltaUnshuffleDevice):
        assert fn(None, None, 0, 4, 1024, 1, None) == glc.CUDPP_SUCCESS                   # nothing to do
        for elem, width, fold in ((3, 64, 1), (0, 64, 1), (16, 64, 0), (4, 0, 0), (4, 1, 0), (4, 65537, 0), (4, 64, 2), (4, 1 << 31, 0), (4, 64, 1 << 31)):
            assert fn(x, y, 4096, elem, width, fold, None) == ILLEGAL
        assert fn(None, y, 4096, 4, 64, 1, None) == ILLEGAL and fn(x, None, 4096, 4, 64, 1, None) == ILLEGAL
        assert fn(x, x + 4095, 4096, 4, 64, 1, None) == ILLEGAL and fn(x + 1, x, 4096, 4, 64, 1, None) == ILLEGAL    # overlapping
    rng = Lb.glcUngridDeltaUnshuffleRangeDevice
    assert rng(x, y, 1 << 20, 4, 100, 1, 4096, 0, None) == glc.CUDPP_SUCCESS              # nothing to do
    for elem, width, fold, first, count in ((4, 0, 0, 0, 8), (4, 65537, 1, 0, 8), (4, 100, 2, 0, 8), (3, 100, 1, 0, 8), (4, 100, 1, 1, 8),
                                            (4, 100, 1, 2048, 8), (4, 100, 1, 4095, 8),       # (the period of width 100 is 4096)
                                            (4, 100, 1, 4096, 1 << 18), (4, 100, 1, (1 << 18) + 4096, 0)):
        assert rng(x, y, 1 << 20, elem, width, fold, first, count, None) == ILLEGAL
    assert rng(x, x + 100, 1 << 20, 4, 100, 1, 0, 8, None) == ILLEGAL                     # overlapping


# --- the transform -----------------------------------------------------------------------------------------------------
def test_the_period():
    assert [G.period(w) for w in (2, 64, 65, 1000, 1024, 1800, 4096, 65536)] == [2048, 2048, 4096, 32768, 32768, 59392, 131072, 2097152]
    for w in range(2, 65537, 97):
        assert G.period(w) % G.RUN == 0 and 32 * w <= G.period(w) < 32 * w + G.RUN


@pytest.mark.parametrize("e", [2, 4, 8])
def test_round_trips_over_the_grid_of_shapes(e):
    for W in WIDTHS:
        for fold in (0, 1):
            for i, n in enumerate(lengths(e, W)):
                x = np.random.default_rng(1000 * e + 10 * W + i).integers(0, 256, n, dtype=np.uint8)
                y = G.grid_delta_shuffle(x, e, W, fold)
                assert y.size == n and np.array_equal(G.ungrid_delta_unshuffle(y, e, W, fold), x), (e, W, fold, n)


def test_the_transform_by_its_definition():
    """element by element on Python integers: a width that divides neither a run nor the period, two bands and a ragged third"""
    e, W, B = 2, 65, 16
    P = G.period(W)
    assert P == 4096
    x = np.random.default_rng(5).integers(0, 1 << B, 2 * P + 300, dtype=np.uint16)
    xs = [int(t) for t in x]
    v = [t if i % P < W else (t - xs[i - W]) % (1 << B) for i, t in enumerate(xs)]
    d = [t if i % G.RUN == 0 else (t - v[i - 1]) % (1 << B) for i, t in enumerate(v)]
    for fold in (0, 1):
        f = [((t << 1) ^ (0 - (t >> (B - 1)))) % (1 << B) for t in d] if fold else d
        want = M.shuffle(np.asarray(f, "<u2").view(np.uint8), e)
        assert np.array_equal(G.grid_delta_shuffle(x.view(np.uint8), e, W, fold), want)
    plane = np.array([[10, 11, 13], [12, 13, 15], [11, 12, 14]], "<i2")      # a plane plus a column pattern: the 2-D residual is 0
    small = G.grid_delta_shuffle(plane.view(np.uint8).reshape(-1), 2, 3, 1).view(np.uint8)[:9]
    assert small.tolist() == [20, 2, 4, 21, 0, 0, 5, 0, 0]    # v = 10 11 13 | 2 2 2 | -1 -1 -1; d = 10 1 2 | -11 0 0 | -3 0 0, folded


@pytest.mark.parametrize("e", [2, 4, 8])
def test_range_inverse_of_the_model(e):
    for W, fold in ((65, 1), (1000, 0), (2, 1)):
        P = G.period(W)
        n = 2 * P * e + 777 * e + (e - 1)
        x = np.random.default_rng(e + W).integers(0, 256, n, dtype=np.uint8)
        y = G.grid_delta_shuffle(x, e, W, fold)
        for first in (0, P, 2 * P):
            for count in (1, P - 1, n // e - first):
                if first + count <= n // e:
                    assert np.array_equal(G.ungrid_delta_unshuffle_range(y, e, W, fold, first, count), x[first * e:(first + count) * e])


# --- format version 12 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c12():
    x = gold.gold_input()
    return x, gold.make()


def test_the_fixture_is_the_writers(c12):
    x, c = c12
    g = open(GOLD, "rb").read()
    assert g == c and 10 << 10 < len(g) < 100 << 10
    assert struct.unpack("<HHII", g[4:16]) == (12, 1 | 2 | 4, gold.BLOCK, 2 | 100 << 8)
    frames = M.layout(g)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(3, gold.BLOCK)] * 2 + [(1, 1235)]
    assert tuple(L.kinds_of(g)) == gold.WANT and set(gold.WANT) == {1, 2, 3, 5}
    assert zlib.crc32(G.read(g).tobytes()) == gold.INPUT_CRC == zlib.crc32(x.tobytes())


def test_small_frames_round_trip():
    for kind, e in GI.KINDS.items():
        for W, fold in ((1024, 1), (721, 0)):
            x = GI.grid_bytes(kind, LENGTH, W)
            c = G.write(x, N, ROWS, e, W, fold)
            assert struct.unpack("<HHII", c[4:16]) == (12, 5 | fold << 1, N, e | W << 8)
            assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(ROWS, N)] * 2 + [(2, N)]
            assert np.array_equal(G.read(c), x)
    for n in (0, 1, 3, 5, N + 9):
        y = GI.grid_bytes("field32", n, 100)
        assert np.array_equal(G.read(G.write(y, N, ROWS, 4, 100, 1)), y)


def test_the_reader_reads_the_older_versions():
    x = GI.grid_bytes("walk32", 2 * N + 5, 64)
    older = [M.write(x, N, 2), M.write(x, N, 2, 4), M.write(x, N, 2, 4, 1), M.write(x, N, 2, 8, 1, delta=True), S.write(x, N, 2, 8, True),
             U.write(x, N, 2, 4, True)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4, 5, 8]
    for c in older:
        assert np.array_equal(G.read(c), x)
    for c in (F.write(x, N, 2), L.write(x, N, 2, 4, 3, 1)):       # versions 10 and 11 are other settings'
        assert _refused(G.read, c) == NONE


def test_refusal_cases(c12):
    x, c = c12
    cases, _ = G.refusal_cases(c, gold11.make())
    names = [k[0] for k in cases]
    for must in ("flags without bit 2", "flags with bit 3", "a non-zero lag field", "width 0", "width 1", "width 65537", "elem 3",
                 "version 12 to a lag plan", "version 12 to an auto plan", "version 12 to a filter-auto plan", "version 12 to a plain plan",
                 "version 11 to a grid plan", "a legal but wrong width: only crc_all sees it"):
        assert must in names
    for name, cont, want, reads in cases:
        assert _refused(G.read, cont, reads=reads) == want, name
    for reads in (L.READS, U.READS_AUTO, F.READS, frozenset(), frozenset(("sparse",)), frozenset(("ans",))):
        assert _refused(G.read, c, reads=reads) == NONE
    assert _refused(U.read, c) == NONE and _refused(M.read, c) == NONE and _refused(F.read, c) == NONE and _refused(L.read, c) == NONE


# --- the claim of tools/grid_when.py -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def when():
    spec = importlib.util.spec_from_file_location("grid_when", os.path.join(ROOT, "tools", "grid_when.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, {(name, w): mod.sizes(x, e, w) for name, e, w, x in mod.inputs(mod.BLOCK * mod.ROWS)}


def test_the_grid_beats_the_folded_delta_on_every_grid_at_every_width(when):
    mod, sizes = when
    assert mod.WIDTHS == (1024, 1800, 721) and len(sizes) == 10
    for kind in GI.KINDS:
        for w in mod.WIDTHS:
            none, delta, fold, grid = sizes[kind, w]
            assert grid < fold and grid < delta and grid < none, (kind, w, sizes[kind, w])


def test_the_grid_loses_on_a_series(when):
    _, sizes = when
    none, delta, fold, grid = sizes["ts64 (no grid)", 1024]
    assert grid > fold


# --- the rule of container_internal.h ---------------------------------------------------------------------------------------
def test_format_rule_period_and_setters_of_the_library_agree_with_the_model(tmp_path):
    """tools/grid_format_check.cpp: format_legal() by brute force over the flag words and the widths, the period, the writer's
    packing and the setter state machine; a host-only build with the address and undefined-behaviour sanitizers, run on the CPU.
    Its legal triples at the widths 2, 1000 and 65536 are the model's."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc for tools/grid_format_check.cpp")
    exe = str(tmp_path / "grid_format_check")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tools", "grid_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "grid_format_check: ok, " in r.stdout, r.stdout[-2000:] + r.stderr
    got = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("legal ")]
    assert len(got) == len(set(got))
    words = [e | w << 8 for e in range(10) for w in (0, 2, 1000, 65536)]
    want = {(v, f, w3) for v in range(14) for w3 in words for f in range(65536 if v == L.VERSION else 16) if G.format_legal(v, f, w3)}
    assert set(got) == want and len([t for t in want if t[0] == G.VERSION]) == 3 * 3 * 2
    total = int(r.stdout.rsplit("ok, ", 1)[1].split()[0])
    assert total == len([t for t in want if t[0] != G.VERSION]) + 3 * 2 * 65535      # every width 2..65536, both folds, three elems
