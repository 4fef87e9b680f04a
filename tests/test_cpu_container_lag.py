"""The lagged, folded delta of the container's filter (format version 11) without a GPU: the library exports the new entry points
and validates their arguments before touching a device; the model (tests/lag_model.py) round-trips over the kernel tests' grid of
shapes, reproduces the golden fixture, reads the older versions, refuses what the format forbids, and meets the ratio conditions
on the inputs of tests/lag_inputs.py; format_legal(), format_of() and the setters of csrc/container_internal.h, run by
tools/lag_format_check.cpp under the host sanitizers, agree with the model's table."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import auto_model as U
import container_model as M
import filter_auto_model as F
import lag_inputs as LI
import lag_model as G
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lag_v11_container.bin")
NEW = ["glcLagDeltaShuffleDevice", "glcUnlagDeltaUnshuffleDevice", "glcUnlagDeltaUnshuffleRangeDevice", "glcPlanSetContainerDeltaLag",
       "glcPlanGetContainerDeltaLag"]
NONE = (M.STREAM_HEADER, -1, -1)
RUN, TILE = 2048, 16384
N, ROWS = 16384, 4                                                # the small frames of the container tests: 2.5 frames
LENGTH = 5 * N * ROWS // 2

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_lag_v11_gold as gold  # noqa: E402


def _refused(read, cont, **kw):
    with pytest.raises(M.ContainerError) as e:
        read(cont, **kw)
    return e.value.what, e.value.frame, e.value.block


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("lag_delta_shuffle", "unlag_delta_unshuffle", "unlag_delta_unshuffle_range", "container_set_delta_lag", "container_get_delta_lag"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)
    internal = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "container_internal.h")).read()
    assert "CT_VERSION_LAG = %d;" % G.VERSION in internal


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    a, b = C.c_uint(77), C.c_uint(78)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for lag, fold in ((1, 0), (2, 1), (0, 0), (17, 2)):
            assert L.glcPlanSetContainerDeltaLag(h, lag, fold) == HANDLE
        assert L.glcPlanGetContainerDeltaLag(h, C.byref(a), C.byref(b)) == HANDLE
    assert (a.value, b.value) == (77, 78)
    x, y = 0x100000, 0x200000
    for fn in (L.glcLagDeltaShuffleDevice, L.glcUnlagDeltaUnshuffleDevice):
        assert fn(None, None, 0, 4, 2, 1, None) == glc.CUDPP_SUCCESS                      # nothing to do
        for elem, lag, fold in ((3, 2, 1), (0, 2, 1), (16, 2, 0), (4, 0, 0), (4, 17, 0), (4, 2, 2), (4, 1 << 31, 0), (4, 1, 1 << 31)):
            assert fn(x, y, 4096, elem, lag, fold, None) == ILLEGAL
        assert fn(None, y, 4096, 4, 2, 1, None) == ILLEGAL and fn(x, None, 4096, 4, 2, 1, None) == ILLEGAL
        assert fn(x, x + 4095, 4096, 4, 2, 1, None) == ILLEGAL and fn(x + 1, x, 4096, 4, 2, 1, None) == ILLEGAL    # overlapping
    rng = L.glcUnlagDeltaUnshuffleRangeDevice
    assert rng(x, y, 1 << 20, 4, 3, 1, 2048, 0, None) == glc.CUDPP_SUCCESS                # nothing to do
    for elem, lag, fold, first, count in ((4, 0, 0, 0, 8), (4, 17, 1, 0, 8), (4, 3, 2, 0, 8), (3, 3, 1, 0, 8), (4, 3, 1, 1, 8), (4, 3, 1, 2047, 8),
                                          (4, 3, 1, 2048, 1 << 18), (4, 3, 1, (1 << 18) + 2048, 0)):
        assert rng(x, y, 1 << 20, elem, lag, fold, first, count, None) == ILLEGAL
    assert rng(x, x + 100, 1 << 20, 4, 3, 1, 0, 8, None) == ILLEGAL                       # overlapping


# --- the transform -----------------------------------------------------------------------------------------------------
def _values(e, n, which, seed):
    dt, top = "<u%d" % e, (1 << (8 * e)) - 1
    q = n // e
    if which == "ones":
        x = np.full(q, top, dtype=dt)
    elif which == "alternating":
        x = np.tile(np.array([0, 1 << (8 * e - 1)], dtype=dt), q // 2 + 1)[:q]
    else:
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return np.concatenate([x.view(np.uint8), np.arange(n - q * e, dtype=np.uint8)])


@pytest.mark.parametrize("e", [2, 4, 8])
def test_round_trips_over_the_grid_of_shapes(e):
    for lag in (1, 2, 3, 5, 8, 16):
        for fold in (0, 1):
            for i, n in enumerate((0, 1, e - 1, e, lag * e - 1, lag * e + e, RUN * e - e, RUN * e, RUN * e + e, TILE, TILE + lag * e + 3, 3 * TILE + 5)):
                for which in ("random", "ones", "alternating"):
                    x = _values(e, n, which, 100 * e + 10 * lag + i)
                    y = G.lag_delta_shuffle(x, e, lag, fold)
                    assert y.size == n and np.array_equal(G.unlag_delta_unshuffle(y, e, lag, fold), x), (e, lag, fold, n, which)
                    if (lag, fold) == (1, 0):
                        assert np.array_equal(y, M.delta_shuffle(x, e))


def test_the_transform_by_its_definition():
    """element by element on Python integers, for a case where RUN % lag != 0 and a chain would cross a run edge"""
    e, lag, W = 2, 3, 16
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1 << W, RUN + 50, dtype=np.uint16)
    for fold in (0, 1):
        f = []
        for i, v in enumerate(int(t) for t in x):
            d = v if i % RUN < lag else (v - int(x[i - lag])) % (1 << W)
            f.append(((d << 1) ^ (0 - (d >> (W - 1)))) % (1 << W) if fold else d)
        want = M.shuffle(np.asarray(f, "<u2").view(np.uint8), e)
        assert np.array_equal(G.lag_delta_shuffle(x.view(np.uint8), e, lag, fold), want)
    small = G.lag_delta_shuffle(np.array([5, 5, 5, 4, 6, 5], "<i2").view(np.uint8), 2, 3, 1)      # differences -1, +1, 0 fold to 1, 2, 0
    assert small.tolist() == [10, 10, 10, 1, 2, 0] + [0] * 6


@pytest.mark.parametrize("e", [2, 4, 8])
def test_range_inverse_of_the_model(e):
    n = 3 * TILE + 2 * RUN * e + 37 * e + (e - 1)
    x = np.random.default_rng(e).integers(0, 256, n, dtype=np.uint8)
    for lag, fold in ((1, 1), (3, 1), (16, 0)):
        y = G.lag_delta_shuffle(x, e, lag, fold)
        for first in (0, RUN, 3 * RUN):
            for count in (1, RUN - 1, RUN, RUN + 1, n // e - first):
                assert np.array_equal(G.unlag_delta_unshuffle_range(y, e, lag, fold, first, count), x[first * e:(first + count) * e])


# --- format version 11 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c11():
    x = gold.gold_input()
    return x, gold.make()


def test_the_fixture_is_the_writers(c11):
    x, c = c11
    g = open(GOLD, "rb").read()
    assert g == c and len(g) < 300 << 10
    assert struct.unpack("<HHII", g[4:16]) == (11, 1 | 2 | 2 << 8, gold.BLOCK, 2)
    frames = M.layout(g)["frames"]
    assert [(f["nb"], f["blk_len"]) for f in frames] == [(3, gold.BLOCK)] * 2 + [(1, 1235)]
    assert tuple(G.kinds_of(g)) == gold.WANT and set(gold.WANT) == {1, 2, 3, 5}
    assert np.array_equal(G.read(g), x)


def test_small_frames_round_trip_and_one_zero_is_version_8():
    for kind, (e, ch) in LI.KINDS.items():
        x = LI.lag_bytes(kind, LENGTH)
        for lag, fold in ((ch, 1), (ch, 0)):
            c = G.write(x, N, ROWS, e, lag, fold)
            assert struct.unpack("<HHII", c[4:16]) == (11, G.flags_of(lag, fold), N, e)
            assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(ROWS, N)] * 2 + [(2, N)]
            assert np.array_equal(G.read(c), x)
        c8 = G.write(x, N, ROWS, e, 1, 0)
        assert c8 == U.write(x, N, ROWS, e, True) and struct.unpack("<HH", c8[4:8]) == (8, 1)
    for n in (0, 1, 3, 5, N + 9):
        y = LI.lag_bytes("xyz32", n)
        assert np.array_equal(G.read(G.write(y, N, ROWS, 4, 3, 1)), y)


def test_the_reader_reads_the_older_versions():
    x = LI.lag_bytes("i32x4", 2 * N + 5)
    older = [M.write(x, N, 2), M.write(x, N, 2, 4), M.write(x, N, 2, 4, 1), M.write(x, N, 2, 8, 1, delta=True), S.write(x, N, 2, 8, True),
             U.write(x, N, 2, 4, True)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4, 5, 8]
    for c in older:
        assert np.array_equal(G.read(c), x)
    with pytest.raises(M.ContainerError):                         # version 10 is filter-auto's
        G.read(F.write(x, N, 2))


def test_refusal_cases(c11):
    x, c = c11
    cases, _ = G.refusal_cases(c)
    names = [k[0] for k in cases]
    for must in ("flags with bit 0 clear", "flags with bit 2 set", "the lag field set under elem 0", "(11, flags 1): what version 8 says",
                 "kind 4 under version 11", "kind 6 under version 11", "a flipped record bit", "a legal but wrong lag: only crc_all sees it",
                 "version 11 to a plan without the setting: the auto mode's", "version 11 to a filter-auto plan"):
        assert must in names
    for name, cont, want, reads in cases:
        assert _refused(G.read, cont, reads=reads) == want, name
    for reads in (U.READS_AUTO, F.READS, frozenset(), frozenset(("sparse",)), frozenset(("ans",))):
        assert _refused(G.read, c, reads=reads) == NONE
    assert _refused(U.read, c) == NONE and _refused(M.read, c) == NONE and _refused(F.read, c) == NONE


# --- the ratio conditions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(LI.KINDS))
def test_lag_equal_to_the_channels_beats_both_version_8_filters(kind):
    e, ch = LI.KINDS[kind]
    x = LI.lag_bytes(kind, LENGTH)
    v8 = min(len(U.write(x, N, ROWS, e, False)), len(U.write(x, N, ROWS, e, True)))
    assert len(G.write(x, N, ROWS, e, ch, 1)) < v8 and len(G.write(x, N, ROWS, e, ch, 0)) < v8


@pytest.mark.parametrize("kind", sorted(LI.FOLD_ONLY))
def test_the_fold_alone_beats_the_plain_delta(kind):
    e = LI.FOLD_ONLY[kind]
    x = LI.fold_bytes(kind, LENGTH)
    assert len(G.write(x, N, ROWS, e, 1, 1)) < len(U.write(x, N, ROWS, e, True))


# --- the rule of container_internal.h ---------------------------------------------------------------------------------------
def test_format_rule_and_setters_of_the_library_agree_with_the_model(tmp_path):
    """tools/lag_format_check.cpp: format_legal() over every (version <= 12, flags, elem <= 9), format_of() and the setter state
    machine; a host-only build with the address and undefined-behaviour sanitizers, run on the CPU.  Its legal triples are the
    model's table."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc for tools/lag_format_check.cpp")
    exe = str(tmp_path / "lag_format_check")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tools", "lag_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lag_format_check: ok, " in r.stdout, r.stdout[-2000:] + r.stderr
    got = {tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("legal ")}
    want = {(v, f, e) for v in range(13) for e in range(10) for f in range(65536 if v == G.VERSION else 16) if G.format_legal(v, f, e)}
    assert got == want and len([t for t in want if t[0] == G.VERSION]) == 3 * 31
    assert all(f < 16 for v, f, e in got if v != G.VERSION)       # (what the model was not asked about is not legal either)
    for v, f, e in got:
        lag, fold = G.lag_fold_of(v, f)
        assert (v == G.VERSION) == ((lag, fold) != (1, 0)) and (v != G.VERSION or f == G.flags_of(lag, fold))
