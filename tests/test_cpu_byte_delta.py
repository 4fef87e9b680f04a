"""The container's byte predictor (format version 15) without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the model (tests/byte_delta_model.py) follows the rule byte by byte in both directions and in
its range form, round-trips containers at every frame cut, reads the older versions, refuses what the format forbids per reader
set, and meets the size orderings of tools/byte_delta_when.py on the inputs of tests/byte_delta_inputs.py; the format rule, the
packing, the setters and the range rounding of csrc/container_internal.h, run by tools/byte_format_check.cpp under the host
sanitizers, agree with the model."""
import ctypes as C
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import auto_model as U
import byte_delta_inputs as BI
import byte_delta_model as B
import container_model as M
import filter_auto_model as F
import lag_model as L
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["glcByteDeltaDevice", "glcUnbyteDeltaDevice", "glcUnbyteDeltaRangeDevice", "glcPlanSetContainerByteDelta", "glcPlanGetContainerByteDelta"]
NONE = (M.STREAM_HEADER, -1, -1)
LAGS, STRIDES = (1, 2, 3, 5, 16), (0, 2, 3, 64, 65, 600, 1281)
N, ROWS = 16384, 4                                                # the small frames of the container tests: 2.5 frames
LENGTH = 5 * N * ROWS // 2


def lengths(lag, S):
    P = B.step(S)
    want = (0, 1, lag - 1, lag, lag + 1, B.RUN - 1, B.RUN, B.RUN + 1, S - 1, S, S + 1, P - 1, P, P + 1, 2 * P + S + 7)
    return sorted({n for n in want if n >= 0})


def naive_forward(x, lag, S):
    """the definition, one Python integer at a time"""
    P = B.period(S) if S else 0
    xs = [int(t) for t in x]
    v = [t if S == 0 or i % P < S else (t - xs[i - S]) % 256 for i, t in enumerate(xs)]
    return np.asarray([t if i % B.RUN < lag else (t - v[i - lag]) % 256 for i, t in enumerate(v)], np.uint8)


def naive_inverse(d, lag, S):
    P = B.period(S) if S else 0
    v, x = [], []
    for i, t in enumerate(int(t) for t in d):
        v.append(t if i % B.RUN < lag else (t + v[i - lag]) % 256)
    for i, t in enumerate(v):
        x.append(t if S == 0 or i % P < S else (t + x[i - S]) % 256)
    return np.asarray(x, np.uint8)


def _refused(read, cont, **kw):
    with pytest.raises(M.ContainerError) as e:
        read(cont, **kw)
    return e.value.what, e.value.frame, e.value.block


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points(glc):
    Lb = glc.lib()
    assert [n for n in NEW if not hasattr(Lb, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("byte_delta", "unbyte_delta", "unbyte_delta_range", "container_set_byte_delta", "container_get_byte_delta"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)
    internal = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "container_internal.h")).read()
    assert "CT_VERSION_BYTE = %d;" % B.VERSION in internal and "CT_READS_BYTE" in internal


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    Lb = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    a, b = C.c_uint(77), C.c_uint(78)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for lag, stride in ((0, 0), (3, 1281), (17, 0), (3, 1)):
            assert Lb.glcPlanSetContainerByteDelta(h, lag, stride) == HANDLE
        assert Lb.glcPlanGetContainerByteDelta(h, C.byref(a), C.byref(b)) == HANDLE
    assert (a.value, b.value) == (77, 78)
    x, y = 0x100000, 0x200000
    for fn in (Lb.glcByteDeltaDevice, Lb.glcUnbyteDeltaDevice):
        assert fn(None, None, 0, 3, 1281, None) == glc.CUDPP_SUCCESS                      # nothing to do
        for lag, stride in ((0, 0), (17, 0), (1 << 31, 0), (1, 1), (3, 65537), (3, 1 << 31), (0, 64)):
            assert fn(x, y, 4096, lag, stride, None) == ILLEGAL
            assert fn(None, None, 0, lag, stride, None) == ILLEGAL                        # (a bad setting is refused at any length)
        assert fn(None, y, 4096, 3, 64, None) == ILLEGAL and fn(x, None, 4096, 3, 64, None) == ILLEGAL
        assert fn(x, x + 4095, 4096, 3, 64, None) == ILLEGAL and fn(x + 1, x, 4096, 3, 64, None) == ILLEGAL      # overlapping
        assert fn(x, x, 4096, 1, 0, None) == ILLEGAL                                      # in place
    rng = Lb.glcUnbyteDeltaRangeDevice
    assert rng(x, y, 1 << 20, 3, 100, 4096, 0, None) == glc.CUDPP_SUCCESS                 # nothing to do
    assert rng(x, y, 1 << 20, 3, 0, 1 << 20, 0, None) == glc.CUDPP_SUCCESS
    for lag, stride, first, count in ((0, 0, 0, 8), (17, 100, 0, 8), (3, 1, 0, 8), (3, 65537, 0, 8), (3, 0, 1, 8), (3, 0, 2047, 8), (3, 100, 1, 8),
                                      (3, 100, 2048, 8), (3, 100, 4095, 8),                   # (the period of stride 100 is 4096)
                                      (3, 100, 4096, 1 << 20), (3, 100, (1 << 20) + 4096, 0), (3, 0, 2048, 1 << 20)):
        assert rng(x, y, 1 << 20, lag, stride, first, count, None) == ILLEGAL
    assert rng(x, x + 100, 1 << 20, 3, 100, 0, 8, None) == ILLEGAL                        # overlapping
    assert rng(None, y, 1 << 20, 3, 100, 0, 8, None) == ILLEGAL and rng(x, None, 1 << 20, 3, 100, 0, 8, None) == ILLEGAL


# --- the transform -----------------------------------------------------------------------------------------------------
def test_the_period_and_the_step():
    assert [B.period(s) for s in (2, 64, 65, 600, 1281, 4096, 65536)] == [2048, 2048, 4096, 20480, 43008, 131072, 2097152]
    assert B.step(0) == B.RUN and B.step(1281) == 43008
    for s in range(2, 65537, 97):
        assert B.period(s) % B.RUN == 0 and 32 * s <= B.period(s) < 32 * s + B.RUN


@pytest.mark.parametrize("lag", LAGS)
def test_forward_and_inverse_agree_with_a_naive_loop(lag):
    for S in STRIDES:
        for i, n in enumerate(lengths(lag, S)):
            x = np.random.default_rng(1000 * lag + 10 * S + i).integers(0, 256, n, dtype=np.uint8)
            want = naive_forward(x, lag, S)
            y = B.byte_delta(x, lag, S)
            assert y.size == n and np.array_equal(y, want), (lag, S, n)
            assert np.array_equal(naive_inverse(want, lag, S), x), (lag, S, n)
            assert np.array_equal(B.unbyte_delta(y, lag, S), x), (lag, S, n)


def test_small_cases_by_hand():
    plane = np.array([[10, 11, 13], [12, 13, 15], [11, 12, 14]], np.uint8)      # a plane plus a column pattern: the 2-D residual is 0
    assert B.byte_delta(plane.reshape(-1), 1, 3).tolist() == [10, 1, 2, 245, 0, 0, 253, 0, 0]   # v = 10 11 13 | 2 2 2 | -1 -1 -1
    rgb = np.array([[5, 100, 200], [6, 101, 201], [8, 103, 203]], np.uint8)     # three channels, each its own level
    assert B.byte_delta(rgb.reshape(-1), 3, 0).tolist() == [5, 100, 200, 1, 1, 1, 2, 2, 2]
    assert B.byte_delta(rgb.reshape(-1), 1, 0).tolist() == [5, 95, 100, 62, 95, 100, 63, 95, 100]
    for lag, S in ((5, 2), (16, 3), (3, 2)):                    # stride < lag is legal: the two differences commute
        y = np.random.default_rng(lag + S).integers(0, 256, 3 * 2048 + 11, dtype=np.uint8)
        assert np.array_equal(B.byte_delta(y, lag, S), naive_forward(y, lag, S)) and np.array_equal(B.unbyte_delta(B.byte_delta(y, lag, S), lag, S), y)


def test_range_inverse_of_the_model():
    for lag, S in ((1, 0), (3, 0), (2, 65), (16, 600), (3, 1281), (5, 2)):
        step = B.step(S)
        n = 4 * step + S + 777
        x = np.random.default_rng(lag + S).integers(0, 256, n, dtype=np.uint8)
        y = B.byte_delta(x, lag, S)
        for first in (0, step, 3 * step):
            for count in (0, 1, step - 1, step, step + 1, n - first):
                assert np.array_equal(B.unbyte_delta_range(y, lag, S, first, count), x[first:first + count]), (lag, S, first, count)
        for first in (1, step - 1, step + 8):
            with pytest.raises(AssertionError):
                B.unbyte_delta_range(y, lag, S, first, 10)
        with pytest.raises(AssertionError):
            B.unbyte_delta_range(y, lag, S, step, n)
        assert B.range_first(step + 5, S) == step and B.range_first(step - 1, S) == 0
    assert B.range_blocks(3 * N + 100, 3 * N + 150, 1281, ROWS, N) == [2, 3] and B.range_blocks(3 * N + 100, 3 * N + 150, 0, ROWS, N) == [3]
    assert B.range_blocks(43004, 43012, 1281, ROWS, N) == [0, 1, 2] and B.range_blocks(0, ROWS * N, 600, ROWS, N) == [0, 1, 2, 3]


# --- format version 15 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c15():
    x = BI.rgb8(LENGTH, 427)
    return x, B.write(x, N, ROWS, 3, 1281)


def test_write_read_round_trips_and_frame_cuts(c15):
    x, c = c15
    assert struct.unpack("<HHII", c[4:16]) == (15, 1 | 4 | 2 << 8, N, 1 | 1281 << 8)
    assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(ROWS, N)] * 2 + [(2, N)]
    assert np.array_equal(B.read(c), x)
    assert set(L.kinds_of(c)) <= {1, 2, 3, 5}
    for lag, S in ((1, 0), (3, 0), (1, 600), (16, 65536), (5, 2)):
        y = BI.grey8(LENGTH, S if 2 <= S <= 4096 else 721)
        c = B.write(y, N, ROWS, lag, S)
        assert struct.unpack("<HHII", c[4:16]) == (15, B.flags_of(lag, S), N, B.word3_of(S))
        assert np.array_equal(B.read(c), y)
    for n in (0, 1, 3, N - 1, N, N + 9, N * ROWS, N * ROWS + 1, N * ROWS + 2049):
        y = x[:n]
        c = B.write(y, N, ROWS, 3, 1281)
        cut = F.cut(n, N, ROWS)
        assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(nb, bl) for _, nb, bl in cut]
        assert np.array_equal(B.read(c), y)
    # every frame is a segment of its own: the second frame's bytes do not depend on the first's
    two = B.write(x[:2 * N * ROWS], N, ROWS, 3, 1281)
    second = B.write(x[N * ROWS:2 * N * ROWS], N, ROWS, 3, 1281)
    fr2, fr = M.layout(two)["frames"][1], M.layout(second)["frames"][0]
    assert two[fr2["start"] + 32:fr2["start"] + 32 + 64] == second[fr["start"] + 32:fr["start"] + 32 + 64]
    # forced kinds: every kind version 8 has
    for kinds in ((1,), (2,), (3,), (5,), (2, 5, 3, 1)):
        c = B.write(x[:N * ROWS + 77], N, ROWS, 3, 1281, kinds=kinds)
        assert np.array_equal(B.read(c), x[:N * ROWS + 77])


def test_with_the_setting_off_the_writer_is_the_auto_modes(c15):
    x, _ = c15
    assert B.write(x, N, ROWS, 0, 0) == U.write(x, N, ROWS) and struct.unpack("<HHII", U.write(x, N, ROWS)[4:16]) == (8, 0, N, 0)


def test_the_reader_reads_the_older_versions():
    x = BI.stereo8(2 * N + 5)
    older = [M.write(x, N, 2), M.write(x, N, 2, 4), M.write(x, N, 2, 4, 1), M.write(x, N, 2, 8, 1, delta=True), S.write(x, N, 2, 8, True),
             U.write(x, N, 2, 4, True), U.write(x, N, 2)]
    assert [struct.unpack("<H", c[4:6])[0] for c in older] == [1, 2, 3, 4, 5, 8, 8]
    for c in older:
        assert np.array_equal(B.read(c), x)
    for c in (F.write(x, N, 2), L.write(x, N, 2, 4, 3, 1)):       # versions 10 and 11 are other settings'
        assert _refused(B.read, c) == NONE


def test_refusal_cases(c15):
    x, c = c15
    cases, _ = B.refusal_cases(c)
    names = [k[0] for k in cases]
    for must in ("flags with bit 0 clear", "the fold bit", "flags with bit 3", "bit 2 against the stride", "stride 1", "stride 65537", "elem 0",
                 "elem 2", "(15, 0, 0)", "version 16", "a non-zero frame word", "a flipped record bit", "kind 4 under version 15",
                 "a legal but wrong lag: only crc_all sees it", "a legal but wrong stride: only crc_all sees it", "cut inside the last frame",
                 "version 15 to an auto plan", "version 15 to a lag plan", "version 15 to a grid plan", "version 15 to a filter-auto plan",
                 "version 15 to a plain plan"):
        assert must in names
    for name, cont, want, reads in cases:
        assert _refused(B.read, cont, reads=reads) == want, name
    for reads in (L.READS, U.READS_AUTO, F.READS, frozenset(), frozenset(("sparse",)), frozenset(("ans",))):
        assert _refused(B.read, c, reads=reads) == NONE
    assert _refused(U.read, c) == NONE and _refused(M.read, c) == NONE and _refused(F.read, c) == NONE and _refused(L.read, c) == NONE
    flat = B.write(x[:N + 9], N, ROWS, 4, 0)                      # a stride-0 stream: the same header refusals
    _, flags, _, word3 = struct.unpack("<HHII", flat[4:16])
    assert (flags, word3) == (1 | 3 << 8, 1)
    for fl, w3 in ((flags | 4, word3), (flags, 1 | 2 << 8), (flags | 2, word3), (flags, 0), (0, 0)):
        assert _refused(B.read, M.with_header(flat, B.VERSION, fl, w3)) == NONE
    one = B.write(x[:N + 9], N, ROWS, 1, 0)                       # (lag 1, stride 0) is legal: no older version can say it
    assert struct.unpack("<HHII", one[4:16]) == (15, 1, N, 1) and np.array_equal(B.read(one), x[:N + 9])


# --- the size orderings of tools/byte_delta_when.py -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def when():
    spec = importlib.util.spec_from_file_location("byte_delta_when", os.path.join(ROOT, "tools", "byte_delta_when.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert (mod.BLOCK, mod.ROWS) == (65536, 4)
    return {name.split(",")[0] + ("" if "width" not in name else " " + name.split("width ")[1].split(",")[0].split(" ")[0]): mod.sizes(x, ch, stride)
            for name, x, ch, stride in mod.inputs(mod.BLOCK * mod.ROWS)}


def test_the_row_above_helps_an_image(when):
    for name in ("grey8 721", "grey8 1800", "grey8 640"):
        none, lag1, _, two_d, _ = when[name]
        assert two_d < lag1 < none, (name, when[name])
    none, lag1, lag3, two_d1, two_d3 = when["rgb8 427"]
    assert two_d3 < lag3 < none and two_d3 < two_d1, when["rgb8 427"]
    assert 1.12 * two_d3 < lag3 and 1.12 * two_d3 < two_d1          # (the margins of the table are 12 % or more)


def test_lag_one_hurts_interleaved_channels_and_the_lag_fixes_it(when):
    for name in ("rgb8 427", "stereo u8 audio"):
        none, lag1, lagc = when[name][:3]
        assert lag1 > none and 1.12 * lagc < none, (name, when[name])


def test_it_loses_on_text_and_does_nothing_on_noise(when):
    none, lag1 = when["text"][:2]
    assert none < lag1
    none, lag1 = when["noise"][:2]
    assert none == lag1


# --- the rule of container_internal.h ---------------------------------------------------------------------------------------
def test_format_rule_packing_setters_and_rounding_of_the_library_agree_with_the_model(tmp_path):
    """tools/byte_format_check.cpp: version 15's legality over every flags word, the packing round trip for every (lag, stride), the
    setter state machine and the range rounding rule; a host-only build with the address and undefined-behaviour sanitizers, run as
    a stand-alone program on the CPU.  Its legal pairs at the strides 0, 2, 1281 and 65536 are the model's."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc for tools/byte_format_check.cpp")
    exe = str(tmp_path / "byte_format_check")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tools", "byte_format_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "byte_format_check: ok, " in r.stdout, r.stdout[-2000:] + r.stderr
    got = [tuple(int(v) for v in line.split()[1:]) for line in r.stdout.splitlines() if line.startswith("legal ")]
    assert len(got) == len(set(got))
    strides = (0, 2, 1281, 65536)
    want = {(f, w3) for w3 in (e | s << 8 for e in range(10) for s in strides + (1, 65537)) for f in range(65536) if B.format_legal(f, w3)}
    assert set(got) == want == {(B.flags_of(lag, s), B.word3_of(s)) for lag in range(1, 17) for s in strides}
    counts = r.stdout.rsplit("ok, ", 1)[1].split()
    assert int(counts[0]) == 16 * 8                               # the legal ones of the twelve strides it tries: 0, 2, 3, 64, 600, 1281, 65535, 65536
    assert int(counts[2]) == 16 * 65536                           # every lag with stride 0 and 2..65536
    assert int(counts[4]) > 40 and int(counts[6]) > 4000          # states, calls
