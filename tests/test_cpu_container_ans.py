"""The rANS mode of the container's order-0 codec without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the model of record kind 5 and format version 7 (tests/ans_model.py) round-trips, its
quantiser keeps its invariants, its records have the size the formula gives, it reproduces the golden fixture and refuses what
the format forbids; the readers of the other versions refuse version 7 as they always did; the encoder's division is exact."""
import ctypes as C
import importlib.util
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import ans_inputs as I
import ans_model as A
import container_model as M
import hd_table_model
import runs_model
import sparse_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "container_v7_ans.bin")
NEW = ["glcAnsEncodeSegments", "glcAnsDecodeSegments", "glcAnsSegmentsWorkBytes", "glcAnsBoundWords", "glcPlanSetContainerAns",
       "glcPlanGetContainerAns"]
TRIPLES = [(0, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)]
LENGTHS = (1, 63, 64, 65, 4097, 32768, 32769, 70000)


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_ans_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS)
    for name in ("container_set_ans", "container_get_ans", "ans_encode_segments", "ans_decode_segments", "ans_bound_words",
                 "ans_work_bytes"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    d = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for on in (0, 1, 2):
            assert L.glcPlanSetContainerAns(h, on) == HANDLE
        assert L.glcPlanGetContainerAns(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerAns(h, None) == HANDLE
    assert d.value == 77
    for n in LENGTHS + (1 << 20,):
        assert glc.ans_bound_words(n) == A.bound_words(n)
    assert glc.ans_bound_words((1 << 20) + 1) == 0
    need = glc.ans_work_bytes(3, 70000)
    assert need >= 3 * 3 * 65536 + 3 * 6144
    assert glc.ans_work_bytes(3, (1 << 20) + 1) == 0 and glc.ans_work_bytes((1 << 22) + 1, 64) == 0 and glc.ans_work_bytes(0, 0) < 4096
    x, o, n, h, r, ro, rw, w = (0x100000 * k for k in range(1, 9))
    enc, dec = L.glcAnsEncodeSegments, L.glcAnsDecodeSegments
    assert enc(None, None, None, 0, 4096, None, None, None, None, None, 0, None) == glc.CUDPP_SUCCESS      # nothing to do
    assert dec(None, None, None, None, None, None, 0, 4096, None, None, 0, None) == glc.CUDPP_SUCCESS
    egood = [x, o, n, 3, 70000, h, r, ro, rw, w, need]
    dgood = [r, ro, rw, h, o, n, 3, 70000, x, w, need]
    for good, call, ptrs in ((egood, enc, (0, 1, 2, 5, 6, 7, 8, 9)), (dgood, dec, (0, 1, 2, 3, 4, 5, 8, 9))):
        for i in ptrs:                                           # each pointer null in turn
            args = list(good)
            args[i] = None
            assert call(*args, None) == ILLEGAL
        for i, v in ((10, need - 1), (good.index(3), (1 << 22) + 1), (good.index(70000), (1 << 20) + 1), (good.index(r), r + 2),
                     (good.index(h), h + 1), (good.index(x), r)):  # too little work space, too many, too long, misaligned, in place
            args = list(good)
            args[i] = v
            assert call(*args, None) == ILLEGAL


# --- the coder -----------------------------------------------------------------------------------------------------------
def test_quantiser_invariants():
    for hist in hd_table_model.random_histograms():
        n = int(sum(int(v) for v in hist))
        q, _ = A.quantise(hist, n)
        assert int(q.sum()) == A.TOTAL
        assert np.array_equal(q >= 1, np.asarray(hist) > 0)
    q, took = A.quantise([1 << 20] + [0] * 255, 1 << 20)             # the product that needs more than 32 bits
    assert int(q[0]) == 4096 and not took
    q, took = A.quantise([8192 - 255] + [1] * 255, 8192)             # R < 0: the largest gives way
    assert took and int(q[0]) == 4096 - 255 and set(q[1:].tolist()) == {1}
    q, took = A.quantise([10, 10] + [0] * 254, 20)                   # a tie goes to the lower symbol; here there is nothing to give
    assert q[:2].tolist() == [2048, 2048]
    q, _ = A.quantise([1, 1, 1] + [0] * 253, 3)
    assert q[:3].tolist() == [1366, 1365, 1365]


@pytest.mark.parametrize("kind", I.KINDS)
def test_records_round_trip_and_have_the_size_of_the_formula(kind):
    rng = np.random.default_rng(I.KINDS.index(kind))
    for n in LENGTHS:
        x = I.segment(kind, n, rng)
        hist, words = A.encode_record(x)
        nch = A.nchunks(n)
        units = words[:nch]
        assert np.array_equal(hist, np.bincount(x, minlength=256))
        assert words.size == A.words_of(units) == nch + sum(64 + (int(u) + 1) // 2 for u in units) <= A.bound_words(n)
        assert all(int(units[c]) <= A.chunk_len(n, c) for c in range(nch))
        assert np.array_equal(A.decode_record(hist, words, n), x)
        assert not A.check_ans_fields(0, [0], hist, words, 0, words.size, n)


def test_sizes_the_format_promises():
    assert A.encode_record(np.full(32768, 9, np.uint8))[1].size * 4 == 260       # a constant chunk: its count and 64 states
    x = I.segment("scattered", 32768, np.random.default_rng(3))
    p = np.bincount(x, minlength=256) / x.size
    entropy = -(p[p > 0] * np.log2(p[p > 0])).sum() * x.size / 8
    size = A.encode_record(x)[1].size * 4
    assert entropy < size < entropy + 330                                         # the states, and the 12-bit table's loss
    assert size < 4 * M.h0_encode(x)[1].size * 0.8                                # what the mode is for: well below Huffman
    lane_short = A.encode_record(np.full(10, 1, np.uint8))[1]                     # lanes 10 .. 63 never own a symbol
    assert lane_short.size == 65 and set(lane_short[11:].tolist()) == {1 << 16}


# --- the container ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,delta", TRIPLES)
def test_model_round_trip(elem, delta):
    x = I.container_input(elem, delta, n=8192, tail=1235)
    c = A.write(x, 8192, I.rows_of(elem), elem, delta)
    assert struct.unpack("<HHII", c[4:16]) == (7, 1 if delta else 0, 8192, elem)
    y, kinds = A.read(c, with_kinds=True)
    assert np.array_equal(x, y) and set(kinds) == {M.RAW, A.ANS}
    assert len(c) <= M.bound(x.size, 8192)
    for empty in (x[:0], x[:1]):
        assert np.array_equal(A.read(A.write(empty, 8192, 4, elem, delta)), empty)


def test_the_other_readers_refuse_version_7_as_ever():
    gold = open(GOLD, "rb").read()
    for reader in (lambda b: M.read(b), lambda b: sparse_model.read(b), lambda b: runs_model.read(b)):
        with pytest.raises(M.ContainerError) as e:
            reader(gold)
        assert (e.value.what, e.value.frame, e.value.block) == (M.STREAM_HEADER, -1, -1)
    for name in ("container_v5_sparse.bin", "container_v6_runs.bin"):                # and this one refuses versions 5 and 6
        with pytest.raises(M.ContainerError) as e:
            A.read(open(os.path.join(os.path.dirname(GOLD), name), "rb").read())
        assert (e.value.what, e.value.frame, e.value.block) == (M.STREAM_HEADER, -1, -1)


def test_golden_fixture():
    spec = importlib.util.spec_from_file_location("make_v7", os.path.join(ROOT, "tests", "golden", "make_container_v7_gold.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = open(GOLD, "rb").read()
    assert len(gold) <= 32768 and gold == mk.make()
    x, kinds = A.read(gold, with_kinds=True)
    assert np.array_equal(x, mk.gold_input()) and kinds == list(mk.KINDS)
    lay = M.layout(gold)
    assert [f["nb"] for f in lay["frames"]] == [3, 3, 1] and lay["frames"][-1]["blk_len"] == 1235
    s, e, kind = lay["frames"][0]["records"][0]
    assert kind == A.ANS and e - s == 4 * 65                                         # the block of one repeated byte
    blocks = mk.filtered_blocks()
    assert A.quantise(np.bincount(blocks[4], minlength=256), blocks[4].size)[1]      # the R < 0 path


@pytest.mark.parametrize("elem,delta", [(0, False), (8, True)])
def test_refusal_cases(elem, delta):
    x = I.container_input(elem, delta, n=8192)
    c7 = A.write(x, 8192, I.rows_of(elem), elem, delta)
    cases, _ = A.refusal_cases(c7, elem)
    assert len(cases) >= 19
    for name, cont, want in cases:
        with pytest.raises(M.ContainerError) as e:
            A.read(cont)
        assert (e.value.what, e.value.frame, e.value.block) == want, name
    # a reader that does speak version 5 or 6 finds the kind-5 block illegal under it
    for name, cont, want in cases:
        if name.startswith("kind 5 under a version-5"):
            with pytest.raises(M.ContainerError) as e:
                sparse_model.read(cont)
            assert e.value.what == M.FRAME_TABLE, name
        if name.startswith("kind 5 under a version-6"):
            with pytest.raises(M.ContainerError) as e:
                runs_model.read(cont)
            assert e.value.what == M.FRAME_TABLE, name


# --- the division ----------------------------------------------------------------------------------------------------------
def test_the_division_checker_under_the_host_sanitizers(tmp_path):
    """tools/ans_div_check.cpp: ans_div against plain division for every f, built with the address and undefined-behaviour
    sanitizers and run on the CPU (about a second)"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ans_div_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "ans_div_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ans_div_check: ok" in r.stdout, r.stdout + r.stderr
