"""The auto mode of the container's order-0 codec without a GPU: the library exports the new entry points and validates their
arguments before touching a device; the cost table and the rule of csrc/auto_rule.h, dumped by tools/auto_rule_check.cpp built
under the host sanitizers, equal the big-integer arithmetic and the rule of the model (tests/auto_model.py); the model of format
version 8 round-trips, holds every kind, is never larger than the sparse or the rANS container of the same input, reproduces the
golden fixture, reads every older version of the order-0 codec and refuses what the format forbids; the readers of the other
versions refuse version 8 as they always did."""
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
import auto_inputs as AI
import auto_model as U
import container_model as M
import runs_model
import sparse_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GOLDEN, "container_v8_auto.bin")
NEW = ["glcProbeSegments", "glcPlanSetContainerAuto", "glcPlanGetContainerAuto"]
TRIPLES = [(0, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)]
NONE = (M.STREAM_HEADER, -1, -1)


def _refused(read, cont):
    with pytest.raises(M.ContainerError) as e:
        read(cont)
    return e.value.what, e.value.frame, e.value.block


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_auto_entry_points(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    for name in ("container_set_auto", "container_get_auto", "probe_segments"):
        assert callable(getattr(glc, name))
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW) and "GLC_PROBE_MAX_LEN" in decl


def test_argument_validation_without_gpu(glc):
    """what is refused before any device work; the pointers below are never dereferenced"""
    L = glc._ct()
    ILLEGAL, HANDLE = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION, glc.CUDPP_ERROR_INVALID_HANDLE
    d = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for on in (0, 1, 2):
            assert L.glcPlanSetContainerAuto(h, on) == HANDLE
        assert L.glcPlanGetContainerAuto(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerAuto(h, None) == HANDLE
    assert d.value == 77
    probe = L.glcProbeSegments
    x, o, n, h, u = (0x100000 * k for k in range(1, 6))
    assert probe(None, None, None, 0, 4096, None, None, None) == glc.CUDPP_SUCCESS                 # nothing to do
    good = [x, o, n, 3, 70000, h, u]
    for i in (0, 1, 2, 5, 6):                                    # each pointer null in turn
        args = list(good)
        args[i] = None
        assert probe(*args, None) == ILLEGAL
    for i, v in ((3, (1 << 22) + 1), (4, (1 << 20) + 1), (5, h + 2), (6, u + 1), (6, h)):   # too many, too long, misaligned rows, one row array
        args = list(good)
        args[i] = v
        assert probe(*args, None) == ILLEGAL
    assert probe(None, None, None, (1 << 22) + 1, 64, None, None, None) == ILLEGAL


# --- the rule --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rule_dump(tmp_path_factory):
    """the output of tools/auto_rule_check.cpp, built with the address and undefined-behaviour sanitizers and run on the CPU"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("auto_rule") / "auto_rule_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "auto_rule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "auto_rule_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def test_the_cost_table_equals_the_big_integer_definition(rule_dump):
    got = {int(t[1]): int(t[2]) for t in rule_dump if t[0] == "cost"}
    assert sorted(got) == list(range(1, 4097))
    for q in range(1, 4097):
        assert got[q] == 3072 - ((q ** 256).bit_length() - 1) == int(U.COST[q]), q
    assert (got[4096], got[2048], got[1]) == (0, 256, 3072)
    assert all(got[q] >= got[q + 1] for q in range(1, 4096))


def test_the_programs_estimates_and_choices_equal_the_models(rule_dump):
    cases = [t for t in rule_dump if t[0] == "case"]
    assert len(cases) >= 40
    names, picks = set(), set()
    for t in cases:
        bl, ws, wa, pick = (int(v) for v in t[2:6])
        H = np.asarray([int(v) for v in t[6:]], np.int64)
        assert H.size == 256 and int(H.sum()) == bl
        assert U.words_a(H, bl) == wa, t[1]
        assert pick == (1 if wa < ws else 0), t[1]                 # a tie goes to candidate S
        names.add(t[1])
        picks.add((pick, ws - wa))
    assert {"one-symbol-2^20", "all-256-even-2^20", "all-256-dominant"} <= names
    assert {(1, 1), (0, 0), (0, -1)} <= picks
    H = np.zeros(256, np.int64)
    H[0] = 1 << 20
    assert U.words_a(H, 1 << 20) == 65 * 32                       # cost(4096) = 0: the states alone


def test_the_rule_from_statistics_alone():
    """wS needs no pass over the data: the probe's statistics and whether the short last chunk is all fill give K's counts"""
    rng = np.random.default_rng(11)
    for n in (1, 63, 64, 65, 4099, 8192):
        for blk in (np.zeros(n, np.uint8), I.segment("scattered", n, rng), AI.skewed(rng, n), I.segment("noise", n, rng),
                    np.concatenate([np.zeros(n - n // 3, np.uint8), I.segment("noise", n // 3, rng)])):
            hist, uniform = U.probe(blk)
            assert np.array_equal(hist, np.bincount(blk, minlength=256)) and int(hist.sum()) == n
            fill = S.fill_of(blk)
            assert int(uniform[fill]) == S.elided(blk)
            kind, ws = U.candidate_s(blk)
            got = S.encode_block(blk, "rule")
            assert (kind, ws) == (got[0], got[4].size)
            pick, ws2, wa = U.rule(blk)
            assert ws2 == ws and pick == (A.ANS if wa < ws else "S")


# --- the container ---------------------------------------------------------------------------------------------------------
_CONT = {}


def _containers(elem, delta, n):
    if (elem, delta, n) not in _CONT:
        x = I.container_input(elem, delta, n=n)
        rows = I.rows_of(elem)
        _CONT[elem, delta, n] = x, U.write(x, n, rows, elem, delta), S.write(x, n, rows, elem, delta), A.write(x, n, rows, elem, delta)
    return _CONT[elem, delta, n]


@pytest.mark.parametrize("n", [8192, 70000])
@pytest.mark.parametrize("elem,delta", TRIPLES)
def test_model_round_trip_kinds_and_sizes(elem, delta, n):
    x, c8, c5, c7 = _containers(elem, delta, n)
    assert struct.unpack("<HHII", c8[4:16]) == (8, 1 if delta else 0, n, elem)
    y, kinds = U.read(c8, with_kinds=True)
    assert np.array_equal(x, y) and set(kinds) == {M.RAW, M.HUFF0, S.SPARSE, A.ANS}
    assert len(c8) <= len(c5) and len(c8) <= len(c7) and len(c8) <= M.bound(x.size, n)
    payload = lambda c: sum(e - s for f in M.layout(c)["frames"] for s, e, _ in f["records"])
    assert payload(c8) <= min(payload(c5), payload(c7))
    if n == 8192:
        for empty in (x[:0], x[:1]):
            assert np.array_equal(U.read(U.write(empty, n, 4, elem, delta)), empty)


def test_never_larger_than_either_mode_on_the_when_inputs():
    spec = importlib.util.spec_from_file_location("auto_when", os.path.join(ROOT, "tools", "auto_when.py"))
    aw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(aw)
    inputs = aw.inputs()
    assert len(inputs) == 9
    for name, _, x, elem, delta in inputs:
        sp, an, au, best, kinds = aw.rows_of(x, elem, delta)
        assert best <= au <= min(sp, an), name
        assert len(kinds) == 16


@pytest.mark.parametrize("elem,delta", [(0, False), (8, True)])
def test_misaligned_blocks(elem, delta):
    x = AI.odd_input(elem, delta)
    c = U.write(x, AI.ODD, AI.rows_of(elem), elem, delta)
    y, kinds = U.read(c, with_kinds=True)
    assert np.array_equal(x, y) and {M.HUFF0, S.SPARSE, A.ANS} <= set(kinds)


def test_every_other_reader_refuses_version_8():
    gold = open(GOLD, "rb").read()
    readers = [lambda b: U.read(b, max_version=7), lambda b: U.read(b, reads=("sparse",)), lambda b: U.read(b, reads=("ans",)),
               lambda b: U.read(b, reads=()), lambda b: M.read(b), lambda b: S.read(b), lambda b: A.read(b), lambda b: runs_model.read(b)]
    for reader in readers:
        assert _refused(reader, gold) == NONE
    assert _refused(lambda b: U.read(b, reads=("ans",)), open(os.path.join(GOLDEN, "container_v5_sparse.bin"), "rb").read()) == NONE
    assert _refused(lambda b: U.read(b, reads=("sparse",)), open(os.path.join(GOLDEN, "container_v7_ans.bin"), "rb").read()) == NONE


def test_the_version_8_reader_reads_the_older_golden_files():
    names = sorted(f for f in os.listdir(GOLDEN) if f.startswith("container_v") and f.endswith(".bin"))
    seen = set()
    for name in names:
        buf = open(os.path.join(GOLDEN, name), "rb").read()
        ver = struct.unpack("<H", buf[4:6])[0]
        seen.add(ver)
        if ver == 6:
            assert name == "container_v6_runs.bin" and _refused(U.read, buf) == NONE
            continue
        x = U.read(buf)
        older = {1: M.read, 2: M.read, 3: M.read, 4: M.read, 5: S.read, 7: A.read, 8: U.read}[ver]
        assert np.array_equal(x, older(buf)), name
    assert {1, 2, 3, 4, 5, 6, 7, 8} <= seen


def test_golden_fixture():
    spec = importlib.util.spec_from_file_location("make_v8", os.path.join(GOLDEN, "make_container_v8_gold.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    gold = open(GOLD, "rb").read()
    assert len(gold) <= 32768 and gold == mk.make()
    x, kinds = U.read(gold, with_kinds=True)
    assert np.array_equal(x, mk.gold_input()) and tuple(kinds) == mk.WANT and set(kinds) == {0, 1, 2, 3, 5}
    assert struct.unpack("<HHII", gold[4:16]) == (8, 1, 8192, 8)
    lay = M.layout(gold)
    assert [f["nb"] for f in lay["frames"]] == [3, 3, 1] and lay["frames"][-1]["blk_len"] == 1235
    # but for the forced block, what the rule alone writes
    want = mk.WANT[:1] + (M.HUFF0,) + mk.WANT[2:]
    assert tuple(U.read(U.write(x, mk.BLOCK, mk.ROWS, mk.ELEM, delta=True), with_kinds=True)[1])[0] == want[0]


@pytest.mark.parametrize("elem,delta", [(0, False), (8, True)])
def test_refusal_cases(elem, delta):
    x = AI.odd_input(elem, delta)
    c8 = U.write(x, AI.ODD, AI.rows_of(elem), elem, delta)
    cases, _ = U.refusal_cases(c8, elem)
    names = [name for name, _, _ in cases]
    assert len(cases) >= 30 and "kind 4 under version 8" in names
    assert sum(n.startswith("kind 3: ") for n in names) >= 9 and sum(n.startswith("kind 5: ") for n in names) >= 10
    for name, cont, want in cases:
        assert _refused(U.read, cont) == want, name
        if name == "kind 4 under version 8":
            assert want[0] == M.FRAME_TABLE and want[1] >= 0 and want[2] >= 0
    # the field checks fire with the triples they always had: the sparse and rANS models' own, made from this container
    for model, tag in ((S, "kind 3: "), (A, "kind 5: ")):
        own = {tag + name: want for name, _, want in model.refusal_cases(c8, elem)[0]}
        assert all(own[name] == want for name, _, want in cases if name.startswith(tag))
