"""The CHOOSE codec with filters without a GPU: the library's new exports and the rule's constants; the classes of
tests/choose_filters_model.py on one 1 MiB block of each of the twelve inputs of the "filter: when" table and on the 8-bit images
of the byte tests; the model's containers of the mixed input at every level read back through the existing model reader of the
level's version; at 64 KiB blocks the level-4 and level-5 containers are smaller than the model's CHOOSE, BWT and filter-auto
containers (the frames' filters are those of tests/golden/choose_filters_picks.json, which tools/choose_filters_when.py writes:
the grid rule of the models needs minutes on these frames); on an input whose blocks are all typed with one element size the
container is the order-0 plan's, byte for byte; and tools/class_rule_check.cpp, csrc/class_rule.h and the setter's state walk
against long-hand arithmetic under the host sanitizers, its named cases against the model."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import byte_delta_inputs as BI
import choose_filters_inputs as CI
import choose_filters_model as CF
import choose_model as CM
import container_model as M
import filter_auto_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICKS = json.load(open(os.path.join(ROOT, "tests", "golden", "choose_filters_picks.json")))
NEW = ["glcPlanSetContainerChooseFilters", "glcPlanGetContainerChooseFilters"]
TYPED = {"float32": 4, "smooth32": 4, "smooth64": 8, "quant16": 2, "ts64": 8, "ids32": 4, "ctr32": 4, "adc16": 2}


def _keys(blk):
    """the key of a block at levels 0 to 5, its probes made once"""
    cost, stats = CF.block_costs(blk, 5), CM.stats(blk)
    return [CF.key_from(level, blk.size, cost, stats) for level in range(6)]


# --- the library -------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points_and_the_rule_has_its_constants(glc):
    L = glc.lib()
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(glc.CONTAINER_SYMBOLS) and not set(NEW) & set(glc.RANGE_SYMBOLS)
    assert callable(glc.container_set_choose_filters) and callable(glc.container_get_choose_filters)
    decl = open(os.path.join(ROOT, "include", "glc_container.h")).read()
    assert all(n + "(" in decl for n in NEW)
    rule = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "class_rule.h")).read()
    assert "CLASS_MAX_LEVEL = %d;" % CF.MAX_LEVEL in rule and "CLASS_BWT = 0xFFu;" in rule and "CLASS_COSTS = FILTER_CANDS + 1;" in rule
    assert "{%s}" % ", ".join(str(v) for v in CF.VERSIONS) in rule
    assert "#include <hip" not in rule and "__global__" not in rule      # host code and nothing else
    probe = open(os.path.join(ROOT, "gpu-lossless-compression_amd", "csrc", "choose.hip")).read()
    assert "k_ch_probe16" in probe and "CH16_MAX_LEN = 65536" in probe


def test_argument_validation_without_gpu(glc):
    L = glc._ct()
    HANDLE = glc.CUDPP_ERROR_INVALID_HANDLE
    d = C.c_uint(77)
    for h in (0, glc.CUDPP_INVALID_HANDLE):
        for level in (0, 1, 5, 6):
            assert L.glcPlanSetContainerChooseFilters(h, level) == HANDLE
        assert L.glcPlanGetContainerChooseFilters(h, C.byref(d)) == HANDLE and L.glcPlanGetContainerChooseFilters(h, None) == HANDLE
    assert d.value == 77


# --- the classes -------------------------------------------------------------------------------------------------------
def test_the_classes_of_the_twelve_inputs_at_1_mib():
    inputs = F.inputs(1 << 20)
    assert set(inputs) == set(TYPED) | {"text", "noise", "zeros", "scattered"}
    for name, v in inputs.items():
        k = _keys(v)
        want = TYPED.get(name, CF.BWT if name == "text" else 0)
        assert k[2:] == [want] * 4, (name, k)
        assert k[0] == k[1] == (CF.BWT if CM.is_bwt(v.size, CM.stats(v)) else 0)       # below level 2: the bigram rule alone
    assert _keys(inputs["ts64"])[0] == _keys(inputs["quant16"])[0] == CF.BWT            # what the bigram rule alone misroutes


def test_the_classes_of_the_8_bit_images():
    for n in (1 << 20, 1 << 16, 8192):
        grey, rgb = _keys(BI.grey8(n, 721)), _keys(BI.rgb8(n, 427))
        assert grey[5] == rgb[5] == 1, n                           # level 5: bytes
        # level 4, recorded: the greyscale image passes for 16-bit elements (its two planes are the byte predictor's at lag 2 but
        # for the borrows, as byte_rule.h says of two channels), the RGB image for nothing typed and, by the bigram rule, order-0
        assert grey[2:5] == [2, 2, 2] and rgb[2:5] == [0, 0, 0], n
    short = BI.grey8(2047, 100)
    assert _keys(short) == [0] * 6 and CF.key(short, 5) == 0       # below MIN_LEN nothing is typed, whatever the costs say


def test_key_from_walks_the_margins():
    p, on = 33 << 30, 1 << 35                                      # 33 * 2^35 = 32 * (33 * 2^30): exactly on the margin
    flat, bwt = (0, 0, 0, 2046), (2046 * 2045, 2046 * 2045, 1023 * 2045, 2046)
    assert CF.key_from(2, 4096, [p, p, p, p, on, p, p, CF.B.NO_COST], flat) == 0
    assert CF.key_from(2, 4096, [p, p, p, p, on - 1, p, p, CF.B.NO_COST], bwt) == 4
    assert CF.key_from(1, 4096, [p, p, p, p, on - 1, p, p, CF.B.NO_COST], bwt) == CF.BWT
    assert CF.key_from(4, 4096, [p] * 7 + [1], bwt) == CF.BWT and CF.key_from(5, 4096, [p] * 7 + [on - 1], bwt) == 1
    assert CF.key_from(5, 4096, [p, p, on - 1, p, p, p, p, on - 1], bwt) == 2 and CF.key_from(5, 4096, [p, p, on - 1, p, p, p, p, on - 2], bwt) == 1


# --- the containers ------------------------------------------------------------------------------------------------------
def _small():
    s = PICKS["small"]
    return CI.mixed(s["block_len"], s["counts"], s["tail"]), s


@pytest.mark.parametrize("level", range(6))
def test_the_mixed_input_round_trips_at_every_level(level):
    x, s = _small()
    n, rows = s["block_len"], s["rows"]
    forced = None
    if level >= 4:
        assert s["level%d" % level]["keys"] == [k for *_, k in CF.plan(x, n, rows, level)]
        forced = s["level%d" % level]["choose"]
    c, frames, picks = CF.write(x, n, rows, level, with_plan=True, picks=forced)
    assert struct.unpack("<HHII", c[4:16]) == (CF.VERSIONS[level], 0, n, 0)
    assert np.array_equal(CF.read(c, level), x)                   # the existing reader of the level's version
    assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(nb, bl) for _, nb, bl, _ in frames]
    assert CF.last_choice(frames)[2] == len(frames) and sum(CF.last_choice(frames)[:2]) == 25
    assert CF.reports(picks, level)[0][7] == len(frames)
    if level == 0:
        assert c == CM.write(x, n, rows) and CF.last_choice(frames) == CM.last_choice(x, n, rows)
    if level >= 2:                                               # the frame words: a BWT frame's is 0
        words = F.frame_words(c)
        assert all(w == 0 for w, (*_, k) in zip(words, frames) if k == CF.BWT) and any(words)
    if level == 5:
        assert CF.reports(picks, level)[3] == (0, 1, 1)           # the image's frame: the byte predictor at its row stride


def test_at_64_kib_levels_4_and_5_beat_choose_bwt_and_filter_auto():
    n, rows = PICKS["block_len"], PICKS["rows"]
    x = CI.mixed(n)
    assert x.size == PICKS["bytes"]
    choose, bwt = len(CM.write(x, n, rows)), len(M.write(x, n, rows, 0, 0))
    assert choose == PICKS["choose_bytes"]
    for level, model in ((4, CF.Q), (5, CF.B)):
        fx = PICKS["level%d" % level]
        c, frames, _ = CF.write(x, n, rows, level, with_plan=True, picks=fx["choose"])
        assert [k for *_, k in frames] == fx["keys"]
        order0 = len(model.write(x, n, rows, [tuple(p) for p in fx["order0"]]))
        print("level %d: choose-filters %d, CHOOSE %d, BWT %d, filter-auto %d bytes; %d frames" % (level, len(c), choose, bwt, order0, len(frames)))
        assert (len(c), order0) == (fx["choose_bytes"], fx["order0_bytes"])      # the when-table's figures
        assert len(c) < choose and len(c) < bwt and len(c) < order0
        assert np.array_equal(CF.read(c, level), x)


@pytest.mark.parametrize("kind,elem", [("float32", 4), ("ts64", 8)])
def test_on_a_uniform_input_the_container_is_the_order_0_plans(kind, elem):
    n, rows = 4096, 4
    x = CI.uniform(kind, 8 * n + 300)
    for level in (2, 3, 4, 5):
        frames = CF.plan(x, n, rows, level)
        assert [(nb, k) for _, nb, _, k in frames] == [(4, elem), (4, elem), (1, 0)]
        picks = CF.picks_of(x, n, rows, level, frames)
        c = CF.write(x, n, rows, level, picks=picks)
        assert c == CF.order0_write(x, n, rows, level), level      # the composition costs nothing where it has nothing to decide
    if kind == "float32":                                        # level 1: the bigram rule sends these blocks to the order-0 codec
        assert CF.write(x, n, rows, 1) == CF.order0_write(x, n, rows, 1)


# --- the rule of class_rule.h and the setter's walk ----------------------------------------------------------------------
def test_class_rule_and_the_setter_under_the_host_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc for tools/class_rule_check.cpp")
    exe = str(tmp_path / "class_rule_check")
    flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc] + flags + [os.path.join(ROOT, "tools", "class_rule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "class_rule_check: ok, " in r.stdout, r.stdout[-2000:] + r.stderr
    cases = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert len(cases) == 6 * 11
    for _, name, level, L, *rest in cases:
        v = [int(t) for t in rest]
        assert CF.key_from(int(level), int(L), v[:8], tuple(v[8:12])) == v[12], (name, level)
    assert {c[-1] for c in cases} == {"0", "1", "2", "4", "8", "255"}
