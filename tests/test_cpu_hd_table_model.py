"""The device table algorithm (tests/hd_table_model.py: rank sort, rank-merged package-merge, multiplicity push-down,
canonical codes) equals glcHdBuildTable on every histogram the GPU table test uses -- the formulation k_hd_table runs,
pinned on the CPU."""
import os

import numpy as np
import pytest

import hd_table_model as M
import test_hd

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cuhd_gold.npz"))


def named_histograms():
    out = [(name, np.bincount(data, minlength=256).astype(np.uint64)) for name, data in test_hd.CASES]
    for name in (str(c) for c in GOLD["cases"]):
        h = GOLD[name + "_hist"] if name + "_hist" in GOLD.files else np.bincount(GOLD[name + "_symbols"], minlength=256)
        out.append(("gold_" + name, np.asarray(h, dtype=np.uint64)))
    out.append(("fibonacci_40", M.fibonacci_hist(40)))
    out.append(("all_256_equal", np.full(256, 7, dtype=np.uint64)))
    return out


NAMED = named_histograms()


@pytest.mark.parametrize("name,hist", NAMED, ids=[n for n, _ in NAMED])
def test_model_equals_host_builder_named(glc, name, hist):
    lens, codes = M.build_table(hist)
    want_l, want_c = glc.hd_build_table(hist)
    assert np.array_equal(lens, want_l) and np.array_equal(codes, want_c)


def test_model_equals_host_builder_random(glc):
    hs = M.random_histograms()
    assert len(hs) >= 2000
    limited = 0
    for i, h in enumerate(hs):
        lens, codes = M.build_table(h)
        want_l, want_c = glc.hd_build_table(h)
        assert np.array_equal(lens, want_l), i
        assert np.array_equal(codes, want_c), i
        limited += int(lens.max() == M.MAX_LEN)
    assert limited > 50                            # the corpus reaches the length limit


def test_model_edge_cases():
    lens, codes = M.build_table(np.zeros(256, dtype=np.uint64))
    assert not lens.any() and not codes.any()
    h = np.zeros(256, dtype=np.uint64)
    h[77] = 5
    lens, codes = M.build_table(h)
    assert lens[77] == 1 and codes[77] == 0 and lens.sum() == 1
    t = M.decoder_table(lens, codes).reshape(2048, 2)
    assert (t[:1024] == (1, 77)).all() and not t[1024:].any()
