"""The CHOOSE codec with filters (glcPlanSetContainerChooseFilters) on the MI355X (-m gpu), at n = 8192 and rows = 8 on the mixed
input of tests/choose_filters_inputs.py -- five blocks each of text, float32, int64 timestamps and an 8-bit image, four of noise,
and a tail of 1235 bytes -- at levels 1 to 5: the device, host-pointer and file entry points write the bytes of the Python model
(tests/choose_filters_model.py; at levels 4 and 5 the frames' filters are the fixture's, tests/golden/choose_filters_picks.json --
the model's grid rule needs most of a minute for them -- while the frames are cut by the model's classes in the test), twice; a plan
with the setting and an order-0 plan with the matching existing settings decode the stream, a default plan refuses it; the index
and range reads across a BWT / order-0 seam; the reports; level 0 after level 5 gives today's CHOOSE bytes; the setter's refusals
and the reset on a codec change; pipelined plans of 1 and 4 rows write what the plain plans write."""
import json
import os
import struct

import numpy as np
import pytest

import choose_filters_inputs as CI
import choose_filters_model as CF
import choose_model as CM
import container_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICKS = json.load(open(os.path.join(ROOT, "tests", "golden", "choose_filters_picks.json")))["small"]
N, ROWS = PICKS["block_len"], PICKS["rows"]
CHOOSE = CM.CODEC_CHOOSE
ILLEGAL = 2
LEVELS = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


_MADE = {}


def _x():
    if "x" not in _MADE:
        _MADE["x"] = CI.mixed(N, PICKS["counts"], PICKS["tail"])
    return _MADE["x"]


def _case(level):
    """(the model's container, its frames, its picks), made once"""
    if level not in _MADE:
        forced = None
        if level >= 4:
            fx = PICKS["level%d" % level]
            assert fx["keys"] == [k for *_, k in CF.plan(_x(), N, ROWS, level)]
            forced = fx["choose"]
        _MADE[level] = CF.write(_x(), N, ROWS, level, with_plan=True, picks=forced)
    return _MADE[level]


def _plan(glc, ctx, level, rows=ROWS, pipelined=False):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, CHOOSE)
    glc.container_set_choose_filters(plan, level)
    return plan


def _order0_plan(glc, ctx, level, rows=3):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=rows)
    glc.container_set_codec(plan, 1)
    glc.container_set_auto(plan, 1)
    for lv, setter in ((2, glc.container_set_filter_auto), (3, glc.container_set_filter_lag), (4, glc.container_set_filter_grid),
                       (5, glc.container_set_filter_byte)):
        if level >= lv:
            setter(plan, 1)
    return plan


def _reports(glc, plan):
    return (glc.container_last_filters(plan), glc.container_last_lag_filters(plan), glc.container_last_grid_filters(plan),
            glc.container_last_byte_filters(plan))


def test_the_case_is_what_it_says():
    """every class comes up, the image is typed with e = 2 below level 5 and with e = 1 at it, and every level's stream is its
    version's and reads back through that version's model reader"""
    x = _x()
    for level in LEVELS:
        c, frames, picks = _case(level)
        assert struct.unpack("<HHII", c[4:16]) == (CF.VERSIONS[level], 0, N, 0)
        assert np.array_equal(CF.read(c, level), x)
        keys = [k for *_, k in frames]
        assert keys[0] == CF.BWT and keys[-1] == 0 and frames[-1][1:3] == (1, PICKS["tail"])
        assert set(keys) == ({CF.BWT, 0} if level == 1 else {CF.BWT, 0, 4, 8, 2 if level < 5 else 1})


@pytest.mark.parametrize("level", LEVELS)
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, level):
    x = _x()
    want, frames, picks = _case(level)
    with _plan(glc, ctx, level) as plan:
        assert glc.container_get_choose_filters(plan) == level and glc.container_get_codec(plan) == CHOOSE
        assert (glc.container_get_auto(plan), glc.container_get_filter_auto(plan), glc.container_get_filter_byte(plan)) == (0, 0, 0)
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert glc.container_last_choice(plan) == CF.last_choice(frames)
        assert _reports(glc, plan) == CF.reports(picks, level)
        assert c.numel() <= glc.container_bound(x.size, N)
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        assert glc.container_last_error(plan) == (0, -1, -1)
        ch = glc.container_compress_host(plan, x)
        assert ch.tobytes() == want and glc.container_last_choice(plan) == CF.last_choice(frames)
        assert np.array_equal(glc.container_decompress_host(plan, ch), x)
        src, dst, back = tmp_path / "in.bin", tmp_path / "out.glcb", tmp_path / "back.bin"
        x.tofile(src)
        glc.container_compress_file(plan, str(src), str(dst))
        assert dst.read_bytes() == want
        glc.container_decompress_file(plan, str(dst), str(back))
        assert back.read_bytes() == x.tobytes()
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # twice: the same bytes, the plan's scratch reused
        assert _reports(glc, plan) == CF.reports(picks, level)
    # no reader changed: the order-0 plan with the level's settings reads the stream; a default plan refuses its version as ever
    d = _gpu(np.frombuffer(want, np.uint8))
    with _order0_plan(glc, ctx, level) as plan:
        assert np.array_equal(_host(glc.container_decompress(plan, d)), x)
        assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(want, np.uint8)), x)
        assert glc.container_last_error(plan) == (0, -1, -1)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plan:
        with pytest.raises(glc.CudppError):
            glc.container_decompress(plan, d)
        assert glc.container_last_error(plan) == (1, -1, -1)
        glc.container_set_codec(plan, CHOOSE)                  # CHOOSE at level 0 is a version-3 reader
        with pytest.raises(glc.CudppError):
            glc.container_decompress(plan, d)
        assert glc.container_last_error(plan) == (1, -1, -1)


@pytest.mark.parametrize("level", LEVELS)
def test_index_and_range_reads_across_the_seams(glc, ctx, cuda, tmp_path, level):
    x = _x()
    want, frames, _ = _case(level)
    host = np.frombuffer(want, np.uint8)
    d = _gpu(host)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    # across the seam between the BWT frame of the text and the order-0 frame behind it; across a super-frame's edge; through the
    # typed frames into the tail; everything; nothing; the last two bytes
    seam = frames[1][0]
    assert frames[0][3] == CF.BWT and frames[1][3] != CF.BWT
    ranges = [(seam - 5000, 10000), (8 * N - 100, 300), (9 * N + 7, 12 * N), (23 * N + 5, N + 1000), (0, x.size), (x.size, 0), (x.size - 2, 2)]
    with _plan(glc, ctx, level) as plan:
        with glc.container_index(plan, d) as ix:
            assert ix.info()[:4] == (x.size, N, len(frames), CF.VERSIONS[level])
            for off, cnt in ranges:
                assert np.array_equal(_host(glc.container_read_range(plan, ix, d, off, cnt)), x[off:off + cnt]), (off, cnt)
        with glc.container_index_host(plan, host) as ix:
            for off, cnt in ranges[:3]:
                assert np.array_equal(glc.container_read_range_host(plan, ix, host, off, cnt), x[off:off + cnt]), (off, cnt)
        with glc.container_index_file(plan, str(path)) as ix:
            off, cnt = ranges[0]
            assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])
    with _order0_plan(glc, ctx, level) as plan:
        with glc.container_index(plan, d) as ix:
            off, cnt = ranges[0]
            assert np.array_equal(_host(glc.container_read_range(plan, ix, d, off, cnt)), x[off:off + cnt])


def test_level_0_after_level_5_gives_todays_choose_bytes(glc, ctx, cuda):
    x = _x()
    today = CM.write(x, N, ROWS)
    with _plan(glc, ctx, 5) as plan:
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _case(5)[0]
        glc.container_set_choose_filters(plan, 0)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == today
        assert glc.container_last_choice(plan) == CM.last_choice(x, N, ROWS)
        assert _reports(glc, plan) == CF.reports([None] * CM.last_choice(x, N, ROWS)[2], 0)
        for level in (3, 1):
            glc.container_set_choose_filters(plan, level)
            assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == _case(level)[0]
        glc.container_set_codec(plan, CHOOSE)                  # the codec call resets the level
        assert glc.container_get_choose_filters(plan) == 0
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == today
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS) as plan:   # and a plan that never had a level
        glc.container_set_codec(plan, CHOOSE)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == today


def test_setter_rules(glc, ctx, cuda):
    def refused(plan, call, *a):
        with pytest.raises(glc.CudppError) as e:
            call(plan, *a)
        return e.value.code == ILLEGAL

    def state(plan):
        return (glc.container_get_codec(plan), glc.container_get_choose_filters(plan), glc.container_get_shuffle(plan), glc.container_get_auto(plan),
                glc.container_get_filter_auto(plan), glc.container_get_filter_lag(plan), glc.container_get_filter_grid(plan),
                glc.container_get_filter_byte(plan))

    with glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=2) as plan:
        assert state(plan) == (0, 0, 0, 0, 0, 0, 0, 0)
        for codec in (0, 1):                                    # legal only while the codec is CHOOSE, level 0 included
            glc.container_set_codec(plan, codec)
            was = state(plan)
            for level in range(0, 7):
                assert refused(plan, glc.container_set_choose_filters, level) and state(plan) == was
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        glc.container_set_filter_auto(plan, 1)
        assert refused(plan, glc.container_set_choose_filters, 2) and state(plan) == (1, 0, 0, 1, 1, 0, 0, 0)
        glc.container_set_codec(plan, CHOOSE)
        for level in range(0, 6):
            glc.container_set_choose_filters(plan, level)
            assert state(plan) == (CHOOSE, level, 0, 0, 0, 0, 0, 0)
            was = state(plan)
            for bad in (6, 7, 255, 1 << 31):
                assert refused(plan, glc.container_set_choose_filters, bad) and state(plan) == was
            # the refusals under CHOOSE answer as they do without a level
            for call, arg in ((glc.container_set_shuffle, 4), (glc.container_set_auto, 1), (glc.container_set_sparse, 1), (glc.container_set_ans, 1),
                              (glc.container_set_runs, 1), (glc.container_set_filter_auto, 1), (glc.container_set_filter_lag, 1)):
                assert refused(plan, call, arg) and state(plan) == was
        for codec in (CHOOSE, 0, 1):                            # every codec call puts the level back to 0
            glc.container_set_codec(plan, CHOOSE)
            glc.container_set_choose_filters(plan, 5)
            glc.container_set_codec(plan, codec)
            assert state(plan) == (codec, 0, 0, 0, 0, 0, 0, 0)
        glc.container_set_codec(plan, CHOOSE)
        glc.container_set_choose_filters(plan, 4)
        assert refused(plan, glc.container_set_codec, 3) and state(plan) == (CHOOSE, 4, 0, 0, 0, 0, 0, 0)      # a refused codec changes nothing


@pytest.mark.parametrize("rows", [1, 4])
def test_pipelined_plans_write_what_the_plain_plans_write(glc, ctx, cuda, rows):
    x = _x()
    d = _gpu(x)
    for level in LEVELS:
        with _plan(glc, ctx, level, rows=rows) as plain, _plan(glc, ctx, level, rows=rows, pipelined=True) as piped:
            want = _host(glc.container_compress(plain, d)).tobytes()
            if rows == ROWS // 2 and level <= 3:                 # (the model's rule is quick up to level 3)
                assert want == CF.write(x, N, rows, level)
            for _ in range(2):
                got = glc.container_compress(piped, d)
                assert _host(got).tobytes() == want
            assert glc.container_last_choice(piped) == glc.container_last_choice(plain)
            assert _reports(glc, piped) == _reports(glc, plain)
            assert np.array_equal(_host(glc.container_decompress(piped, got)), x)
