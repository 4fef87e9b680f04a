"""The CHOOSE codec of the BWT container on the MI355X (-m gpu): the device, host-pointer and file entry points write the bytes of
the Python model (tests/choose_model.py) with pipelining off and on -- at n = 8192 with rows = 8 over a stream whose super-frames
come out all BWT, all order-0, alternating block by block and in two runs, with a tail of 1235 bytes; at n = 4099 (misaligned
blocks); at n = 70000 with rows = 4 (a tail long enough to go to the BWT codec) -- glcContainerLastChoice gives the model's
counts, the size stays within the bound, a default plan and an order-0 plan decode the stream, range reads across frame seams
give the input's slices, compressing twice gives the same bytes, CHOOSE then codec 0 or 1 gives the old bytes again, the refused setter
combinations leave the settings as they were, a capacity failure reports the needed length, the golden fixture decodes."""
import os
import struct

import numpy as np
import pytest

import choose_inputs as CI
import choose_model as CM
import container_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL = 2
CHOOSE = CM.CODEC_CHOOSE                                        # GLC_CONTAINER_CODEC_CHOOSE
# n -> (rows, layout, tail, glcContainerLastChoice)
CASES = {8192: (8, CI.EIGHT, ("logs", 1235), CI.EIGHT_WANT),
         4099: (8, ("text", "zipf") * 4 + ("logs",) * 3 + ("zeros90",) * 2, ("zipf", 777), (7, 7, 11)),
         70000: (4, ("text", "zipf", "zipf", "logs", "noise", "text"), ("text", 30000), (4, 3, 6))}


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


def _case(n):
    """(input, the model's container), made once"""
    if n not in _MADE:
        rows, layout, tail, _ = CASES[n]
        x = CI.stream(n, layout, tail)
        _MADE[n] = (x, CM.write(x, n, rows))
    return _MADE[n]


def _plan(glc, ctx, n, rows, codec=CHOOSE, pipelined=False):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows)
    plan.set_pipelining(pipelined)
    glc.container_set_codec(plan, codec)
    return plan


def _frames(c):
    return [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]]


def test_the_cases_are_what_they_say():
    x, want = _case(8192)
    assert _frames(want) == [(8, 8192), (8, 8192)] + [(1, 8192)] * 8 + [(2, 8192), (2, 8192), (1, 1235)]
    assert _frames(_case(4099)[1]) == [(1, 4099)] * 8 + [(3, 4099), (2, 4099), (1, 777)]
    assert _frames(_case(70000)[1]) == [(1, 70000), (2, 70000), (1, 70000), (1, 70000), (1, 70000), (1, 30000)]
    for n, (rows, _, _, choice) in CASES.items():
        x, want = _case(n)
        assert CM.last_choice(x, n, rows) == choice and struct.unpack("<HHII", want[4:16]) == (3, 0, n, 0)
        y, kinds = M.read(want, with_kinds=True, max_version=3)
        assert np.array_equal(y, x) and {M.HUFF, M.HUFF0} <= set(kinds)
    assert M.RAW in M.read(_case(8192)[1], with_kinds=True, max_version=3)[1]


@pytest.mark.parametrize("n", sorted(CASES))
@pytest.mark.parametrize("pipelined", [False, True])
def test_all_entry_points_equal_the_model_and_round_trip(glc, ctx, cuda, tmp_path, n, pipelined):
    rows, _, _, choice = CASES[n]
    x, want = _case(n)
    with _plan(glc, ctx, n, rows, pipelined=pipelined) as plan:
        assert glc.container_get_codec(plan) == glc.CONTAINER_CODEC_CHOOSE
        c = glc.container_compress(plan, _gpu(x))
        assert _host(c).tobytes() == want
        assert glc.container_last_choice(plan) == choice
        assert c.numel() <= glc.container_bound(x.size, n)
        assert np.array_equal(_host(glc.container_decompress(plan, c)), x)
        assert glc.container_last_error(plan) == (0, -1, -1)
        ch = glc.container_compress_host(plan, x)
        assert ch.tobytes() == want and glc.container_last_choice(plan) == choice
        assert np.array_equal(glc.container_decompress_host(plan, ch), x)
        src, dst, back = tmp_path / "in.bin", tmp_path / "out.glcb", tmp_path / "back.bin"
        x.tofile(src)
        glc.container_compress_file(plan, str(src), str(dst))
        assert dst.read_bytes() == want
        glc.container_decompress_file(plan, str(dst), str(back))
        assert back.read_bytes() == x.tobytes()
        for L in (0, 1, n):
            y = x[:L]
            c = glc.container_compress(plan, _gpu(y))
            assert _host(c).tobytes() == CM.write(y, n, rows)
            assert glc.container_last_choice(plan) == CM.last_choice(y, n, rows)
            assert np.array_equal(_host(glc.container_decompress(plan, c)), y)
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want       # twice: the same bytes, the plan's scratch reused
    # any plan reads the stream: a default one and an order-0 one, of other rows
    d = _gpu(np.frombuffer(want, np.uint8))
    for codec, r in ((0, 3), (1, rows)):
        with _plan(glc, ctx, n, r, codec=codec, pipelined=pipelined) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, d)), x)
            assert np.array_equal(glc.container_decompress_host(plan, np.frombuffer(want, np.uint8)), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


def test_range_reads_across_frame_seams(glc, ctx, cuda, tmp_path):
    n, rows = 8192, 8
    x, want = _case(n)
    path = tmp_path / "c.glcb"
    path.write_bytes(want)
    host = np.frombuffer(want, np.uint8)
    d = _gpu(host)
    # inside the all-BWT frame; across its seam to the all-order-0 frame; over five one-block frames; across the two runs of the
    # last super-frame and into the tail; everything; nothing; the last two bytes
    ranges = [(40000, 100), (8 * n - 5000, 10000), (16 * n + 100, 4 * n + 50), (26 * n - 1, 2 * n + 100), (0, x.size), (x.size, 0),
              (x.size - 2, 2)]
    for codec in (0, CHOOSE):                                   # a default plan reads it like the plan that wrote it
        with _plan(glc, ctx, n, rows, codec=codec) as plan:
            with glc.container_index(plan, d) as ix:
                assert ix.info() == (x.size, n, len(_frames(want)), 3, 0, 0)
                for off, cnt in ranges:
                    assert np.array_equal(_host(glc.container_read_range(plan, ix, d, off, cnt)), x[off:off + cnt]), (off, cnt)
                assert glc.container_last_range_stats(plan)[:2] == (1, 1)          # (the last range: the tail's frame alone)
            with glc.container_index_host(plan, host) as ix:
                for off, cnt in ranges[:4]:
                    assert np.array_equal(glc.container_read_range_host(plan, ix, host, off, cnt), x[off:off + cnt]), (off, cnt)
            with glc.container_index_file(plan, str(path)) as ix:
                off, cnt = ranges[3]
                assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), off, cnt), x[off:off + cnt])


def test_choose_then_codec_0_or_1_gives_the_old_bytes(glc, ctx, cuda):
    n, rows = 8192, 8
    x, want = _case(n)
    with _plan(glc, ctx, n, rows) as plan:
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == want
        for codec in (0, 1, CHOOSE, 1, 0):
            glc.container_set_codec(plan, codec)
            got = _host(glc.container_compress(plan, _gpu(x))).tobytes()
            assert got == (want if codec == CHOOSE else M.write(x, n, rows, 0, codec)), codec
            nblk = (x.size + n - 1) // n
            if codec != CHOOSE:                                      # every block to the plan's codec, one frame per super-frame
                assert glc.container_last_choice(plan) == ((nblk, 0, 5) if codec == 0 else (0, nblk, 5))


def test_setter_rules(glc, ctx, cuda):
    def refused(plan, call, *a):
        with pytest.raises(glc.CudppError) as e:
            call(plan, *a)
        return e.value.code == ILLEGAL

    def state(plan):
        return (glc.container_get_codec(plan), glc.container_get_shuffle(plan), glc.container_get_delta(plan), glc.container_get_sparse(plan),
                glc.container_get_runs(plan), glc.container_get_ans(plan), glc.container_get_auto(plan))

    modes = (glc.container_set_sparse, glc.container_set_runs, glc.container_set_ans, glc.container_set_auto)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 8192, rows=2) as plan:
        assert glc.container_last_choice(plan) == (0, 0, 0)
        for elem in (2, 4, 8):                                  # refused while the shuffle is on, with or without the delta
            for delta in (0, 1):
                glc.container_set_shuffle(plan, elem)
                glc.container_set_delta(plan, delta)
                was = state(plan)
                assert refused(plan, glc.container_set_codec, CHOOSE) and state(plan) == was
        glc.container_set_shuffle(plan, 0)
        for codec, mode in ((0, glc.container_set_runs), (1, glc.container_set_sparse), (1, glc.container_set_ans), (1, glc.container_set_auto)):
            glc.container_set_codec(plan, codec)                # otherwise it clears the mode, as every codec change does
            mode(plan, 1)
            glc.container_set_codec(plan, CHOOSE)
            assert state(plan) == (CHOOSE, 0, 0, 0, 0, 0, 0)
        was = state(plan)
        for elem in (2, 4, 8):                                  # while it is the codec: no filter ...
            assert refused(plan, glc.container_set_shuffle, elem) and state(plan) == was
        assert refused(plan, glc.container_set_delta, 1) and state(plan) == was
        for mode in modes:                                      # ... and no mode
            assert refused(plan, mode, 1) and state(plan) == was
            mode(plan, 0)                                       # off is always legal
            assert state(plan) == was
        for elem in (0, 1):
            glc.container_set_shuffle(plan, elem)
        glc.container_set_delta(plan, 0)
        assert state(plan) == was
        for bad in (2, 3, 5, 7, 255, 1 << 31):
            assert refused(plan, glc.container_set_codec, bad) and state(plan) == was
        glc.container_set_codec(plan, 1)
        glc.container_set_auto(plan, 1)
        assert state(plan) == (1, 0, 0, 0, 0, 0, 1)
        glc.container_set_codec(plan, 0)
        glc.container_set_shuffle(plan, 4)
        assert state(plan) == (0, 4, 0, 0, 0, 0, 0)


def test_capacity_failure_reports_the_needed_length(glc, ctx, cuda):
    import torch
    n, rows = 8192, 8
    x, want = _case(n)
    need = len(want)
    with _plan(glc, ctx, n, rows) as plan:
        for cap in (need - 1, need // 2, 100):
            out = torch.full((cap + 256,), 0xCD, dtype=torch.uint8, device=cuda)
            d_len = torch.zeros(1, dtype=torch.int64, device=cuda)
            rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), cap, d_len.data_ptr())
            assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
            assert bool((out[cap:] == 0xCD).all()), cap
        c = glc.container_compress(plan, _gpu(x), cap=need)
        assert c.numel() == need and _host(c).tobytes() == want
        with pytest.raises(glc.CudppError):                     # the host form: its sink is full
            glc.container_compress_host(plan, x, cap=need - 1)
        assert glc.container_last_error(plan)[0] == 6
        assert glc.container_compress_host(plan, x, cap=need).tobytes() == want


def test_gpu_reads_the_golden_fixture(glc, ctx, cuda):
    gold = open(os.path.join(GOLDEN, "container_v3_choose.bin"), "rb").read()
    x, kinds = M.read(gold, with_kinds=True, max_version=3)
    assert set(kinds) == {0, 1, 2}
    g = np.frombuffer(gold, np.uint8)
    for n, rows, codec, pipelined in ((4096, 4, CHOOSE, False), (4096, 1, 0, True), (8192, 2, 1, False)):
        with _plan(glc, ctx, n, rows, codec=codec, pipelined=pipelined) as plan:
            assert np.array_equal(_host(glc.container_decompress(plan, _gpu(g))), x)
            assert np.array_equal(glc.container_decompress_host(plan, g), x)
            assert glc.container_last_error(plan) == (0, -1, -1)
    with _plan(glc, ctx, 4096, 4) as plan:                      # and the GPU writer makes the fixture
        assert _host(glc.container_compress(plan, _gpu(x))).tobytes() == gold
