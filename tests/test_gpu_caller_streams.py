"""Work is queued on the caller's stream, and enqueue-only entries only enqueue (-m gpu).

include/glc_container.h promises "work is queued on the plan's stream", include/cudpp.h has glcPlanSetStream, and every
*Segments / *Device / *RangeDevice entry takes a stream and says it only enqueues on it.  The other tests pass the null stream
and then wait for the whole device, where a launch, memset or copy that forgot its stream argument, or a host wait inside an
enqueue-only call, cannot be seen.  Here every call runs through tests/stream_rig.py: on a non-blocking stream S, behind a
gate that delivers the real input late, with the null stream blocked for the duration, and the result is compared with the
CPU model or the oracle -- the functions the entry's own tests use.  The control test shows that the rig sees a stage on the
wrong stream."""
import contextlib
import functools
import zlib

import numpy as np
import pytest

import ans_model
import auto_model
import byte_delta_model as BD
import choose_model
import container_model as M
import datagen
import dec_huff_inputs as D
import dedup_model
import filter_auto_model as F
import filter_byte_model as FB
import filter_grid_model as FQ
import filter_lag_model as FL
import grid_model
import lag_model
import oracle_lib as O
import runs_model
import small_container as S
import sparse_model
import stream_rig as R
import tier_batches as T

pytestmark = pytest.mark.gpu
N1M = 1 << 20
serial_and_pipelined = pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])


@pytest.fixture
def st(cuda):
    return R.independent_stream()


@contextlib.contextmanager
def _plan_on(glc, stream, algorithm, n, rows=1, pipelined=False):
    """a plan set to `stream`; the device is idle before the plan goes"""
    import torch
    with glc.Cudpp() as ctx, glc.Plan(ctx, algorithm, n, rows=rows) as plan:
        plan.set_stream(glc._stream_ptr(stream))
        if pipelined:
            plan.set_pipelining(True)
        try:
            yield plan
        finally:
            torch.cuda.synchronize()


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


# --- the plan's batch calls: the oracle's streams ---------------------------------------------------------------------------------
def _strided_host(glc, wants, n):
    """the oracle's streams of blocks of n bytes as glcDecompressBatch takes them: bwt_index, hist, offsets, words (int32 arrays)"""
    nsub, stride = (n + D.SUB - 1) // D.SUB, glc.compressed_stride_words(n)
    words = np.zeros(len(wants) * stride, dtype=np.uint32)
    offsets = np.zeros(len(wants) * nsub, dtype=np.uint32)
    for b, r in enumerate(wants):
        words[b * stride:b * stride + r["size"]] = r["words"]
        offsets[b * nsub:b * nsub + r["offsets"].size] = r["offsets"]
    idx = np.asarray([r.get("bwt_index", 0) for r in wants], np.int32)
    return [idx, _i32(np.concatenate([r["hist"] for r in wants])), _i32(offsets), _i32(words)]


def _comp(glc, n, idx, hist, offsets, words):
    return dict(bwt_index=idx, hist=hist, offsets=offsets, words=words, nsub=(n + D.SUB - 1) // D.SUB, stride=glc.compressed_stride_words(n))


def _assert_streams(got, wants, what, index=True):
    stride, nsub = got["stride"], got["nsub"]
    for i, w in enumerate(wants):
        size = int(got["size"][i])
        assert size == w["size"] and (not index or int(got["bwt_index"][i]) == w["bwt_index"]), "%s: index / size of block %d" % (what, i)
        assert np.array_equal(got["words"][i * stride:i * stride + size].view(np.uint32), w["words"]), "%s: stream of block %d" % (what, i)
        assert np.array_equal(got["hist"][i * 256:(i + 1) * 256].view(np.uint32), w["hist"]), "%s: histogram of block %d" % (what, i)
        assert np.array_equal(got["offsets"][i * nsub:i * nsub + w["offsets"].size].view(np.uint32), w["offsets"]), "%s: offsets of block %d" % (what, i)


def _round_trip_on(glc, stream, plan, n, blocks_a, wants_a, blocks_b, wants_b, group, what):
    """glcCompressBatch and glcDecompressBatch through the rig, each against the oracle"""
    nblk = len(blocks_b)

    def compress(d_in):
        out = glc.compress_batch(plan, d_in, n, nblk)
        plan.synchronize()
        return out

    def decompress(*d):
        back = glc.decompress_batch(plan, _comp(glc, n, *d), n, nblk)
        plan.synchronize()
        return back

    got = R.behind_the_gate(stream, compress, [np.concatenate(blocks_a)], [np.concatenate(blocks_b)], group)
    stats = plan.last_sort_stats(), plan.last_sort_resumed()
    _assert_streams(got, wants_b, what)
    back = R.behind_the_gate(stream, decompress, _strided_host(glc, wants_a, n), _strided_host(glc, wants_b, n), group)
    assert np.array_equal(back, np.concatenate(blocks_b)), "%s: glcDecompressBatch" % what
    return stats


@functools.lru_cache(maxsize=None)
def _one_block(kind):
    """(B, the oracle's stream, A, its stream): test_gpu_call_history.py's 1203-byte text block and 70001-byte random block; A is
    B backwards"""
    x = datagen.text_bytes(1203, seed=1203) if kind == "text_1203" else np.random.default_rng(70001).integers(0, 256, 70001, dtype=np.uint8)
    a = np.ascontiguousarray(x[::-1])
    return x, O.compress(x), a, O.compress(a)


@serial_and_pipelined
@pytest.mark.parametrize("kind", ["text_1203", "random_70001"])
def test_one_block_on_a_plan_of_64k(glc, st, kind, pipelined):
    x, want, a, want_a = _one_block(kind)
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, max(65536, x.size), 1, pipelined) as plan:    # (a plan takes no block above its n)
        _round_trip_on(glc, st, plan, x.size, [a], [want_a], [x], [want], "small", kind)


@serial_and_pipelined
def test_every_tier_of_the_sorter(glc, st, pipelined):
    """the only input that reaches the `aux` side stream, the periodic tier and the resumed doubling.  A is the same nine blocks
    one place on"""
    blocks, wants = list(T.all_tiers_blocks_1m()), list(T.all_tiers_compressed_1m())
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, N1M, len(blocks), pipelined) as plan:
        stats = _round_trip_on(glc, st, plan, N1M, blocks[1:] + blocks[:1], wants[1:] + wants[:1], blocks, wants, "all_tiers", "all tiers")
        assert stats == (T.ALL_TIERS_STATS, T.ALL_TIERS_RESUMED), stats


@functools.lru_cache(maxsize=None)
def _block_12345():
    x = datagen.text_bytes(12345, seed=12345)
    a = datagen.zipf_bytes(12345, seed=12346)
    return x, a


def test_suffix_array_plan(glc, st):
    import torch
    x, a = _block_12345()
    n = x.size
    with _plan_on(glc, st, glc.CUDPP_SA, n) as plan:
        def call(d_in):
            d_out = torch.zeros(n + 1, dtype=torch.int32, device=d_in.device)
            assert glc.lib().cudppSuffixArray(plan.handle, d_in.data_ptr(), d_out.data_ptr(), n) == glc.CUDPP_SUCCESS
            plan.synchronize()
            return d_out
        got = R.behind_the_gate(st, call, [a], [x]).view(np.uint32)
    assert got[0] == n and np.array_equal(got[1:], O.suffix_array(x))


def test_bwt_plan(glc, st):
    import torch
    x, a = _block_12345()
    n = x.size
    with _plan_on(glc, st, glc.CUDPP_BWT, n) as plan:
        def call(d_in):
            d_out = torch.zeros(n, dtype=torch.uint8, device=d_in.device)
            d_idx = torch.zeros(1, dtype=torch.int32, device=d_in.device)
            assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, 1) == glc.CUDPP_SUCCESS
            plan.synchronize()
            return d_out, d_idx
        got, idx = R.behind_the_gate(st, call, [a], [x])
    want, widx = O.bwt(x)
    assert int(idx[0]) == widx and np.array_equal(got, want)


def test_mtf_plan(glc, st):
    import torch
    x, a = _block_12345()
    n = x.size
    with _plan_on(glc, st, glc.CUDPP_MTF, n) as plan:
        def call(d_in):
            d_out = torch.zeros_like(d_in)
            assert glc.lib().glcMtfBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), n, 1) == glc.CUDPP_SUCCESS
            plan.synchronize()
            return d_out
        got = R.behind_the_gate(st, call, [a], [x])
    assert np.array_equal(got, O.mtf(x))


# --- the stages on their own --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _symbols(name):
    """(blocks of symbols B, the oracle's stream of each, A, its streams): dec_huff_inputs' smallest single blocks and two
    blocks of 4096"""
    if name == "two_of_4096":
        b = D.batch_blocks(4096, 2)
    else:
        b = [D.single_block_cases()[name]]
    a = [np.ascontiguousarray(x[::-1]) for x in b][::-1]
    return b, [D.encode(x) for x in b], a, [D.encode(x) for x in a]


STAGE_CASES = ("size_1", "size_4097", "two_of_4096")


@pytest.mark.parametrize("name", STAGE_CASES)
def test_huffman_encode_stage(glc, st, name):
    b, wants, a, _ = _symbols(name)
    n, nblk = b[0].size, len(b)
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, nblk) as plan:
        def call(d_sym):
            out = glc.huffman_encode_batch(plan, d_sym, n, nblk)
            plan.synchronize()
            return out
        got = R.behind_the_gate(st, call, [np.concatenate(a)], [np.concatenate(b)])
    _assert_streams(got, wants, name, index=False)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_huffman_decode_stage(glc, st, name, mode):
    b, wants, a, wants_a = _symbols(name)
    n, nblk = b[0].size, len(b)
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, nblk) as plan:
        plan.set_huff_decoder(mode)

        def call(*d):
            sym = glc.huffman_decode_batch(plan, _comp(glc, n, *d), n, nblk)
            plan.synchronize()
            return sym
        got = R.behind_the_gate(st, call, _strided_host(glc, wants_a, n), _strided_host(glc, wants, n))
    assert np.array_equal(got, np.concatenate(b)), name


@pytest.mark.parametrize("name", STAGE_CASES)
def test_inverse_mtf_stage(glc, st, name):
    b, _, a, _ = _symbols(name)
    n, nblk = b[0].size, len(b)
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, nblk) as plan:
        def call(d_mtf):
            back = glc.mtf_inverse_batch(plan, d_mtf, n, nblk)
            plan.synchronize()
            return back
        got = R.behind_the_gate(st, call, [np.concatenate(a)], [np.concatenate(b)])
    assert np.array_equal(got, np.concatenate([O.imtf(x) for x in b])), name


@functools.lru_cache(maxsize=None)
def _two_blocks():
    b = [datagen.text_bytes(4096, seed=71), datagen.zipf_bytes(4096, seed=72)]
    a = b[::-1]
    return b, [O.compress(x) for x in b], a, [O.compress(x) for x in a]


@serial_and_pipelined
def test_compact_layout(glc, st, pipelined):
    """glcCompressBatchCompact writes the oracle's streams back to back; glcDecompressBatchCompact reads that layout"""
    b, wants, a, wants_a = _two_blocks()
    n, nblk = 4096, 2

    def compact_host(ws):
        off = np.concatenate([[0], np.cumsum([w["size"] for w in ws])]).astype(np.int64)
        idx, hist, offsets, _ = _strided_host(glc, ws, n)
        return [idx, hist, offsets, _i32(np.concatenate([w["words"] for w in ws])), off]

    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, nblk, pipelined) as plan:
        def compress(d_in):
            out = glc.compress_batch_compact(plan, d_in, n, nblk)
            plan.synchronize()
            return out

        def decompress(idx, hist, offsets, words, off):
            comp = dict(bwt_index=idx, hist=hist, offsets=offsets, words=words, block_off=off, nsub=1)
            back = glc.decompress_batch_compact(plan, comp, n, nblk)
            plan.synchronize()
            return back

        got = R.behind_the_gate(st, compress, [np.concatenate(a)], [np.concatenate(b)])
        want = compact_host(wants)
        assert np.array_equal(got["block_off"], want[4])
        assert np.array_equal(got["words"][:int(want[4][-1])], want[3])
        for i, w in enumerate(wants):
            assert int(got["bwt_index"][i]) == w["bwt_index"] and int(got["size"][i]) == w["size"]
            assert np.array_equal(got["hist"][i * 256:(i + 1) * 256].view(np.uint32), w["hist"])
        back = R.behind_the_gate(st, decompress, compact_host(wants_a), want)
    assert np.array_equal(back, np.concatenate(b))


# --- the container, device form -----------------------------------------------------------------------------------------------------
# A container call keeps its tables, its pinned readback words and the host forms' staging with the plan (CtDevSlot / CtPinSlot,
# csrc/container_internal.h): a primed call frees nothing.  It used to allocate and free them itself, and hipFree / hipHostFree
# wait for the whole device -- then every row below ended with the blocker completed.
def _group(name):
    return "container" if name in S.FILTERS else "small"


@functools.lru_cache(maxsize=None)
def _other_input(name):
    """A of a container entry: its input rolled by an odd count, so every frame holds other bytes"""
    return np.roll(S.entry(name)[2], 4097)


@serial_and_pipelined
@pytest.mark.parametrize("name", list(S.ALL))
def test_container_device_form(glc, st, name, pipelined):
    """compress, decompress, the index walk and one range read across a frame boundary, each through the rig"""
    import torch
    n, rows, x, want = S.entry(name)
    a = _other_input(name)
    off, count = (rows - 1) * n + 100, n + 500
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, rows) as plan:
        S.configure(glc, plan, name, pipelined)
        with torch.cuda.stream(st):                            # A's container, from the GPU: it only primes the decoder
            c_a = R.to_host(glc.container_compress(plan, torch.from_numpy(a.copy()).cuda()))
        group = _group(name)
        c = R.behind_the_gate(st, lambda d: glc.container_compress(plan, d), [a], [x], group)
        assert c.tobytes() == want, "container bytes"
        w = np.frombuffer(want, np.uint8)
        back = R.behind_the_gate(st, lambda d: glc.container_decompress(plan, d, cap=x.size), [c_a], [w], group)
        assert np.array_equal(back, x), "decode"
        assert glc.container_last_error(plan) == (0, -1, -1)

        def index_and_read(d):
            with glc.container_index(plan, d) as ix:
                return ix.info(), glc.container_read_range(plan, ix, d, off, count)
        info, got = R.behind_the_gate(st, index_and_read, [c_a], [w], group)
        assert info[:2] == (x.size, n) and np.array_equal(got, x[off:off + count]), "index / range read"


# --- the container, host-pointer and file forms ---------------------------------------------------------------------------------------
# They take host memory, so there is no device input to gate: the plan is primed with the call on another input (A's
# leftovers in its scratch and staging), then the call on B runs on the plan's stream behind the blocked null stream, where a
# copy between the pinned staging and the device that goes through stream 0 -- a blocking hipMemcpy does -- waits for the blocker.
HOST_FORMS = ("bwt", "huff0_delta", "filter_byte")


@serial_and_pipelined
@pytest.mark.parametrize("name", HOST_FORMS)
def test_container_host_pointer_form(glc, st, name, pipelined):
    n, rows, x, want = S.entry(name)
    a = _other_input(name)
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, rows) as plan:
        S.configure(glc, plan, name, pipelined)
        c_a = glc.container_compress_host(plan, a)             # (A's container, from the GPU: it only primes the decoder)
        c = R.behind_the_gate(st, lambda: glc.container_compress_host(plan, x), [], [], _group(name),
                              prime=lambda: glc.container_compress_host(plan, a))
        assert c.tobytes() == want
        back = R.behind_the_gate(st, lambda: glc.container_decompress_host(plan, np.frombuffer(want, np.uint8)), [], [], _group(name),
                                 prime=lambda: glc.container_decompress_host(plan, c_a))
        assert np.array_equal(back, x)
        assert glc.container_last_error(plan) == (0, -1, -1)


@serial_and_pipelined
@pytest.mark.parametrize("name", HOST_FORMS)
def test_container_file_form(glc, st, tmp_path, name, pipelined):
    """glcContainerCompressFile reads its frames back per chunk (compress_stream): the one place a blocking copy stood"""
    n, rows, x, want = S.entry(name)
    files = {k: tmp_path / k for k in ("a.bin", "a.glcb", "a.back", "in.bin", "out.glcb", "back.bin")}
    _other_input(name).tofile(files["a.bin"])
    x.tofile(files["in.bin"])
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, n, rows) as plan:
        S.configure(glc, plan, name, pipelined)

        def compress(src, dst):
            glc.container_compress_file(plan, str(files[src]), str(files[dst]))
            return files[dst].read_bytes()

        def decompress(src, dst):
            glc.container_decompress_file(plan, str(files[src]), str(files[dst]))
            return files[dst].read_bytes()
        got = R.behind_the_gate(st, lambda: compress("in.bin", "out.glcb"), [], [], _group(name), prime=lambda: compress("a.bin", "a.glcb"))
        assert got == want
        back = R.behind_the_gate(st, lambda: decompress("out.glcb", "back.bin"), [], [], _group(name), prime=lambda: decompress("a.glcb", "a.back"))
        assert back == x.tobytes()


# --- the enqueue-only entries -----------------------------------------------------------------------------------------------------------
# Three segments of unequal length in one buffer -- one empty, one of one byte, one of 3 * 4096 + 5 bytes at an odd offset -- and
# per entry: what the call reads (gated), the call, and the value of the model its own kernel test uses.
OFFS, LENS = (7, 9, 33), (0, 1, 3 * 4096 + 5)
TOTAL = OFFS[2] + LENS[2] + 64
MAXLEN = LENS[2]
GUARD = 0xEE


@functools.lru_cache(maxsize=None)
def _segments(which):
    """the segments of B or of A.  The long one: int16 samples (something for every filter), a stretch of zeros and of one fill
    byte (the zero-run and sparse kernels), the first 1024 bytes again (the dedup map), text"""
    rng = np.random.default_rng(5 if which == "b" else 6)
    t = np.arange(2048)
    wave = (2000 * np.sin(t / (23.0 if which == "b" else 31.0)) + rng.integers(-3, 4, t.size)).astype("<i2").view(np.uint8)
    long = np.concatenate([wave, np.zeros(1024, np.uint8), np.full(1024, 0x20, np.uint8), wave[:1024], datagen.text_bytes(LENS[2] - 7168, seed=8 if which == "b" else 9)])
    assert long.size == LENS[2]
    return (np.zeros(0, np.uint8), np.asarray([0x41 if which == "b" else 0x42], np.uint8), long)


def _placed(segs, fill=GUARD):
    buf = np.full(TOTAL, fill, np.uint8)
    for o, s in zip(OFFS, segs):
        buf[o:o + s.size] = s
    return buf


def _per_segment(fn, which):
    return [fn(s) for s in _segments(which)]


class E:
    """one entry: inputs(which) -> the numpy arrays it reads; call(glc, K, *device inputs) -> outputs; check(got, which)"""

    def __init__(self, inputs, call, check):
        self.inputs, self.call, self.check = inputs, call, check


def _buf_in(which):
    return [_placed(_segments(which))]


def _eq(got, want, what=""):
    assert np.array_equal(np.asarray(got), np.asarray(want)), what


def _zeros(K, shape, dtype):
    import torch
    return torch.zeros(shape, dtype=dtype, device="cuda")


def _out_like_buffer(K):
    import torch
    return torch.full((TOTAL,), GUARD, dtype=torch.uint8, device="cuda")


def _want_placed(fn, which):
    return _placed([fn(s) for s in _segments(which)])


def _shuffled_in(which):
    return [_want_placed(lambda s: M.shuffle(s, 4), which)]


ENTRIES = {}
ENTRIES["shuffle_segments"] = E(_buf_in, lambda glc, K, d: glc.shuffle_segments(d, _out_like_buffer(K), K.off, K.ln, 4, stream=K.st, keep=K.keep),
                                lambda got, w: _eq(got, _want_placed(lambda s: M.shuffle(s, 4), w)))
ENTRIES["unshuffle_segments"] = E(_shuffled_in, lambda glc, K, d: glc.shuffle_segments(d, _out_like_buffer(K), K.off, K.ln, 4, inverse=True, stream=K.st, keep=K.keep),
                                  lambda got, w: _eq(got, _placed(_segments(w))))
ENTRIES["crc32_segments"] = E(_buf_in, lambda glc, K, d: glc.crc32_segments_device(d, K.off, K.ln, stream=K.st, keep=K.keep),
                              lambda got, w: _eq(got.view(np.uint32), [zlib.crc32(s.tobytes()) for s in _segments(w)]))


def _check_probe(got, w):
    pairs = _per_segment(auto_model.probe, w)
    _eq(got[0].view(np.uint32), np.stack([p[0] for p in pairs]), "hist")
    _eq(got[1].view(np.uint32), np.stack([p[1] for p in pairs]), "uniform")


ENTRIES["probe_segments"] = E(_buf_in, lambda glc, K, d: glc.probe_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep), _check_probe)
ENTRIES["bigram_probe_segments"] = E(_buf_in, lambda glc, K, d: glc.bigram_probe_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep),
                                     lambda got, w: _eq(got, np.asarray(_per_segment(choose_model.stats, w), np.int64).reshape(3, 4)))


def _check_filter_probe(got, w):
    rows = _per_segment(F.probe, w)
    _eq(got[0].view(np.uint32), np.stack(rows), "planes")
    _eq(got[1], np.asarray([F.costs(r) for r in rows], np.int64), "costs")


ENTRIES["filter_probe_segments"] = E(_buf_in, lambda glc, K, d: glc.filter_probe_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep),
                                     _check_filter_probe)


def _lag_both(glc, K, d):
    s, w = glc.lag_probe_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep)
    return (s, w) + glc.lag_planes_segments(d, K.off, K.ln, w, max_len=MAXLEN, stream=K.st, keep=K.keep)


def _check_lag(got, w):
    segs = _segments(w)
    sums = [FL.sums(s) for s in segs]
    wins = [FL.winners(x) for x in sums]
    rows = [FL.lag_planes(s, v) for s, v in zip(segs, wins)]
    _eq(got[0], np.asarray(sums, np.int64).reshape(3, FL.SUMS), "sums")
    _eq(got[1], np.asarray(wins, np.int64).reshape(3, 3), "winners")
    _eq(got[2].view(np.uint32), np.stack(rows), "planes")
    _eq(got[3], np.asarray([FL.lag_costs(r) for r in rows], np.int64), "costs")


ENTRIES["lag_probe_and_planes_segments"] = E(_buf_in, _lag_both, _check_lag)


def _grid_both(glc, K, d):
    s, w = glc.grid_probe_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep)
    return (s, w) + glc.grid_planes_segments(d, K.off, K.ln, w, max_len=MAXLEN, stream=K.st, keep=K.keep)


def _check_grid(got, w):
    segs = _segments(w)
    sums = [FQ.sums(s) for s in segs]
    wins = [FQ.winners(x) for x in sums]
    rows = [FQ.grid_planes(s, v) for s, v in zip(segs, wins)]
    _eq(got[0].view(np.uint32), np.stack(sums).astype(np.uint32), "sums")
    _eq(got[1], np.asarray(wins, np.int64).reshape(3, 3), "winners")
    _eq(got[2].view(np.uint32), np.stack(rows), "planes")
    _eq(got[3], np.asarray([FQ.grid_costs(r, v) for r, v in zip(rows, wins)], np.int64), "costs")


ENTRIES["grid_probe_and_planes_segments"] = E(_buf_in, _grid_both, _check_grid)


def _byte_both(glc, K, d):
    a, s, w = glc.byte_probe_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep)
    return (a, s, w) + glc.byte_planes_segments(d, K.off, K.ln, w, max_len=MAXLEN, stream=K.st, keep=K.keep)


def _check_byte(got, w):
    segs = _segments(w)
    A = [FB.lag_sums(s) for s in segs]
    Ss = [FB.stride_sums(s) for s in segs]
    wins = [FB.winners(a, s) for a, s in zip(A, Ss)]
    rows = [FB.byte_planes(s, v) for s, v in zip(segs, wins)]
    _eq(got[0], np.asarray(A, np.int64).reshape(3, 16), "lag sums")
    _eq(got[1].view(np.uint32), np.stack(Ss).astype(np.uint32), "stride sums")
    _eq(got[2], np.asarray(wins, np.int64).reshape(3, 2), "winners")
    _eq(got[3].view(np.uint32), np.stack(rows), "planes")
    _eq(got[4], np.asarray([FB.byte_costs(s, r, v) for s, r, v in zip(segs, rows, wins)], np.int64), "costs")


ENTRIES["byte_probe_and_planes_segments"] = E(_buf_in, _byte_both, _check_byte)


# rANS: the records of the non-empty segments (the model takes none of length 0)
def _ans_records(which):
    return [ans_model.encode_record(s) if s.size else None for s in _segments(which)]


def _ans_rec_off(glc):
    off, total = [], 0
    for l in LENS:
        off.append(total)
        total += glc.ans_bound_words(l)
    return off, total


def _check_ans_encode(glc):
    def check(got, w):
        hist, rec, words = got
        rec_off, _ = _ans_rec_off(glc)
        for i, r in enumerate(_ans_records(w)):
            if r is not None:
                _eq(hist[i].view(np.uint32), r[0], "hist %d" % i)
                assert int(words[i]) == r[1].size
                _eq(rec[rec_off[i]:rec_off[i] + r[1].size].view(np.uint32), r[1], "record %d" % i)
    return check


def _ans_encode(glc, K, d):
    hist, rec, _, words = glc.ans_encode_segments(d, K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep, rec_off=K.rec_off)
    return hist, rec, words


def _ans_decode_inputs(glc):
    def inputs(which):
        rec_off, total = _ans_rec_off(glc)
        rec = np.zeros(max(1, total), np.uint32)
        hist = np.zeros((3, 256), np.uint32)
        words = np.zeros(3, np.int64)
        for i, r in enumerate(_ans_records(which)):
            if r is not None:
                hist[i], words[i] = r[0], r[1].size
                rec[rec_off[i]:rec_off[i] + r[1].size] = r[1]
        return [_i32(rec), words, _i32(hist)]
    return inputs


def _ans_decode(glc, K, rec, words, hist):
    return glc.ans_decode_segments(rec, K.rec_off, words, hist, _out_like_buffer(K), K.off, K.ln, max_len=MAXLEN, stream=K.st, keep=K.keep)


def _zrun_parts(which):
    parts = _per_segment(runs_model.split, which)
    return ([a for a, _ in parts], [b for _, b in parts])


def _zrun_split(glc, K, d):
    d_a, d_b = _out_like_buffer(K), _out_like_buffer(K)
    alen, blen = glc.zerorun_split_segments(d, d_a, d_b, K.off, K.ln, stream=K.st, keep=K.keep)
    return d_a, d_b, alen, blen


def _check_zrun_split(got, w):
    A, B = _zrun_parts(w)
    _eq(got[0], _placed(A), "A")
    _eq(got[1], _placed(B), "B")
    _eq(got[2], [a.size for a in A], "A lengths")
    _eq(got[3], [b.size for b in B], "B lengths")


def _zrun_join_inputs(which):
    A, B = _zrun_parts(which)
    return [_placed(A), _placed(B), np.asarray([a.size for a in A], np.int64), np.asarray([b.size for b in B], np.int64)]


ENTRIES["zerorun_split_segments"] = E(_buf_in, _zrun_split, _check_zrun_split)
ENTRIES["zerorun_join_segments"] = E(_zrun_join_inputs,
                                     lambda glc, K, a, b, al, bl: glc.zerorun_join_segments(a, b, _out_like_buffer(K), K.off, al, bl, K.ln, stream=K.st, keep=K.keep),
                                     lambda got, w: _eq(got, _placed(_segments(w))))

FILLS = (0, 0x41, 0x20)                                        # the fill byte of each segment for the sparse kernels


def _sparse_parts(which):
    return [sparse_model.split(s, f) for s, f in zip(_segments(which), FILLS)]


def _sparse_mask(which, glc):
    mask = np.zeros((3, glc.sparse_mask_words(MAXLEN)), np.uint32)
    for i, (_, m, _) in enumerate(_sparse_parts(which)):
        mask[i, :m.size] = m
    return mask


def _sparse_split(glc, K, d):
    kept = _out_like_buffer(K)
    mask, klen = glc.sparse_split_segments(d, kept, K.off, K.ln, K.fill, stream=K.st, keep=K.keep)
    return kept, mask, klen


def _check_sparse_split(glc):
    def check(got, w):
        parts = _sparse_parts(w)
        _eq(got[0], _placed([k for _, _, k in parts]), "kept")
        _eq(got[1].view(np.uint32), _sparse_mask(w, glc), "mask")
        _eq(got[2], [k.size for _, _, k in parts], "kept lengths")
    return check


def _dedup_src(which):
    return dedup_model.map_segments(list(_segments(which)), MAXLEN)


def _dedup_fill_inputs(which):
    """the buffer with every repeated chunk overwritten (the filler must bring it back) and the model's map"""
    segs = [s.copy() for s in _segments(which)]
    src = _dedup_src(which)
    nch = dedup_model.nchunks(MAXLEN)
    for g, e in enumerate(src.tolist()):
        if e < g:
            i, c = divmod(g, nch)
            segs[i][512 * c:512 * c + 512] = 0xCC
    assert any(e < g for g, e in enumerate(src.tolist())), "the long segment repeats no chunk"
    return [_placed(segs), _i32(src)]


ENTRIES["dedup_map_segments"] = E(_buf_in, lambda glc, K, d: glc.dedup_map_segments(d, K.off, K.ln, MAXLEN, stream=K.st, keep=K.keep),
                                  lambda got, w: _eq(got.view(np.uint32), _dedup_src(w)))
ENTRIES["dedup_fill_segments"] = E(_dedup_fill_inputs, lambda glc, K, d, src: glc.dedup_fill_segments(d, K.off, K.ln, src, MAXLEN, stream=K.st, keep=K.keep),
                                   lambda got, w: _eq(got, _placed(_segments(w))))


# the *Device and *RangeDevice forms on the long segment alone, at an odd address
def _long(which):
    return _segments(which)[2]


def _device_pair(name, forward, inverse, model_f, args):
    """a filter and its inverse: forward reads the segment, the inverse reads the model's filtered bytes"""
    ENTRIES[name] = E(lambda w: [_long(w)], lambda glc, K, d: getattr(glc, forward)(d, *args, stream=K.st),
                      lambda got, w: _eq(got, model_f(_long(w), *args)))
    ENTRIES["un" + name] = E(lambda w: [np.ascontiguousarray(model_f(_long(w), *args))], lambda glc, K, d: getattr(glc, inverse)(d, *args, stream=K.st),
                             lambda got, w: _eq(got, _long(w)))


_device_pair("shuffle_device", "shuffle", "unshuffle", M.shuffle, (4,))
_device_pair("delta_shuffle_device", "delta_shuffle", "undelta_unshuffle", M.delta_shuffle, (2,))
_device_pair("lag_delta_shuffle_device", "lag_delta_shuffle", "unlag_delta_unshuffle", lag_model.lag_delta_shuffle, (2, 3, 1))
_device_pair("grid_delta_shuffle_device", "grid_delta_shuffle", "ungrid_delta_unshuffle", grid_model.grid_delta_shuffle, (2, 100, 1))
_device_pair("byte_delta_device", "byte_delta", "unbyte_delta", BD.byte_delta, (3, 100))

# range forms: elements [first, first + count) behind the first restart point, read from the filtered bytes
RUN = 2048
ENTRIES["unshuffle_range"] = E(lambda w: [np.ascontiguousarray(M.shuffle(_long(w), 4))],
                               lambda glc, K, d: glc.unshuffle_range(d, 4, 1001, 777, stream=K.st),
                               lambda got, w: _eq(got, _long(w)[4 * 1001:4 * (1001 + 777)]))
ENTRIES["undelta_unshuffle_range"] = E(lambda w: [np.ascontiguousarray(M.delta_shuffle(_long(w), 2))],
                                       lambda glc, K, d: glc.undelta_unshuffle_range(d, 2, RUN, 3001, stream=K.st),
                                       lambda got, w: _eq(got, _long(w)[2 * RUN:2 * (RUN + 3001)]))
ENTRIES["unlag_delta_unshuffle_range"] = E(lambda w: [np.ascontiguousarray(lag_model.lag_delta_shuffle(_long(w), 2, 3, 1))],
                                           lambda glc, K, d: glc.unlag_delta_unshuffle_range(d, 2, 3, 1, RUN, 3001, stream=K.st),
                                           lambda got, w: _eq(got, _long(w)[2 * RUN:2 * (RUN + 3001)]))
ENTRIES["ungrid_delta_unshuffle_range"] = E(lambda w: [np.ascontiguousarray(grid_model.grid_delta_shuffle(_long(w), 2, 60, 1))],
                                            lambda glc, K, d: glc.ungrid_delta_unshuffle_range(d, 2, 60, 1, grid_model.period(60), 3001, stream=K.st),
                                            lambda got, w: _eq(got, _long(w)[2 * grid_model.period(60):2 * (grid_model.period(60) + 3001)]))
ENTRIES["unbyte_delta_range"] = E(lambda w: [np.ascontiguousarray(BD.byte_delta(_long(w), 3, 100))],
                                  lambda glc, K, d: glc.unbyte_delta_range(d, 3, 100, BD.step(100), 5001, stream=K.st),
                                  lambda got, w: _eq(got, _long(w)[BD.step(100):BD.step(100) + 5001]))
LATE = ("ans_encode_segments", "ans_decode_segments", "sparse_split_segments", "sparse_join_segments")     # (they need the binding: made per test)


class _Call:
    """what an entry's call needs beside its inputs: the stream, the list that keeps the helpers' temporaries, and the segment
    lists uploaded ahead of the call"""

    def __init__(self, glc, stream):
        import torch
        self.st, self.keep = stream, []
        with torch.cuda.stream(stream):
            self.off, self.ln = glc.SegmentList(OFFS, "cuda"), glc.SegmentList(LENS, "cuda")
            self.fill = glc.SegmentList(FILLS, "cuda", torch.int32)
            self.rec_off = glc.SegmentList(_ans_rec_off(glc)[0], "cuda")
            stream.synchronize()


def _entry(glc, name):
    if name == "ans_encode_segments":
        return E(_buf_in, _ans_encode, _check_ans_encode(glc))
    if name == "ans_decode_segments":
        return E(_ans_decode_inputs(glc), _ans_decode, lambda got, w: _eq(got, _placed([s for s in _segments(w)])))
    if name == "sparse_split_segments":
        return E(_buf_in, _sparse_split, _check_sparse_split(glc))
    if name == "sparse_join_segments":
        return E(lambda w: [_placed([k for _, _, k in _sparse_parts(w)]), _i32(_sparse_mask(w, glc))],
                 lambda glc_, K, kept, mask: glc_.sparse_join_segments(kept, _out_like_buffer(K), K.off, K.ln, K.fill, mask, stream=K.st, keep=K.keep),
                 lambda got, w: _eq(got, _placed(_segments(w))))
    return ENTRIES[name]


@pytest.mark.parametrize("name", list(ENTRIES) + list(LATE))
def test_enqueue_only_entry(glc, st, name):
    """the call returns with the gate still shut, and what it queued ran behind the gate: the model's values of B"""
    e = _entry(glc, name)
    K = _Call(glc, st)
    got = R.behind_the_gate(st, lambda *d: e.call(glc, K, *d), e.inputs("a"), e.inputs("b"), enqueue_only=True)
    e.check(got, "b")
    assert K.keep or name.endswith(("_device", "_range")), "the helper kept no temporaries: it did not take the keep path"


# --- the control: the rig sees a stage on the wrong stream ------------------------------------------------------------------------------
def test_control_a_stage_on_the_null_stream_returns_stale_bytes(glc, st):
    """a two-step pipeline written here, wrong on purpose: glcShuffleDevice on S, then glcUnshuffleDevice with stream=None.  The
    second stage does not wait for the first (S is non-blocking), so it reads what the scratch held -- A's shuffled bytes -- and
    the output is not B.  Nothing faults: every address is valid.  The null stream is not blocked in this run (the stage on it
    has to run), so the protocol is written out here around the rig's own gate (stream_rig.shut_gate)."""
    import torch
    b, a = _long("b"), _long("a")
    with torch.cuda.stream(st):
        d_b, d_in = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(a.copy()).cuda()
        mid, out = torch.empty_like(d_in), torch.empty_like(d_in)
        glc.shuffle(d_in, 4, out=mid, stream=st)               # primed with A
        st.synchronize()
        d_in.copy_(torch.from_numpy(R.decoy(b)).cuda())
        st.synchronize()
        gate = R.shut_gate(st, [d_in], [d_b])                  # (the rig's own step 3)
        glc.shuffle(d_in, 4, out=mid, stream=st)
        glc.unshuffle(mid, 4, out=out, stream=None)            # the mistake
        torch.cuda.default_stream().synchronize()              # the wrong stage has run ...
        assert not gate.query(), "the gate had opened before the mis-streamed stage ran: this run proved nothing"
        st.synchronize()
        got = out.cpu().numpy()
    torch.cuda.synchronize()
    assert not np.array_equal(got, b), "a stage on the null stream went unseen"
    assert np.array_equal(got, a)                              # ... on A's leftovers


# --- a plan that moves between streams, and two plans driven in turn ------------------------------------------------------------------------
def test_one_plan_moves_from_stream_to_stream(glc, st, cuda):
    import torch
    x, want, a, want_a = _one_block("random_70001")
    s2 = R.independent_stream()
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, x.size, 1) as plan:
        _round_trip_on(glc, st, plan, x.size, [a], [want_a], [x], [want], "small", "on S1")
        plan.synchronize()
        plan.set_stream(s2.cuda_stream)
        _round_trip_on(glc, s2, plan, x.size, [a], [want_a], [x], [want], "small", "on S2")
        plan.synchronize()
        plan.set_stream(None)
        out = glc.compress_batch(plan, torch.from_numpy(x.copy()).cuda(), x.size, 1)
        plan.synchronize()
        _assert_streams(R.to_host(out), [want], "on the null stream")
        back = glc.decompress_batch(plan, out, x.size, 1)
        plan.synchronize()
        assert np.array_equal(back.cpu().numpy(), x)


def test_two_plans_on_two_streams_driven_in_turn(glc, st, cuda):
    """one host thread, calls alternating between the plans; each result against its model"""
    import torch
    s2 = torch.cuda.Stream()
    x1, w1, _, _ = _one_block("random_70001")
    n2, rows2, x2, w2 = S.entry("filter_lag")
    with _plan_on(glc, st, glc.CUDPP_COMPRESS, x1.size, 1, True) as p1, _plan_on(glc, s2, glc.CUDPP_COMPRESS, n2, rows2) as p2:
        S.configure(glc, p2, "filter_lag", True)
        with torch.cuda.stream(st):
            d1 = torch.from_numpy(x1.copy()).cuda()
        with torch.cuda.stream(s2):
            d2 = torch.from_numpy(x2.copy()).cuda()
        for rnd in range(3):
            with torch.cuda.stream(st):
                out = glc.compress_batch(p1, d1, x1.size, 1)   # queued, not waited for
            with torch.cuda.stream(s2):
                c = glc.container_compress(p2, d2)
            with torch.cuda.stream(st):
                back = glc.decompress_batch(p1, out, x1.size, 1)
            with torch.cuda.stream(s2):
                y = glc.container_decompress(p2, c, cap=x2.size)
                assert R.to_host(c).tobytes() == w2 and np.array_equal(R.to_host(y), x2), rnd
            with torch.cuda.stream(st):
                p1.synchronize()
                _assert_streams(R.to_host(out), [w1], "round %d" % rnd)
                assert np.array_equal(R.to_host(back), x1), rnd
