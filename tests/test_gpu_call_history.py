"""No result may depend on what the plan's previous call was (-m gpu).

A plan keeps state between calls: the container's grow-only buffers (carved differently by every mode), the call parity of
the sorter's per-call masks and of the filter's staging, the streak of text-like calls that lets small calls skip the bucket
sorter, the epoch of the look-back granules, the halves of the pipelined BWT buffers, whether the side stream was used, the
pinned readback words.  The other tests repeat one call on a plan; here a DIFFERENT call P runs first on a fresh plan, then
the target call T, and T's result is compared with the CPU model or the oracle -- the value a fresh plan gives, but asserted
against the model.  Each (P, T) pair runs twice in a row on the plan, so T is seen at both call parities."""
import functools

import numpy as np
import pytest

import container_model as M
import datagen
import oracle_lib as O
import small_container as S
import tier_batches as T

pytestmark = pytest.mark.gpu
N1M = 1 << 20
ILLEGAL, UNKNOWN = 2, 9999


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.uint8, copy=True)).cuda()


def _host(t):
    return t.cpu().numpy()


def _reset_container(glc, plan):
    """every container setting back to a new plan's, each by its own setter (off is always legal), innermost first; then the
    getters must all say so"""
    glc.container_set_filter_byte(plan, 0)
    glc.container_set_filter_grid(plan, 0)
    glc.container_set_filter_lag(plan, 0)
    glc.container_set_byte_delta(plan, 0, 0)
    glc.container_set_filter_auto(plan, 0)
    glc.container_set_delta_grid(plan, 0, 0)
    glc.container_set_delta_lag(plan, 1, 0)
    for off in (glc.container_set_dedup, glc.container_set_auto, glc.container_set_ans, glc.container_set_sparse,
                glc.container_set_runs, glc.container_set_delta, glc.container_set_shuffle):
        off(plan, 0)
    glc.container_set_codec(plan, glc.CONTAINER_CODEC_BWT)
    state = (glc.container_get_codec(plan), glc.container_get_shuffle(plan), glc.container_get_delta(plan), glc.container_get_runs(plan),
             glc.container_get_sparse(plan), glc.container_get_ans(plan), glc.container_get_auto(plan), glc.container_get_dedup(plan),
             glc.container_get_filter_auto(plan), tuple(glc.container_get_delta_lag(plan)), tuple(glc.container_get_delta_grid(plan)),
             glc.container_get_filter_byte(plan), glc.container_get_filter_grid(plan), glc.container_get_filter_lag(plan),
             tuple(glc.container_get_byte_delta(plan)))
    assert state == (glc.CONTAINER_CODEC_BWT, 0, 0, 0, 0, 0, 0, 0, 0, (1, 0), (0, 0), 0, 0, 0, (0, 0)), state


@functools.lru_cache(maxsize=None)
def _short():
    x = datagen.text_bytes(1203, seed=1203)
    return x, O.compress(x)


@functools.lru_cache(maxsize=None)
def _random_block(n):
    x = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    return x, O.compress(x)


@functools.lru_cache(maxsize=None)
def _container_input(n, rows):
    """The rigs' frame pattern at the plan's own shape: two full frames, a frame of one block, a tail of 1203 bytes.  On the
    small plans that is small_container's input; on a plan of 1 MiB blocks, 2 * rows + 1 blocks of that size and the tail."""
    if (n, rows) == (S.N, S.ROWS):
        return S.data()
    parts = [datagen.text_bytes(n, seed=300 + i) if i % 3 == 0 else datagen.zipf_bytes(n, seed=300 + i) for i in range(2 * rows + 1)]
    x = np.concatenate(parts + [datagen.text_bytes(S.TAIL, seed=10)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want_container(codec, n, rows):
    """the model's container of _container_input under the plain setting of `codec`, once per shape"""
    c = M.write(_container_input(n, rows), n, rows, 0, codec)
    assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(rows, n), (rows, n), (1, n), (1, S.TAIL)]
    return c


def _assert_block(out, i, want, what):
    size = int(out["size"][i].item())
    assert int(out["bwt_index"][i].item()) == want["bwt_index"] and size == want["size"], "%s: index / size" % what
    words = _host(out["words"][i * out["stride"]:i * out["stride"] + size]).view(np.uint32)
    assert np.array_equal(words, want["words"]), "%s: stream" % what
    assert np.array_equal(_host(out["hist"][i * 256:(i + 1) * 256]).view(np.uint32), want["hist"]), "%s: histogram" % what


def _one_block(glc, plan, x, want, what):
    out = glc.compress_batch(plan, _gpu(x), x.size, 1)
    plan.synchronize()
    _assert_block(out, 0, want, what)
    back = glc.decompress_batch(plan, out, x.size, 1)
    plan.synchronize()
    assert np.array_equal(_host(back), x), "%s: decode" % what


# --- the target calls --------------------------------------------------------------------------------------------------------
def t_short_block(glc, plan, pipelined):
    """one block of 1203 bytes, the rigs' tail"""
    plan.set_pipelining(pipelined)
    _one_block(glc, plan, *_short(), "one block of 1203")


def _t_container(glc, plan, pipelined, codec):
    plan.set_pipelining(pipelined)
    _reset_container(glc, plan)
    glc.container_set_codec(plan, codec)
    c = glc.container_compress(plan, _gpu(_container_input(plan.n, plan.rows)))
    assert _host(c).tobytes() == _want_container(codec, plan.n, plan.rows), "container bytes, codec %d" % codec


def t_container_bwt(glc, plan, pipelined):
    _t_container(glc, plan, pipelined, 0)


def t_container_huff0(glc, plan, pipelined):
    _t_container(glc, plan, pipelined, 1)


def t_container_decode(glc, plan, pipelined):
    """the model's containers of both codecs read back"""
    plan.set_pipelining(pipelined)
    _reset_container(glc, plan)
    for codec in (0, 1):
        glc.container_set_codec(plan, codec)
        d_c = _gpu(np.frombuffer(_want_container(codec, plan.n, plan.rows), np.uint8))
        assert np.array_equal(_host(glc.container_decompress(plan, d_c)), _container_input(plan.n, plan.rows)), "container decode, codec %d" % codec
        assert glc.container_last_error(plan) == (0, -1, -1)


TARGETS = {"short_block": t_short_block, "container_bwt": t_container_bwt, "container_huff0": t_container_huff0,
           "container_decode": t_container_decode}


# --- the calls that go first: name -> (plan n, plan rows, the call, T's pipelining, a call behind T or None) --------------------
@functools.lru_cache(maxsize=None)
def _all_tiers_want():
    return list(T.all_tiers_compressed_1m())


def p_all_tiers(glc, plan):
    """every tier of the sorter, every block at the plan's full n: the general sorter's arrays get allocated, the look-back
    epoch moves, the side stream may run"""
    blocks = T.all_tiers_blocks_1m()
    out = glc.compress_batch(plan, _gpu(np.concatenate(blocks)), N1M, len(blocks))
    plan.synchronize()
    assert plan.last_sort_stats() == T.ALL_TIERS_STATS and plan.last_sort_resumed() == T.ALL_TIERS_RESUMED
    for i, w in enumerate(_all_tiers_want()):
        _assert_block(out, i, w, "all tiers, block %d" % i)


@functools.lru_cache(maxsize=None)
def _streak_text():
    x = datagen.text_bytes(N1M, seed=77)                       # (test_gpu_sample_sorter.py's streak test: the probe calls it text-like)
    return x, O.compress(x)


def p_text_streak(glc, plan):
    """one-block text calls until the streak is eight long, which arms the skip of the bucket sorter: T runs on an armed plan"""
    x, want = _streak_text()
    d = _gpu(x)
    while plan.last_sort_skipped()[1] < 8:                     # (eight on a fresh plan; the pair's second round starts from what T left)
        before = plan.last_sort_skipped()[1]
        out = glc.compress_batch(plan, d, N1M, 1)
        plan.synchronize()
        assert plan.last_sort_skipped() == (False, before + 1), "the probe did not call the text block text-like"
        _assert_block(out, 0, want, "text call %d of the streak" % (before + 1))
    out = glc.compress_batch(plan, d, N1M, 1)
    plan.synchronize()
    assert plan.last_sort_skipped()[0] is True, "the armed plan did not skip"
    _assert_block(out, 0, want, "a skipped text call")


def after_text_streak(glc, plan):
    """behind T: a random block, which is not text-like, ends whatever streak there is -- with the oracle's bytes"""
    y, want_y = _random_block(70001)
    out = glc.compress_batch(plan, _gpu(y), y.size, 1)
    plan.synchronize()
    assert plan.last_sort_skipped()[1] == 0, plan.last_sort_skipped()
    _assert_block(out, 0, want_y, "the random block behind the streak")


def p_other_modes(glc, plan):
    """the encoder's codec scratch carved for the runs mode, then for the order-0 codec, then for its dedup mode"""
    plan.set_pipelining(False)
    for name in ("bwt_runs", "huff0", "dedup"):
        _reset_container(glc, plan)
        S.configure(glc, plan, name)
        c = glc.container_compress(plan, _gpu(S.data()))
        assert _host(c).tobytes() == S.want(name), name
        assert np.array_equal(_host(glc.container_decompress(plan, c)), S.data()), name


@functools.lru_cache(maxsize=None)
def _bigger():
    y = np.concatenate([datagen.text_bytes(8 * S.N, seed=21), datagen.zipf_bytes(9 * S.N, seed=22), datagen.float_bytes(3 * S.N + 777, seed=23)])
    return y, M.write(y, S.N, 8, 4)                            # frames of 8 rows where the plan has 4, through the shuffle: staged


def p_bigger_container_decodes_first(glc, plan):
    """the plan's first container call is a DECODE, of frames longer than its own and filtered: the staging grows twice"""
    _reset_container(glc, plan)
    y, c = _bigger()
    assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(c, np.uint8)))), y)


def p_refusals(glc, plan):
    """a decode refused at the stream header and a compress refused for capacity: both leave early"""
    import torch
    _reset_container(glc, plan)
    x = S.data()
    c = bytearray(_want_container(0, plan.n, plan.rows))
    c[0] ^= 0x20                                               # the stream header's magic
    with pytest.raises(glc.CudppError) as e:
        glc.container_decompress(plan, _gpu(np.frombuffer(bytes(c), np.uint8)), cap=x.size)
    assert e.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
    need = len(_want_container(0, plan.n, plan.rows))
    out = torch.full((need + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    rc = glc._ct().glcContainerCompressDevice(plan.handle, _gpu(x).data_ptr(), x.size, out.data_ptr(), need - 1, d_len.data_ptr())
    assert rc == ILLEGAL and glc.container_last_error(plan)[0] == 6 and int(d_len.item()) == need
    assert bool((out[need - 1:] == 0xCD).all())


def p_pipelined_container(glc, plan):
    plan.set_pipelining(True)
    _reset_container(glc, plan)
    S.configure(glc, plan, "bwt_shuffle4", True)
    c = glc.container_compress(plan, _gpu(S.data()))
    assert _host(c).tobytes() == S.want("bwt_shuffle4")
    assert np.array_equal(_host(glc.container_decompress(plan, c)), S.data())


def p_serial_container(glc, plan):
    plan.set_pipelining(False)
    _reset_container(glc, plan)
    S.configure(glc, plan, "bwt_shuffle4", False)
    c = glc.container_compress(plan, _gpu(S.data()))
    assert _host(c).tobytes() == S.want("bwt_shuffle4")
    assert np.array_equal(_host(glc.container_decompress(plan, c)), S.data())


def p_timing3(glc, plan):
    """a call under the stage timer and the live kernel profile (one stream, no side stages, event pairs around launches)"""
    plan.enable_timing(3)
    try:
        x, want = _random_block(S.N)
        _one_block(glc, plan, x, want, "a call under enable_timing(3)")
        c = glc.container_compress(plan, _gpu(S.data()))
        plan.synchronize()
        assert np.array_equal(_host(glc.container_decompress(plan, c)), S.data())
    finally:
        plan.enable_timing(0)


PREVIOUS = {
    "all_tiers": (N1M, 9, p_all_tiers, False, None),
    "text_streak": (N1M, 4, p_text_streak, False, after_text_streak),
    "other_modes": (S.N, S.ROWS, p_other_modes, False, None),
    "bigger_container_decodes_first": (S.N, S.ROWS, p_bigger_container_decodes_first, False, None),
    "refusals": (S.N, S.ROWS, p_refusals, False, None),
    "pipelined_then_serial": (S.N, S.ROWS, p_pipelined_container, False, None),
    "serial_then_pipelined": (S.N, S.ROWS, p_serial_container, True, None),
    "timing3": (S.N, S.ROWS, p_timing3, False, None),
}


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("previous", list(PREVIOUS))
def test_target_call_behind_another_call(glc, cuda, previous, target):
    n, rows, first, t_pipelined, behind = PREVIOUS[previous]
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
        for rnd in range(2):
            first(glc, plan)
            TARGETS[target](glc, plan, t_pipelined)
            if behind:
                behind(glc, plan)


# --- the second matrix: formats 13 to 16 on plans of (65536, 4) ---------------------------------------------------------------------
# The filter probes of formats 13, 14 and 16 keep their winners in device memory between launches and read a wider pinned
# record back; the hand-set byte predictor of format 15 carves the same staging its own way.  Inputs and expected bytes are
# small_container.FILTERS' (the golden fixtures, the byte-delta model).
BIG_N, BIG_ROWS = S.BIG_N, S.BIG_ROWS


def _configured(glc, plan, name, pipelined):
    _reset_container(glc, plan)
    assert S.entry(name)[:2] == (plan.n, plan.rows)
    return S.configure(glc, plan, name, pipelined)


def _encode_equals(glc, plan, name, pipelined):
    _configured(glc, plan, name, pipelined)
    _, _, x, want = S.entry(name)
    c = glc.container_compress(plan, _gpu(x))
    assert _host(c).tobytes() == want, "%s: container bytes" % name


def _decode_equals(glc, plan, name, pipelined):
    _configured(glc, plan, name, pipelined)
    _, _, x, want = S.entry(name)
    assert np.array_equal(_host(glc.container_decompress(plan, _gpu(np.frombuffer(want, np.uint8)))), x), "%s: decode" % name
    assert glc.container_last_error(plan) == (0, -1, -1)


@functools.lru_cache(maxsize=None)
def _bwt_text():
    x = datagen.text_bytes(5 * BIG_N + S.TAIL, seed=31)        # a full frame, a frame of one block, a tail
    return x, M.write(x, BIG_N, BIG_ROWS)


@functools.lru_cache(maxsize=None)
def _refused_v16():
    """one case of filter_byte_model.refusal_cases: a flipped bit in a record, which the reader meets after it has started"""
    import filter_byte_model as B
    cases, _ = B.refusal_cases(S.entry("filter_byte")[3])
    (cont, want), = [(c, w) for name, c, w, reads in cases if name == "a flipped record bit" and reads == B.READS]
    assert want[0] == M.RECORD_CRC
    return cont, want


def p2_bwt_text(glc, plan):
    """a BWT container of text: the sorter's arrays, the BWT codec's carving of the scratch"""
    plan.set_pipelining(False)
    _reset_container(glc, plan)
    x, want = _bwt_text()
    c = glc.container_compress(plan, _gpu(x))
    assert _host(c).tobytes() == want
    assert np.array_equal(_host(glc.container_decompress(plan, c)), x)


def p2_v15_hand_set(glc, plan):
    _encode_equals(glc, plan, "byte_delta", False)
    _decode_equals(glc, plan, "byte_delta", False)


def p2_v14_encode(glc, plan):
    _encode_equals(glc, plan, "filter_grid", False)


def p2_v16_decode(glc, plan):
    """on a fresh plan its first call"""
    _decode_equals(glc, plan, "filter_byte", False)


def p2_v16_refused(glc, plan):
    _configured(glc, plan, "filter_byte", False)
    cont, want = _refused_v16()
    with pytest.raises(glc.CudppError) as e:
        glc.container_decompress(plan, _gpu(np.frombuffer(cont, np.uint8)), cap=S.entry("filter_byte")[2].size)
    assert e.value.code == UNKNOWN and glc.container_last_error(plan) == want


def t2_v16_encode(glc, plan, pipelined):
    """the fixture's bytes, and the four reports of the picks its frame words name"""
    import filter_auto_model as F
    import filter_byte_model as B
    _encode_equals(glc, plan, "filter_byte", pipelined)
    picks = [B.word_format(w) for w in F.frame_words(S.entry("filter_byte")[3])]
    assert glc.container_last_filters(plan) == B.last_filters(picks)
    assert glc.container_last_lag_filters(plan) == B.last_lag_filters(picks)
    assert glc.container_last_grid_filters(plan) == B.last_grid_filters(picks)
    assert glc.container_last_byte_filters(plan) == B.last_byte_filters(picks)


def t2_v16_decode(glc, plan, pipelined):
    _decode_equals(glc, plan, "filter_byte", pipelined)


def t2_v15(glc, plan, pipelined):
    for name in ("byte_delta", "byte_delta_lag"):
        _encode_equals(glc, plan, name, pipelined)
        _decode_equals(glc, plan, name, pipelined)


PREVIOUS2 = {"bwt_text": p2_bwt_text, "v15_hand_set": p2_v15_hand_set, "v14_encode": p2_v14_encode, "v16_decode_first": p2_v16_decode,
             "v16_refused": p2_v16_refused}
TARGETS2 = {"v16_encode": t2_v16_encode, "v16_decode": t2_v16_decode, "v15_encode_decode": t2_v15}


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
@pytest.mark.parametrize("target", list(TARGETS2))
@pytest.mark.parametrize("previous", list(PREVIOUS2))
def test_filter_target_behind_another_call(glc, cuda, previous, target, pipelined):
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, BIG_N, rows=BIG_ROWS) as plan:
        for rnd in range(2):
            PREVIOUS2[previous](glc, plan)
            TARGETS2[target](glc, plan, pipelined)
