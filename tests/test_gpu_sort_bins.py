"""k_fs_sort_bwt's rank step by bin occupancy (csrc/bwt_bucket.hip).  A bin of more than four words is flagged in its start
entry by the words that arrived fifth and later; a flagged or tied word takes a second look at the keys behind the first
four, which settles bins of up to eight words in straight-line code, and only longer bins walk the loop; whether a
workgroup has work-list entries to write is read from its own counter.  Which of these a block exercises is a property of
the input: every test asserts it with the CPU model (fs_bin_model.py) BEFORE the GPU call, then compares BWT bytes and
index with the oracle and asserts that no block was flagged.

i.i.d. bytes give bins of 5 and 6; longer bins come from a short segment planted k times in uniform bytes (suffixes that
share their first three symbols share a bin, and what follows keeps their codes apart); ties from a longer segment planted
twice.  The seeds were found by searching on the CPU for the properties asserted below."""
import numpy as np
import pytest

import datagen
import fs_bin_model as B
import fs_fill_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _mixture(n, share=0.6):
    """the first int(share n) bytes from 8 symbols, the rest from 256: buckets from nearly empty to nearly full"""
    rng = np.random.default_rng(3)
    k = int(share * n)
    return np.concatenate([rng.integers(0, 8, k, dtype=np.uint8), rng.integers(0, 256, n - k, dtype=np.uint8)])


def _planted(base, segments, seed):
    """every (segment, copies) of `segments` planted at distinct 16-byte slots of a copy of `base`"""
    rng = np.random.default_rng(seed)
    x = base.copy()
    slots = rng.choice(x.size // 16 - 1, sum(c for _, c in segments), replace=False)
    at = 0
    for seg, copies in segments:
        seg = np.frombuffer(bytes(seg), dtype=np.uint8)
        for s in slots[at:at + copies]:
            x[16 * s:16 * s + seg.size] = seg
        at += copies
    return x


def _clusters(seed):
    """three 3-byte segments planted 7, 8 and 11 times: bins of 7, 8 and more than 8 words with distinct codes"""
    rng = np.random.default_rng(seed + 1000)
    segs = [(rng.integers(0, 256, 3, dtype=np.uint8).tobytes(), k) for k in (7, 8, 11)]
    return _planted(_uniform(65536, seed), segs, seed)


def _tie_in_big_bin(seed):
    """a 3-byte segment four times and a 12-byte one that starts with it twice: a bin of six or more with a tied pair"""
    rng = np.random.default_rng(seed + 2000)
    long = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
    return _planted(_uniform(65536, seed), [(long[:3], 4), (long, 2)], seed)


def _top_of_last_bucket(seed):
    """the largest symbol three times in a row, planted six times: the block's last bin"""
    return _planted(_uniform(65536, seed), [(b"\xff\xff\xff", 6)], seed)


def _one_tied_bucket(seed):
    """one 5-byte segment planted twice in uniform bytes (40 bits of a 36-bit code): the only equal codes of the block"""
    rng = np.random.default_rng(seed + 3000)
    return _planted(_uniform(65536, seed), [(rng.integers(0, 256, 5, dtype=np.uint8).tobytes(), 2)], seed)


SEED_ZIPF, SEED_CLUSTERS, SEED_TIE_BIG, SEED_LAST, SEED_ONE = 1, 0, 0, 0, 0


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _check(glc, ctx, x, rows=1):
    import torch
    n = x.size // rows
    want = [O.bwt(x[i * n:(i + 1) * n]) for i in range(rows)]
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros(x.size, dtype=torch.uint8, device=d_in.device)
    d_idx = torch.zeros(rows, dtype=torch.int32, device=d_in.device)
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, rows) == 0
        torch.cuda.synchronize()
        got, gidx = d_out.cpu().numpy(), d_idx.cpu().numpy()
        for i, (w, widx) in enumerate(want):
            assert int(gidx[i]) == widx, "block %d: BWT index" % i
            assert np.array_equal(got[i * n:(i + 1) * n], w), "block %d: BWT bytes" % i
        assert plan.last_flagged_blocks() == 0


def _sane(x):
    assert M.fills(x).max() <= M.FS_FILLMAX and M.longest_equal_run(x) <= M.FS_MAX_GROUP


def test_iid_bins_of_five_and_six(glc, ctx, cuda):
    """Zipf bytes, 128 buckets: flagged bins of 5 and 6 distinct codes in buckets of 3 and of 4 full rounds, and tied pairs
    in bins of at most four"""
    x = datagen.zipf_bytes(262144, seed=SEED_ZIPF)
    _sane(x)
    assert {5, 6} <= B.distinct_bin_sizes(x) and {3, 4} <= B.rounds_with_big_bin(x) and M.full_rounds(x) == {3, 4}
    assert min(B.tied_bin_sizes(x)) <= B.FSS_LOOK
    _check(glc, ctx, x)


def test_bins_of_seven_eight_and_more(glc, ctx, cuda):
    """the second look's last two sizes, and the loop behind it"""
    x = _clusters(SEED_CLUSTERS)
    _sane(x)
    sizes = B.distinct_bin_sizes(x)
    assert {7, 8} <= sizes and max(sizes) >= 9
    _check(glc, ctx, x)


def test_tied_pair_in_a_flagged_bin(glc, ctx, cuda):
    x = _tie_in_big_bin(SEED_TIE_BIG)
    _sane(x)
    assert any(5 <= s <= 8 for s in B.tied_bin_sizes(x))
    _check(glc, ctx, x)


def test_flagged_bin_in_front_of_the_sentinels(glc, ctx, cuda):
    """a bucket whose last non-empty bin has five or more words: the second look reads the sentinels"""
    x = _top_of_last_bucket(SEED_LAST)
    _sane(x)
    assert 5 <= B.last_bin_sizes(x)[-1] <= 8
    _check(glc, ctx, x)


def test_flagged_bins_in_the_guarded_body(glc, ctx, cuda):
    """buckets of 0-2 and 5-6 full rounds with bins of more than four"""
    x = _mixture(65536)
    _sane(x)
    assert B.rounds_with_big_bin(x) - {3, 4} and M.equal_code_pairs(x) > 0
    _check(glc, ctx, x)


def test_block_without_equal_codes(glc, ctx, cuda):
    """no workgroup has a work-list entry: every one of them leaves on its own counter"""
    x = _uniform(65536, 11)
    _sane(x)
    assert M.equal_code_pairs(x) == 0 and B.tie_buckets(x) == set()
    _check(glc, ctx, x)


def test_ties_in_a_single_bucket(glc, ctx, cuda):
    """one workgroup of the block reserves work-list entries, the others write none"""
    x = _one_tied_bucket(SEED_ONE)
    _sane(x)
    assert len(B.tie_buckets(x)) == 1 and M.equal_code_pairs(x) >= 1
    _check(glc, ctx, x)


def test_batch_of_four(glc, ctx, cuda):
    """per-block work-list counters: blocks with no ties, ties in one bucket, ties in many, and long bins, in one call"""
    blocks = [_uniform(65536, 11), _one_tied_bucket(SEED_ONE), _mixture(65536), _clusters(SEED_CLUSTERS)]
    for blk in blocks:
        _sane(blk)
    assert [len(B.tie_buckets(blk)) for blk in blocks[:2]] == [0, 1] and len(B.tie_buckets(blocks[2])) > 1
    _check(glc, ctx, np.concatenate(blocks), rows=4)
