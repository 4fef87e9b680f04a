"""What a workgroup of k_fs_sort_bwt does once (csrc/bwt_bucket.hip): its place in the grid by shift and mask -- right only
if the grid's x size is the 1 << nbl the kernel is told --, the one batch of scalar loads (the block's flag, the bucket's
fill and rank base, the block's zero bucket), the initial value of s_deep, and bin_starts() on packed halves.  Every
result is compared byte for byte and index for index with the oracle; the one-block shapes also as a suffix array
(cudppSuffixArray, which runs k_fs_sort on the same buckets).  Properties of an input a case stands on -- bucket count,
fills, crowded bins, tied words, the bucket of suffix 0, the longest run of equal codes -- are asserted with the CPU model
(fs_fill_model.py) before the GPU call."""
import numpy as np
import pytest

import datagen
import fs_fill_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

# one n for every bucket count the host can choose, nbl = 4 .. 9 (the next count starts behind FS_AVG << nbl bytes;
# test_shapes_cover_every_bucket_count asks the library's own fs_bucket_log2 about every n and every threshold, so a change
# to the host's rule fails there and does not pass as a stale table): alternately near the top of the count's range
# (buckets of ~2048 words: the instances of 3 and 4 full rounds) and just behind its lower threshold (~1024 words: the
# guarded body), and 1 MiB
SHAPES = {4: (M.FS_AVG << 4) - 19, 5: (M.FS_AVG << 4) + 13, 6: (M.FS_AVG << 6) - 7, 7: (M.FS_AVG << 6) + 5,
          8: (M.FS_AVG << 8) - 11, 9: 1 << 20}
ROWS = (1, 5, 17)                                              # one tile per workgroup / four / the batch form; 5 and 17: a grid y
                                                               # that is no power of two and no multiple of 8

_want = {}                                                     # (n, seed) -> (block, BWT, index): computed once


def _zipf_block(n, seed):
    if (n, seed) not in _want:
        x = datagen.zipf_bytes(n, seed=seed)
        _want[(n, seed)] = (x,) + O.bwt(x)
    return _want[(n, seed)]


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _bwt(glc, ctx, blocks):
    """one glcBwtBatch call over equally long blocks: (BWT rows, indices, last_sort_stats())"""
    import torch
    n, rows = blocks[0].size, len(blocks)
    d_in = torch.from_numpy(np.ascontiguousarray(np.concatenate(blocks))).cuda()
    d_out = torch.zeros(rows * n, dtype=torch.uint8, device=d_in.device)
    d_idx = torch.full((rows,), -1, dtype=torch.int32, device=d_in.device)
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, rows) == 0
        torch.cuda.synchronize()
        stats = plan.last_sort_stats()
    return d_out.cpu().numpy().reshape(rows, n), d_idx.cpu().numpy(), stats


def _exact(blocks, got, gidx, want=None):
    for i, blk in enumerate(blocks):
        w, widx = want[i] if want else O.bwt(blk)
        assert int(gidx[i]) == widx, "block %d of %d, n = %d: BWT index" % (i, len(blocks), blk.size)
        assert np.array_equal(got[i], w), "block %d of %d, n = %d: BWT bytes" % (i, len(blocks), blk.size)


def _host_bucket_log2(glc):
    """the host's fs_bucket_log2 (csrc/bwt_bucket.hip), the function the launch takes nbl and the grid's x size from.  It is
    C++ with no entry in the C headers: the library exports it under its mangled name, glc::fs_bucket_log2(unsigned int)."""
    import ctypes as C
    f = getattr(glc.lib(), "_ZN3glc14fs_bucket_log2Ej")
    f.argtypes, f.restype = [C.c_uint32], C.c_uint32
    return f


def test_shapes_cover_every_bucket_count(glc):
    log2 = _host_bucket_log2(glc)
    assert [log2(n) for n in SHAPES.values()] == list(SHAPES.keys()) == list(range(4, M.FS_MAXNB_LOG2 + 1))
    assert log2(1) == 4 and log2(0xFFFFFFFF) == M.FS_MAXNB_LOG2    # no count below the first or above the last
    for l in SHAPES:                                           # the thresholds, from the function
        assert log2(M.FS_AVG << l) == l and (l == M.FS_MAXNB_LOG2 or log2((M.FS_AVG << l) + 1) == l + 1)
    for n in list(SHAPES.values()) + [40000, 65536]:           # ... and the model the other cases stand on follows it
        assert M.bucket_log2(n) == log2(n)
    assert SHAPES[9] == 1 << 20


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nbl", list(SHAPES.keys()))
def test_bucket_counts_and_launch_shapes(glc, ctx, cuda, nbl, rows):
    n = SHAPES[nbl]
    recs = [_zipf_block(n, 100 * nbl + i) for i in range(rows)]
    blocks = [r[0] for r in recs]
    got, gidx, stats = _bwt(glc, ctx, blocks)
    _exact(blocks, got, gidx, want=[r[1:] for r in recs])
    assert stats == (0, 0)                                     # every block finished by the bucket sorter


@pytest.mark.parametrize("nbl", list(SHAPES.keys()))
def test_suffix_array_of_one_block(glc, ctx, cuda, nbl):
    import torch
    n = SHAPES[nbl]
    x = _zipf_block(n, 100 * nbl)[0]
    want = O.suffix_array(x)
    with glc.Plan(ctx, glc.CUDPP_SA, n) as plan:
        d_out = torch.zeros(n + 1, dtype=torch.int32, device=cuda)
        assert glc.lib().cudppSuffixArray(plan.handle, torch.from_numpy(x).cuda().data_ptr(), d_out.data_ptr(), n) == 0
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(np.uint32)
        assert plan.last_flagged_blocks() == 0
    assert got[0] == n and np.array_equal(got[1:], want)


def test_blocks_flagged_before_the_kernel_starts(glc, ctx, cuda):
    """blocks 0 and 2 of 5 are not the bucket sorter's before k_fs_sort_bwt starts: a text-like block (flagged by
    k_fs_tables: its workgroups leave on the scalar load) and a constant block (finished by k_fs_tables, no tier's
    business).  One block goes on to the sample sorter, which finishes it: (1, 0), as before the entry was rebuilt."""
    n = 1 << 20
    blocks = [datagen.text_bytes(n, seed=2), _zipf_block(n, 900)[0], np.full(n, 0x55, dtype=np.uint8),
              _zipf_block(n, 901)[0], _zipf_block(n, 902)[0]]
    got, gidx, stats = _bwt(glc, ctx, blocks)
    assert stats == (1, 0), stats
    _exact(blocks, got, gidx)


def test_block_flagged_by_a_bucket_while_the_kernel_runs(glc, ctx, cuda):
    """600 equal bytes inside Zipf bytes in block 2 of 5: more than FS_MAX_GROUP suffixes share one code, the bucket that
    holds them flags the block through s_deep and the next tier sorts it.  What this can check of s_deep's INITIAL value
    (the second read of the flag) is one direction only: a value that is wrongly non-zero -- another block's flag, a stale
    register -- makes buckets of the four clean blocks leave, and then either more than one block is handed on or a row is
    wrong.  That the later buckets of block 2 see the flag and skip their sort changes no result (the kernel's comment says
    why), so a constant 0 would pass here: that half is a matter of time, not of output."""
    n = 65536
    blocks = [_zipf_block(n, 910 + i)[0] for i in range(5)]
    blocks[2] = blocks[2].copy()
    blocks[2][10000:10600] = blocks[2][10000]
    assert M.longest_equal_run(blocks[2]) > M.FS_MAX_GROUP and M.fills(blocks[2]).max() <= M.FS_FILLMAX
    for i in (0, 1, 3, 4):
        assert M.longest_equal_run(blocks[i]) <= M.FS_MAX_GROUP
    got, gidx, stats = _bwt(glc, ctx, blocks)
    assert stats[0] == 1, stats
    _exact(blocks, got, gidx)


def _four_symbols(n):
    return np.random.default_rng(41).choice(np.array([3, 70, 71, 200], dtype=np.uint8), n)


def _mixture(n, share=0.6):
    """the first int(share n) bytes from 8 symbols, the rest from 256 (as in test_gpu_sort_rounds.py): narrow and wide symbol
    intervals in one table, so buckets from nearly empty to full and hundreds of crowded bins, with next to no equal codes"""
    rng = np.random.default_rng(3)
    k = int(share * n)
    return np.concatenate([rng.integers(0, 8, k, dtype=np.uint8), rng.integers(0, 256, n - k, dtype=np.uint8)])


def _planted(base, seg_len, copies, seed):
    """one random segment planted `copies` times: the suffixes inside the copies share their codes, `copies` words to a bin"""
    rng = np.random.default_rng(seed)
    x = base.copy()
    seg = rng.integers(0, 256, seg_len, dtype=np.uint8)
    for p in rng.choice((x.size - seg_len) // seg_len, copies, replace=False):
        x[p * seg_len:(p + 1) * seg_len] = seg
    return x


def _big_bins(x):
    """bins (12 bits below the bucket number) that hold more than four words: the ones whose start entry gets the flag"""
    nbl = M.bucket_log2(x.size)
    return int(np.count_nonzero(np.bincount((M.codes(x) >> np.uint64(64 - nbl - 12)).astype(np.int64)) > 4))


def _tied_words(x):
    """words in runs of equal 36-bit codes: each takes an entry of the block's work list, which holds max(1024, n / 8); a
    block with more is flagged by wl_base() and sorted again by the next tier"""
    k = np.sort(M.codes(x) >> np.uint64(28))
    d = np.diff(np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1], [True]])))
    return int(d[d > 1].sum())


def _probe_repeats_at_most(x):
    """upper bound of what k_fs_hist's 6-gram probe counts in a block that starts 16-byte aligned (any other start: it
    does not look): per 32 KB slice, vectors 0 .. 255 and 1024 .. 1279 give a fingerprint of their first six bytes, and a
    sample is a repeat if the slot it hashes to holds its fingerprint already.  Which of two different fingerprints takes
    a shared slot is a race; samples minus distinct fingerprints bounds the count whatever the order.  FS_DUP_FLAG = 48
    repeats flag the block as text-like before k_fs_sort_bwt starts."""
    tot = 0
    for lo in range(0, x.size, 32768):
        s = x[lo:lo + 32768]
        nvec = s.size // 16
        idx = [i for i in list(range(256)) + list(range(1024, 1280)) if i < nvec]
        v = s[:nvec * 16].reshape(nvec, 16)[idx].astype(np.uint32)
        w0 = v[:, 0] | v[:, 1] << 8 | v[:, 2] << 16 | v[:, 3] << 24
        w1 = v[:, 4] | v[:, 5] << 8
        fp = (w0 * np.uint32(0x9E3779B1) + w1 * np.uint32(0x85EBCA6B)) | np.uint32(1)
        tot += fp.size - np.unique(fp).size
    return tot


FS_DUP_FLAG = 48

# name: (generator, c // 512 over the buckets, (lowest, highest) fill, bins of more than FSS_LOOK = 4 words, tied words).
# bin_starts() for counts far from 2048, with crowded bins, in blocks that STAY with the bucket sorter (the model says so
# before the call -- no text-like flag, the work list not full, no run past FS_MAX_GROUP -- and last_sort_stats() after it), so
# the rows compared are the ones laid out from bin_starts()' starts.  40 000 bytes are 32 buckets of ~1250 words: two full
# rounds, the guarded body.  The mixture has buckets of 239 to 2144 words, every instance in one block.  65 536 bytes with
# the same planted segment: crowded bins in the instances of 3 and 4 full rounds.
FILLS = {
    "zipf_40000": (lambda: datagen.zipf_bytes(40000, seed=40000), {2}, (1212, 1297), 2, 0),
    "planted_40000": (lambda: _planted(datagen.zipf_bytes(40000, seed=40000), 100, 6, 7), {2}, (1170, 1316), 102, 584),
    "mixture_40000": (lambda: _mixture(40000), {0, 1, 2, 3, 4}, (239, 2144), 624, 12),
    "planted_65536": (lambda: _planted(datagen.zipf_bytes(65536, seed=65536), 100, 6, 7), {3, 4}, (1996, 2126), 115, 584),
}


@pytest.mark.parametrize("name", list(FILLS.keys()))
def test_fills_far_from_2048(glc, ctx, cuda, name):
    gen, rounds, span, big, tied = FILLS[name]
    x = gen()
    f = M.fills(x)
    assert M.full_rounds(x) == rounds and (int(f[f > 0].min()), int(f.max())) == span and f.max() <= M.FS_FILLMAX
    assert _big_bins(x) == big and _tied_words(x) == tied <= max(1024, x.size // 8)
    assert _probe_repeats_at_most(x) < FS_DUP_FLAG and M.longest_equal_run(x) <= M.FS_MAX_GROUP
    got, gidx, stats = _bwt(glc, ctx, [x])
    assert stats == (0, 0), stats                              # finished by the bucket sorter: these ARE k_fs_sort_bwt's rows
    _exact([x], got, gidx)


@pytest.mark.parametrize("n", [40000, 65536])
def test_four_symbol_block_is_handed_on(glc, ctx, cuda, n):
    """four symbols give eight of them 16 bits of code: tens of thousands of words with equal codes, several times what the
    block's work list holds.  k_fs_sort_bwt sorts every bucket (guarded body at 40 000 bytes, 3 and 4 full rounds at 65 536),
    the reservation that passes the list's end flags the block, and the next tier's rows are the ones compared: what this
    checks of the kernel is that it hands such a block on and writes nothing outside its rows, not bin_starts()."""
    x = _four_symbols(n)
    assert M.fills(x).max() <= M.FS_FILLMAX and _tied_words(x) > 2 * max(1024, n // 8)
    got, gidx, stats = _bwt(glc, ctx, [_zipf_block(n, 930)[0], x, _zipf_block(n, 931)[0]])
    assert stats[0] == 1, stats
    _exact([_zipf_block(n, 930)[0], x, _zipf_block(n, 931)[0]], got, gidx)


@pytest.mark.parametrize("where", ["first", "last"])
def test_bucket_of_suffix_0(glc, ctx, cuda, where):
    """suffix 0 in bucket 0 and in the last bucket: the one bucket that looks for the BWT index (zero_bucket, d_index)"""
    n = 65536
    x = _zipf_block(n, 920)[0].copy()
    x[:8] = x.min() if where == "first" else x.max()
    x[-1] = x.max()                                            # (both ends of the alphabet are in the block)
    nb = 1 << M.bucket_log2(n)
    assert int(M.codes(x)[0] >> np.uint64(64 - M.bucket_log2(n))) == (0 if where == "first" else nb - 1)
    blocks = [_zipf_block(n, 921)[0], x, _zipf_block(n, 922)[0]]
    got, gidx, stats = _bwt(glc, ctx, blocks)
    assert stats == (0, 0)
    _exact(blocks, got, gidx)
