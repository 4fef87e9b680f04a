"""k_fs_sort_bwt's instances (csrc/bwt_bucket.hip): a bucket of c words runs c // 512 full rounds, and the kernel has a
straight-line body for 3 and for 4 of them and the eight-slot guarded body for every other count.  Which counts a block's
buckets take is a property of the input: every test asserts it with the CPU model (fs_fill_model.py) BEFORE the GPU call,
so a case cannot drift off the instance it is there for.  Results are compared byte for byte and index for index with the
oracle.

The model's figures for the inputs below (n, buckets, fills, c // 512):
    zipf 4000      16   237-258    0                    zipf 32768     16  2003-2099   3, 4   (two buckets with c % 512 == 0)
    zipf 16384     16   990-1054   1, 2  (one such)     zipf 65536     32  1995-2133   3, 4
    zipf 24576     16  1490-1563   2, 3  (three)        mixture 65536  32   444-3501   0-6, 33 pairs of equal 36-bit codes
c // 512 == 7 (3584-4031 words, the guarded body's last slot): the mixture with int(0.55 n) bytes of the small alphabet has
buckets of every count 0-7 with its fullest at 3768 words, under the 4032 past which a block goes to another tier."""
import numpy as np
import pytest

import datagen
import fs_fill_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _bwt(glc, plan, torch, x, rows=1):
    n = x.size // rows
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros(x.size, dtype=torch.uint8, device=d_in.device)
    d_idx = torch.zeros(rows, dtype=torch.int32, device=d_in.device)
    assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, rows) == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_idx.cpu().numpy()


def _zipf(n, seed=None):
    return datagen.zipf_bytes(n, seed=n if seed is None else seed)


def _mixture(n, share=0.6):
    """the first int(share n) bytes from 8 symbols, the rest from 256: narrow and wide symbol intervals in one table, so
    buckets from nearly empty to nearly full"""
    rng = np.random.default_rng(3)
    k = int(share * n)
    return np.concatenate([rng.integers(0, 8, k, dtype=np.uint8), rng.integers(0, 256, n - k, dtype=np.uint8)])


def _planted(base, seg_len, copies, seed):
    """one random segment planted `copies` times: suffixes inside the copies tie for up to seg_len bytes"""
    rng = np.random.default_rng(seed)
    x = base.copy()
    seg = rng.integers(0, 256, seg_len, dtype=np.uint8)
    for p in rng.choice((x.size - seg_len) // seg_len, copies, replace=False):
        x[p * seg_len:(p + 1) * seg_len] = seg
    return x


# name: (generator, c // 512 over the buckets, buckets with c % 512 == 0, (lowest, highest) fill)
CASES = {
    "zipf_4000": (lambda: _zipf(4000), {0}, 0, (237, 258)),
    "zipf_16384": (lambda: _zipf(16384), {1, 2}, 1, (990, 1054)),
    "zipf_24576": (lambda: _zipf(24576), {2, 3}, 3, (1490, 1563)),
    "zipf_32768": (lambda: _zipf(32768), {3, 4}, 2, (2003, 2099)),
    "zipf_65536": (lambda: _zipf(65536), {3, 4}, 2, (1995, 2133)),
    "mixture_65536": (lambda: _mixture(65536), {0, 1, 2, 3, 4, 5, 6}, 0, (444, 3501)),
    "mixture_full7_65536": (lambda: _mixture(65536, 0.55), {0, 1, 2, 3, 4, 5, 6, 7}, 0, None),
}


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _check(glc, ctx, x, rows=1, flagged=0):
    import torch
    n = x.size // rows
    want = [O.bwt(x[i * n:(i + 1) * n]) for i in range(rows)]
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        got, gidx = _bwt(glc, plan, torch, x, rows=rows)
        for i, (w, widx) in enumerate(want):
            assert int(gidx[i]) == widx, "block %d: BWT index" % i
            assert np.array_equal(got[i * n:(i + 1) * n], w), "block %d: BWT bytes" % i
        assert plan.last_flagged_blocks() == flagged


@pytest.mark.parametrize("name", list(CASES.keys()))
def test_rounds_per_bucket(glc, ctx, cuda, name):
    gen, rounds, no_partial, span = CASES[name]
    x = gen()
    f = M.fills(x)
    assert M.full_rounds(x) == rounds and M.partial_free(x) == no_partial and f.max() <= M.FS_FILLMAX
    if span:
        assert (int(f[f > 0].min()), int(f.max())) == span
    if name == "mixture_65536":
        assert M.equal_code_pairs(x) == 33                     # the tie path, from buckets of every instance
    _check(glc, ctx, x)


def test_ties_inside_the_straight_line_instances(glc, ctx, cuda):
    """work-list entries from buckets of 3 and 4 full rounds only"""
    x = _planted(_zipf(32768), 40, 16, 5)
    assert M.full_rounds(x) == {3, 4} and M.fills(x).max() <= M.FS_FILLMAX
    assert M.equal_code_pairs(x) >= 16 * 30 and M.longest_equal_run(x) <= M.FS_MAX_GROUP
    _check(glc, ctx, x)


def test_run_of_equal_codes_flags_the_block(glc, ctx, cuda):
    """more than 512 equal codes in one bin: the straight-line instance leaves through s_deep and another tier sorts the block"""
    x = _zipf(32768).copy()
    x[10000:10600] = x[10000]
    assert M.full_rounds(x) == {3, 4} and M.fills(x).max() <= M.FS_FILLMAX
    assert M.longest_equal_run(x) > M.FS_MAX_GROUP
    _check(glc, ctx, x, flagged=1)


def test_batch_of_four(glc, ctx, cuda):
    """the block index in the workgroup order, and rows that start at all four alignments of the output pointer"""
    blocks = [_zipf(32768, seed=s) for s in (1, 2, 3, 4)]
    starts = set()
    for blk in blocks:
        f = M.fills(blk)
        assert M.full_rounds(blk) == {3, 4} and f.max() <= M.FS_FILLMAX
        starts |= set(((np.cumsum(f) - f) % 4).tolist())
    assert starts == {0, 1, 2, 3}
    _check(glc, ctx, np.concatenate(blocks), rows=4)
