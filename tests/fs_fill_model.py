"""NumPy model of the bucket a suffix goes to in the bucket sorter (csrc/bwt_bucket.hip): which of k_fs_sort_bwt's
instances a block's buckets take is a property of the input, and a test asserts it before it calls the GPU.

    {C, p}   as k_fs_tables builds them with step = 1 (the block's own histogram; hstep is 1 under 16 slices of 32 KB, so
             this holds for every n below 480 KiB): floor(2^32 * exclusive cumulative count / n), floor(2^32 * count / n)
    X        the 8-symbol recurrence of k_fs_part2, symbols past the end of the block contributing C = p = 0:
             y7 = C[s7];  y_d = C[s_d] + floor(p[s_d] * y_{d+1} / 2^32)  (d = 6..1);  X = C[s0] * 2^32 + p[s0] * y1
    bucket   X >> (64 - nbl),  nbl = fs_bucket_log2(n)

A bucket of c words runs c // 512 full rounds and one partial round of c % 512 words."""
import numpy as np

FS_DEPTH, FS_AVG, FS_MAXNB_LOG2, FS_FILLMAX, FSS_NT, FS_MAX_GROUP = 8, 2048, 9, 4032, 512, 512
MAX_N = 15 * 32768                                             # 16 slices and more: k_fs_hist samples (step > 1)


def bucket_log2(n):
    l = 4
    while (FS_AVG << l) < n and l < FS_MAXNB_LOG2:
        l += 1
    return l


def tables(x):
    h = np.bincount(x, minlength=256).astype(np.uint64)
    c = np.cumsum(h) - h
    n = np.uint64(x.size)
    lim = np.uint64(0xFFFFFFFF)
    return np.minimum((c << np.uint64(32)) // n, lim), np.minimum((h << np.uint64(32)) // n, lim)


def codes(x):
    """X of every suffix of the block, as uint64"""
    assert 0 < x.size < MAX_N and x.dtype == np.uint8
    C, P = tables(x)
    n = x.size
    pad = np.concatenate([x.astype(np.int64), np.full(FS_DEPTH, 256, dtype=np.int64)])   # 256: past the end
    C = np.concatenate([C, np.zeros(1, dtype=np.uint64)])
    P = np.concatenate([P, np.zeros(1, dtype=np.uint64)])
    sym = [pad[d:d + n] for d in range(FS_DEPTH)]
    y = C[sym[FS_DEPTH - 1]]
    for d in range(FS_DEPTH - 2, 0, -1):
        y = C[sym[d]] + ((P[sym[d]] * y) >> np.uint64(32))     # < 2^32: C[s] + p[s] <= C[s + 1]
    return (C[sym[0]] << np.uint64(32)) + P[sym[0]] * y


def fills(x):
    """words per bucket, [1 << nbl]"""
    nbl = bucket_log2(x.size)
    return np.bincount((codes(x) >> np.uint64(64 - nbl)).astype(np.int64), minlength=1 << nbl)


def full_rounds(x):
    """the set of c // 512 over the block's non-empty buckets"""
    f = fills(x)
    return set((f[f > 0] // FSS_NT).tolist())


def partial_free(x):
    """buckets whose fill is a positive multiple of 512: no partial round"""
    f = fills(x)
    return int(np.count_nonzero((f > 0) & (f % FSS_NT == 0)))


def equal_code_pairs(x):
    """pairs of neighbours, in code order, with equal top 36 bits of X: what the sorter hands to k_fs_ties"""
    k = np.sort(codes(x) >> np.uint64(28))
    return int(np.count_nonzero(k[1:] == k[:-1]))


def longest_equal_run(x):
    """most suffixes that share one 36-bit code (more than FS_MAX_GROUP of them in a bin: the block is flagged)"""
    k = np.sort(codes(x) >> np.uint64(28))
    edge = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1], [True]]))
    return int(np.diff(edge).max())
