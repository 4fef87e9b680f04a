"""NumPy model of the BIN a suffix goes to inside its bucket in k_fs_sort_bwt (csrc/bwt_bucket.hip), on top of
fs_fill_model's codes and buckets: the 12 bits of X below the bucket number,

    bin = (X >> (64 - nbl - 12)) & 4095,

and what the kernel's rank step makes of a bin's occupancy: a bin of more than FSS_LOOK = 4 words is flagged by the
words that arrive fifth and later, its words take the rare path's second look (up to 8 words) or its loop (9 and more);
words with equal 36-bit codes ("ties") take the rare path whatever their bin's size and go to the block's work list."""
import numpy as np

from fs_fill_model import FSS_NT, bucket_log2, codes

FS_BIN_BITS, FSS_LOOK = 12, 4


def bin_of(x):
    """bin of every suffix of the block inside its bucket"""
    nbl = bucket_log2(x.size)
    return ((codes(x) >> np.uint64(64 - nbl - FS_BIN_BITS)) & np.uint64((1 << FS_BIN_BITS) - 1)).astype(np.int64)


def occupancy(x):
    """words per (bucket, bin), [1 << nbl][4096]"""
    nbl = bucket_log2(x.size)
    gb = (codes(x) >> np.uint64(64 - nbl - FS_BIN_BITS)).astype(np.int64)
    return np.bincount(gb, minlength=1 << (nbl + FS_BIN_BITS)).reshape(1 << nbl, 1 << FS_BIN_BITS)


def tied_per_bin(x):
    """words per (bucket, bin) that share their 36-bit code with another word, [1 << nbl][4096]"""
    nbl = bucket_log2(x.size)
    k = np.sort(codes(x) >> np.uint64(28))
    same = k[1:] == k[:-1]
    tied = np.concatenate([[False], same]) | np.concatenate([same, [False]])
    gb = (k[tied] >> np.uint64(36 - nbl - FS_BIN_BITS)).astype(np.int64)
    return np.bincount(gb, minlength=1 << (nbl + FS_BIN_BITS)).reshape(1 << nbl, 1 << FS_BIN_BITS)


def distinct_bin_sizes(x):
    """sizes of the bins of more than FSS_LOOK words whose codes are all different"""
    occ, tied = occupancy(x), tied_per_bin(x)
    return set(occ[(occ > FSS_LOOK) & (tied == 0)].tolist())


def tied_bin_sizes(x):
    """sizes of the bins that hold at least one pair of equal codes"""
    occ, tied = occupancy(x), tied_per_bin(x)
    return set(occ[tied > 0].tolist())


def tie_buckets(x):
    """the buckets that hold words with equal codes"""
    return set(np.flatnonzero(tied_per_bin(x).sum(axis=1)).tolist())


def last_bin_sizes(x):
    """size of the last non-empty bin of every non-empty bucket: what the rank step reads behind it are the sentinels"""
    occ = occupancy(x)
    out = []
    for row in occ[occ.sum(axis=1) > 0]:
        out.append(int(row[np.flatnonzero(row)[-1]]))
    return out


def rounds_with_big_bin(x):
    """c // 512 of the buckets that have a bin of more than FSS_LOOK words"""
    occ = occupancy(x)
    big = (occ > FSS_LOOK).any(axis=1)
    return set((occ.sum(axis=1)[big] // FSS_NT).tolist())
