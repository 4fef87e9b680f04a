"""The CHOOSE codec of the BWT container (INTEGRATION.md 4b "choose", csrc/choose_rule.h) in numpy and Python integers: the collision
statistic of the bigram probe (csrc/choose.hip), the rule, and a writer built from container_model's parts.  There is no new format
and no reader here: what write() makes is format version 3 and container_model.read(..., max_version=3) reads it.

  A segment x of L bytes; for 2 <= p < L, ctx(p) = (31 x[p-2] + x[p-1]) & 255 and sym(p) = x[p].  N[a][b] counts the p with ctx = a
  and sym = b, M = L - 2 (0 below two bytes), R and C are N's row and column sums, S2 = sum N (N - 1), SR = sum R (R - 1),
  SC = sum C (C - 1).  X = S2 M (M - 1) / (SR SC): observed collisions of (context, symbol) pairs over what independence gives.
  A block is BWT exactly when L >= MIN_LEN, SR > 0, SC > 0 and DEN S2 M (M - 1) >= NUM SR SC; every other block is order-0."""
import struct
import zlib

import numpy as np

import container_model as M

MIN_LEN = 2048
NUM, DEN = 3, 2
CODEC_CHOOSE = 4


def table(x):
    """N as an int64 array [256, 256]"""
    a = M._u8(x).reshape(-1).astype(np.int64)
    if a.size < 3:
        return np.zeros((256, 256), np.int64)
    key = (((31 * a[:-2] + a[1:-1]) & 255) << 8) | a[2:]
    return np.bincount(key, minlength=65536).astype(np.int64).reshape(256, 256)


def stats(x):
    """(S2, SR, SC, M) of one segment, Python integers"""
    L = M._u8(x).size
    N = table(x)
    R, C = N.sum(axis=1), N.sum(axis=0)
    pairs = lambda v: sum(int(k) * (int(k) - 1) for k in v[v > 1].tolist())   # noqa: E731
    return pairs(N.reshape(-1)), pairs(R), pairs(C), max(L - 2, 0)


def is_bwt(L, s):
    S2, SR, SC, m = s
    return L >= MIN_LEN and SR > 0 and SC > 0 and DEN * S2 * m * (m - 1) >= NUM * SR * SC


def X(x):
    """the statistic as a float (for tables; the rule never divides); nan where it is not defined"""
    S2, SR, SC, m = stats(x)
    return S2 * m * (m - 1) / (SR * SC) if SR and SC else float("nan")


def super_frames(n, block_len, rows):
    """[(pos, nb, bl)]: what is one frame with the other codecs -- up to `rows` blocks, the ragged tail on its own"""
    out, pos = [], 0
    while pos < n:
        left = n - pos
        nb, bl = (min(rows, left // block_len), block_len) if left >= block_len else (1, left)
        out.append((pos, nb, bl))
        pos += nb * bl
    return out


def plan(data, block_len, rows):
    """[(pos, nb, bl, kind)] of the frames the writer makes (kind: M.HUFF = the BWT codec, M.HUFF0 = the order-0 codec): every
    super-frame cut into its maximal runs of blocks of one choice"""
    a = M._u8(data).reshape(-1)
    frames = []
    for pos, nb, bl in super_frames(a.size, block_len, rows):
        pick = [M.HUFF if is_bwt(bl, stats(a[pos + i * bl: pos + (i + 1) * bl])) else M.HUFF0 for i in range(nb)]
        i = 0
        while i < nb:
            j = i + 1
            while j < nb and pick[j] == pick[i]:
                j += 1
            frames.append((pos + i * bl, j - i, bl, pick[i]))
            i = j
    return frames


def last_choice(data, block_len, rows):
    """glcContainerLastChoice: (blocks to the BWT codec, blocks to the order-0 codec, frames)"""
    p = plan(data, block_len, rows)
    return (sum(nb for _, nb, _, k in p if k == M.HUFF), sum(nb for _, nb, _, k in p if k == M.HUFF0), len(p))


def write(data, block_len, rows):
    """the container a writer plan with the CHOOSE codec makes of `data`"""
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    fmt = M.writer_format(0, M.CODEC_HUFF0)                       # version 3, no filter
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", fmt.version, fmt.flags, block_len, fmt.elem) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    frames = plan(a, block_len, rows)
    for pos, nb, bl, kind in frames:
        out.append(M._frame([a[pos + i * bl: pos + (i + 1) * bl] for i in range(nb)], bl, [kind] * nb))
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)
