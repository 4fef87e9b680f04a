"""Inputs of the dedup-mode tests and of tools/dedup_when.py: what frame-wide duplicate elimination is for, and where it loses."""
import numpy as np

import datagen

PAGE = 4096
NAMES = ("pages", "pages_noise", "zeros", "tar_like", "shifted", "text")


def _page(rng, noise):
    """one 4 KiB page: incompressible, or sixteen symbols of a skewed distribution"""
    if noise:
        return rng.integers(0, 256, PAGE, dtype=np.uint8)
    return rng.choice(16, PAGE, p=np.array([32, 16, 8, 8] + [3] * 12) / 100.0).astype(np.uint8)


def pages(n, seed=1, noise=False):
    """4 KiB pages; about half of them are drawn from a pool of 64 pages, so they repeat frame-wide, the others occur once"""
    rng = np.random.default_rng(seed)
    npg = (n + PAGE - 1) // PAGE
    pool = [_page(rng, noise) for _ in range(min(64, max(1, npg // 8)))]
    out = [pool[rng.integers(0, len(pool))] if rng.random() < 0.5 else _page(rng, noise) for _ in range(npg)]
    return np.concatenate(out)[:n]


def pages_noise(n, seed=2):
    return pages(n, seed, noise=True)


def zeros(n, seed=0):
    return np.zeros(n, np.uint8)


def tar_like(n, seed=3):
    """members of text behind 512-byte headers, every member padded to 512, some members stored twice"""
    rng = np.random.default_rng(seed)
    members, out, size = [], [], 0
    while size < n:
        if members and rng.random() < 0.4:
            m = members[rng.integers(0, len(members))]
        else:
            body = datagen.text_bytes(int(rng.integers(200, 20000)), seed=int(rng.integers(1, 1 << 30)))
            head = np.zeros(512, np.uint8)
            head[:100] = rng.integers(97, 123, 100, dtype=np.uint8)
            m = np.concatenate([head, body, np.zeros(-body.size % 512, np.uint8)])
            members.append(m)
        out.append(m)
        size += m.size
    return np.concatenate(out)[:n]


def shifted(n, seed=1):
    """the pages of `pages`, each shifted one byte further than the one in front of it (one byte of header per page).  Two copies
    of a page then lie at different offsets modulo 512 unless their page numbers differ by a multiple of 512, so below 512 pages
    (2 MiB) no chunk repeats another and the mode gains nothing; beyond that it finds about one repeat in 512."""
    p = pages(n, seed)
    p = np.concatenate([p, np.zeros(-p.size % PAGE, np.uint8)]).reshape(-1, PAGE)
    return np.concatenate([np.full((p.shape[0], 1), 0x5A, np.uint8), p], axis=1).reshape(-1)[:n]


def text(n, seed=4):
    return datagen.text_bytes(n, seed=seed)


GOLDEN = dict(block_len=481 * 512 + 100, rows=3, elem=8, delta=True)   # 482 chunks a block: 16 mask words, so E = 1 stays kind 2


def golden_input():
    """the input of tests/golden/dedup_v9_container.bin, built in the FILTERED domain (the input is what the inverse filter makes of
    each frame): two frames of three blocks and a ragged tail.
      frame 0   block 0 noise (raw; the source of what follows); block 1 mostly chunks of block 0, some chunks of its own with
                repeats among them, and block 0's short last chunk as its own; block 2 equal to block 0: nothing kept
      frame 1   block 0 sixteen skewed symbols (kind 2); block 1 the same kind of data with ONE chunk of block 0 in it (E = 1:
                kind 2 under the rule); block 2 a first half of its own and a second half that repeats it (sources in itself)
      tail      1636 bytes: chunk 1 repeats chunk 0"""
    import container_model as M
    import dedup_model as D
    bl = GOLDEN["block_len"]
    nch = D.nchunks(bl)
    fmt = D.stream_format(D.VERSION, M.FLAG_DELTA, GOLDEN["elem"])[0]
    rng = np.random.default_rng(909)

    def skewed(n):
        return rng.choice(16, n, p=np.array([940] + [4] * 15) / 1000.0).astype(np.uint8)

    a0 = rng.integers(0, 256, bl, dtype=np.uint8)
    a1 = a0.copy()
    for c in range(0, nch - 1, 7):                                 # chunks of its own, every third of them a repeat of the one before
        a1[512 * c:512 * c + 512] = skewed(512) if (c // 7) % 3 or c == 0 else a1[512 * (c - 7):512 * (c - 7) + 512]
    perm = rng.permutation(nch - 1)[:40]                           # and some of block 0's chunks at other places
    for k in range(0, 40, 2):
        if perm[k] % 7 and perm[k + 1] % 7:
            a1[512 * perm[k]:512 * perm[k] + 512] = a0[512 * perm[k + 1]:512 * perm[k + 1] + 512]
    b0, b1 = skewed(bl), skewed(bl)
    b1[512 * 5:512 * 6] = b0[512 * 9:512 * 10]
    b2 = skewed(bl)
    half = (nch // 2) * 512
    b2[half:] = b2[:bl - half]                                     # (its short last chunk is the head of a full one: kept)
    tail = skewed(1636)
    tail[512:1024] = tail[:512]
    frames = ([a0, a1, a0.copy()], [b0, b1, b2], [tail])
    x = np.concatenate([M.unfilter_frame(np.concatenate(f), fmt) for f in frames])
    x.setflags(write=False)
    return x


N, ROWS, TAIL = 8192 + 100, 8, 1235                              # the GPU container tests' plan: 17 chunks a block, the last of 100 bytes


def container_input(elem, delta):
    """the input of the GPU container tests, built in the FILTERED domain: with a plan of n = N and ROWS rows,
      frame 0   0 noise (raw); 1, 2 skewed symbols (kind 2); 3 = block 0: nothing kept; 4 its own chunks, chunks of block 1 (sources
                three blocks earlier, the short last chunk among them) and a repeat of one of its own; 5 a repeat inside itself only;
                6 noise; 7 chunks of block 6 (sources in a raw block) among its own
      frame 1   0 = frame 0's block 1 (kept whole: sources never cross a frame); 1 = block 0; the rest skewed symbols
      frame 2   two blocks, the second the first again
      tail      TAIL bytes whose chunk 1 repeats chunk 0"""
    import container_model as M
    import dedup_model as D
    fmt = D.stream_format(D.VERSION, M.FLAG_DELTA if delta else 0, 0 if elem == 1 else elem)[0]
    rng = np.random.default_rng(500 + elem + (50 if delta else 0))

    def skewed(n):
        return rng.choice(16, n, p=np.array([40, 20, 10, 6] + [2] * 12) / 100.0).astype(np.uint8)

    def put(dst, c, src, sc):
        dst[512 * c:512 * c + 512] = src[512 * sc:512 * sc + 512]

    a = [rng.integers(0, 256, N, dtype=np.uint8), skewed(N), skewed(N), None, skewed(N), skewed(N), rng.integers(0, 256, N, dtype=np.uint8), skewed(N)]
    a[3] = a[0].copy()
    for c, sc in ((1, 5), (2, 0), (7, 7), (12, 15)):
        put(a[4], c, a[1], sc)
    a[4][512 * 16:] = a[1][512 * 16:]
    put(a[4], 9, a[4], 3)
    put(a[5], 10, a[5], 2)
    put(a[5], 11, a[5], 2)
    for c in (0, 4, 5, 13):
        put(a[7], c, a[6], c + 1)
    b = [a[1].copy(), a[1].copy()] + [skewed(N) for _ in range(ROWS - 2)]
    c0 = skewed(N)
    tail = skewed(TAIL)
    tail[512:1024] = tail[:512]
    x = np.concatenate([M.unfilter_frame(np.concatenate(f), fmt) for f in (a, b, [c0, c0.copy()], [tail])])
    x.setflags(write=False)
    return x


def make(name, n):
    x = globals()[name](n)
    assert x.size == n and x.dtype == np.uint8
    return x
