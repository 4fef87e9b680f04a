"""Blocks for the chain-group tests (tests/test_gpu_chains.py, tests/test_gpu_chains_sa.py): periodic regions, stretches inside
ordinary data, either direction of a chain's exit, arithmetic progressions that are not chains, random mosaics of periodic
pieces, and blocks at the strides and lengths the kernels branch on.  Test infrastructure, never imported by the product."""
import numpy as np

import datagen


def regions(n, rng, periods, alphabet):
    """len(periods) periodic regions of (about) equal length, random words over `alphabet`"""
    cuts = [n * k // len(periods) for k in range(len(periods) + 1)]
    x = np.empty(n, dtype=np.uint8)
    for k, p in enumerate(periods):
        w = rng.choice(np.asarray(alphabet, dtype=np.uint8), size=p)
        m = cuts[k + 1] - cuts[k]
        x[cuts[k]:cuts[k + 1]] = np.tile(w, m // p + 1)[:m]
    return x


REGION_KINDS = (((3, 5), [0, 1]), ((7, 7), [1, 2, 3]), ((1, 2), [0, 255]), ((40, 300), list(range(256))), ((17, 4, 90), [5, 6, 7, 8]),
                ((400, 2, 31, 31), list(range(97, 123))), ((5000, 3), list(range(256))), ((2, 2, 2), [0, 1]))


def region_blocks(seed, n=1 << 17):
    """two and more periodic regions: every kind of REGION_KINDS once"""
    rng = np.random.default_rng(9000 + seed)
    return [regions(n, rng, periods, al) for periods, al in REGION_KINDS]


def stretch_blocks(n=1 << 18):
    """periodic stretches and runs inside ordinary data"""
    rng = np.random.default_rng(77)
    z = datagen.zipf_bytes(n, seed=5).copy()
    t = datagen.text_bytes(n, seed=6).copy()
    a = z.copy(); a[50000:150000] = np.tile(rng.integers(0, 256, 37, dtype=np.uint8), 100000 // 37 + 1)[:100000]
    b = t.copy(); b[100000:180000] = 32                           # a run of blanks inside text (d = 1)
    c = z.copy(); c[n - 70000:] = np.tile(np.frombuffer(b"xyz", dtype=np.uint8), 70000 // 3 + 1)[:70000]   # a stretch up to the end of the block
    d = t.copy(); d[:90000] = 0; d[200000:260000] = np.tile(np.frombuffer(b"ab", dtype=np.uint8), 30000)
    e = z.copy()                                                  # the same pattern twice, far apart: groups hold two chains until the doubling separates them
    w = rng.integers(0, 256, 29, dtype=np.uint8)
    e[20000:60000] = np.tile(w, 40000 // 29 + 1)[:40000]
    e[150000:200000] = np.tile(w, 50000 // 29 + 1)[:50000]
    return [a, b, c, d, e]


def direction_blocks(n=1 << 17):
    """the symbol behind the stretch smaller / larger than the one the period would continue with; the stretch ending the block"""
    blocks = []
    for nxt in (0, 255):
        x = np.tile(np.frombuffer(b"mnop", dtype=np.uint8), n // 4).copy()
        x[n // 2:] = nxt
        x[n - 1] = 7
        blocks.append(x)
    y = np.tile(np.frombuffer(b"mnop", dtype=np.uint8), n // 4).copy()
    y[:1000] = np.arange(1000, dtype=np.uint32).astype(np.uint8)
    blocks.append(y)
    return blocks


def full_size_blocks(n=1 << 20):
    """bench.py's two_regions kinds at 1 MiB: two periodic halves, a 256 KiB stretch inside Zipf data"""
    rng = np.random.default_rng(11)
    h = regions(n, rng, (211, 97), list(range(256)))
    z = datagen.zipf_bytes(n, seed=9).copy()
    z[300000:300000 + 262144] = np.tile(rng.integers(0, 256, 123, dtype=np.uint8), 262144 // 123 + 1)[:262144]
    return [h, z]


def not_chain_blocks(n=1 << 17):
    """groups whose members ARE an arithmetic progression with a stride the chain pass tries (<= 4096) but whose text is not
    periodic over it: a 600-byte phrase every 2048 bytes with different random bytes in between; a periodic stretch with ONE byte
    changed in its middle (every residue class still has a member every d bytes across the defect); two stretches of one pattern
    a whole number of periods apart (each stretch on its own holds true chains)"""
    rng = np.random.default_rng(31)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    phrase = rng.integers(97, 123, 600, dtype=np.uint8)
    for o in range(1000, n - 700, 2048):
        a[o:o + 600] = phrase
    w = rng.integers(0, 4, 23, dtype=np.uint8)
    b = np.tile(w, n // 23 + 1)[:n].copy()
    b[n // 2 + 7] ^= 1
    c = rng.integers(0, 256, n, dtype=np.uint8)
    w2 = rng.integers(0, 256, 50, dtype=np.uint8)
    c[10000:30000] = np.tile(w2, 400)
    c[30000 + 50 * 100:30000 + 50 * 100 + 20000] = np.tile(w2, 400)      # the same phase, 100 periods of other bytes in between
    return [a, b, c]


def large_mosaic_blocks(seed, count=12):
    """blocks glued from random pieces -- periodic stretches of random period and alphabet, runs, random bytes, copies of earlier
    pieces -- of one length drawn from the seed (64 KiB .. 200 000)"""
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.choice([1 << 16, (1 << 16) + 123, 1 << 17, 200000]))
    blocks = []
    for _ in range(count):
        x = np.empty(n, dtype=np.uint8)
        o = 0
        pieces = []
        while o < n:
            kind = int(rng.integers(0, 5))
            m = int(min(n - o, rng.integers(50, n // 2)))
            if kind == 0:
                p = int(rng.integers(1, 600))
                al = int(rng.choice([2, 3, 4, 26, 256]))
                seg = np.tile(rng.integers(0, al, p, dtype=np.uint8), m // p + 1)[:m]
            elif kind == 1:
                seg = np.full(m, int(rng.integers(0, 256)), dtype=np.uint8)
            elif kind == 2 and pieces:
                src = pieces[int(rng.integers(0, len(pieces)))]
                seg = np.resize(src, m)
            else:
                seg = rng.integers(0, int(rng.choice([2, 4, 256])), m, dtype=np.uint8)
            x[o:o + m] = seg
            pieces.append(seg[:min(m, 5000)])
            o += m
        blocks.append(x)
    return n, blocks


def stride_block(d, n, seed, ahead=333, tail=b"", defect=None):
    """random bytes, then a d-periodic stretch over a random word of d bytes from `ahead` up to the end of the block (or up to
    `tail`); defect = k: one byte changed in the k-th period from the stretch's end (1: the last)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    m = n - ahead - len(tail)
    x[ahead:ahead + m] = np.resize(rng.integers(0, 256, d, dtype=np.uint8), m)
    if tail:
        x[n - len(tail):] = np.frombuffer(tail, dtype=np.uint8)
    if defect:
        at = ahead + m - defect * d + d // 2
        x[at] ^= 0x5A
    return x


def repeats_block(n, seed, L, d, start=None):
    """a d-byte word of random bytes repeated so that each residue class of the stretch holds L members at depth ~d: L + 1
    copies of the word (L members per residue class once the depth passes d) inside random bytes"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    o = int(rng.integers(0, n - (L + 1) * d)) if start is None else start
    x[o:o + (L + 1) * d] = np.resize(rng.integers(0, 256, d, dtype=np.uint8), (L + 1) * d)
    return x
