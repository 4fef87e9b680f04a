"""numpy restatement of k_hd_table (csrc/hd_encode.hip): glcHdBuildTable formulated for one workgroup.

* the present symbols sorted stably by count (ties: lower symbol first) as a RANK computation;
* package-merge over 11 lists, each level a RANK MERGE: L0 = the leaves; Lk merges the leaves with the pairs (2j, 2j+1)
  of L(k-1); an item's position is its own index plus the items of the other list ahead of it -- packages lighter than a
  leaf, leaves no heavier than a package (a leaf goes before a package of equal weight, glcHdBuildTable's `<=`);
* code length of a leaf = its occurrences in the first 2m - 2 items of L10, found by pushing MULTIPLICITIES down the
  package references (not with per-item leaf vectors);
* canonical codes by (length, symbol); m = 1 gives length 1, code 0; no symbol gives all zeros.

Also the random histograms the table tests share, and the reference's 2048-entry decoder table built from lens / codes."""
import numpy as np

MAX_LEN = 11


def build_table(hist):
    """hist: 256 counts -> (lens u8[256], codes u16[256])"""
    h = np.asarray(hist, dtype=np.uint64)
    lens = np.zeros(256, dtype=np.uint8)
    codes = np.zeros(256, dtype=np.uint16)
    present = np.nonzero(h)[0]
    m = present.size
    if m == 0:
        return lens, codes
    hp = h[present]
    rank = (hp[None, :] < hp[:, None]).sum(1) + ((hp[None, :] == hp[:, None]) & (present[None, :] < present[:, None])).sum(1)
    leaf = np.empty(m, dtype=np.uint64)
    sym = np.empty(m, dtype=np.int64)
    leaf[rank] = hp
    sym[rank] = present
    if m == 1:
        lens[sym[0]] = 1
    else:
        w = leaf.copy()
        refs = [np.arange(m)]                       # item reference: leaf index i >= 0, package j as -(j + 1)
        for _ in range(1, MAX_LEN):
            npk = w.size // 2
            pk = w[0:2 * npk:2] + w[1:2 * npk:2]
            pos_leaf = np.arange(m) + np.searchsorted(pk, leaf, side="left")      # packages < leaf weight
            pos_pk = np.arange(npk) + np.searchsorted(leaf, pk, side="right")     # leaves <= package weight
            n = m + npk
            nw = np.empty(n, dtype=np.uint64)
            ref = np.empty(n, dtype=np.int64)
            nw[pos_leaf], ref[pos_leaf] = leaf, np.arange(m)
            nw[pos_pk], ref[pos_pk] = pk, -(np.arange(npk) + 1)
            w = nw
            refs.append(ref)
        mult = np.zeros(w.size, dtype=np.int64)
        mult[:min(2 * m - 2, w.size)] = 1
        length = np.zeros(m, dtype=np.int64)
        for k in range(MAX_LEN - 1, -1, -1):
            ref = refs[k]
            isleaf = ref >= 0
            length[ref[isleaf]] += mult[isleaf]     # a leaf occurs once per level
            if k:
                nxt = np.zeros(refs[k - 1].size, dtype=np.int64)
                j = -ref[~isleaf] - 1
                nxt[2 * j] = mult[~isleaf]
                nxt[2 * j + 1] = mult[~isleaf]
                mult = nxt
        lens[sym] = length
    cnt = np.bincount(lens[lens > 0], minlength=MAX_LEN + 1)       # cnt[0] = 0
    nxt, c = np.zeros(MAX_LEN + 1, dtype=np.int64), 0
    for b in range(1, MAX_LEN + 1):                 # deflate's next_code
        c = (c + int(cnt[b - 1])) << 1
        nxt[b] = c
    for s in range(256):
        if lens[s]:
            codes[s] = nxt[lens[s]]
            nxt[lens[s]] += 1
    return lens, codes


def decoder_table(lens, codes):
    """the reference's cuhd::CUHDCodetableItemSingle[2048] as 4096 bytes: {num_bits, symbol} per 11-bit prefix, {0, 0}
    where no codeword reaches"""
    t = np.zeros((2048, 2), dtype=np.uint8)
    for s in np.nonzero(lens)[0]:
        ln = int(lens[s])
        lo = int(codes[s]) << (MAX_LEN - ln)
        t[lo:lo + (1 << (MAX_LEN - ln))] = (ln, s)
    return t.reshape(-1)


def random_histograms(n=2000, seed=20261016):
    """seeded histograms: any number of symbols, few symbols, heavy ties, counts up to 2^40, exponential counts that hit
    the 11-bit limit"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        kind = i % 5
        m = int(rng.integers(2, 9)) if kind == 1 else int(rng.integers(1, 257))
        syms = rng.choice(256, m, replace=False)
        if kind == 0:
            c = rng.integers(1, 1 << 20, m)
        elif kind == 1:
            c = rng.integers(1, 1000, m)
        elif kind == 2:                             # heavy ties: a handful of distinct counts
            c = rng.choice(rng.integers(1, 50, int(rng.integers(1, 4))), m)
        elif kind == 3:
            c = rng.integers(1, 1 << 40, m, dtype=np.int64)
        else:
            c = np.floor(2.0 ** rng.uniform(0, 40, m)).astype(np.int64)
        h = np.zeros(256, dtype=np.uint64)
        h[syms] = np.asarray(c, dtype=np.uint64)
        out.append(h)
    return out


def fibonacci_hist(k=30):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    h = np.zeros(256, dtype=np.uint64)
    h[:k] = f
    return h
