"""Pure Python + numpy model of the grid probe and of the rule that lets filter-auto find the 2-D predictor's row width per segment
(INTEGRATION.md 4b "Filter: auto with grid"; csrc/grid_probe.hip, csrc/grid_rule.h), built from filter_lag_model, grid_model and
filter_auto_model.

  A segment of L bytes; only its first P = L - L % 8 bytes are counted.  x_e[i] are its N = P / e elements of e = 2, 4, 8 bytes.
  N < 1024: the element size has no grid candidate, its width is 0.  Else Wmax = min(65536, N // 2) and the sample is T = 32 tiles
  of B = 256 targets at b_t = Wmax + t (N - Wmax - 256) // 31.
    sums     S_e[W] = sum over t, j < 256 of bitlen(fold(x_e[b_t + j] - x_e[b_t + j - W] mod 2^(8 e))), W = 2 .. Wmax: a row of
             3 * 65537 words, S_e[W] at k * 65537 + W, 0xFFFFFFFF where W is no candidate
    winners  w_e = the W with the smallest S_e[W], ties to the smallest W; 0 without a candidate
    planes   the e byte planes of grid_model.grid_delta_shuffle(x, e, w_e, fold = 1), bands and run heads included: 14 rows of 256
             counts in filter_lag_model's layout, zero where w_e = 0
    costs    filter_auto_model.plane_cost summed per element size; NO_COST = 1 << 56 where w_e = 0
  The walk: thirteen candidates, filter_lag_model's ten in their order, then the grid filter at (2, w_2), (4, w_4), (8, w_8) with
  the fold; pick = 0 and candidate i replaces the pick exactly when 33 * cost[i] < 32 * cost[pick].

A candidate here is (elem, delta, lag, fold, width): width 0 for filter_lag_model's ten."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import filter_auto_model as F
import filter_lag_model as FL
import grid_model as G

ELEMS = M.ELEMS
MIN_ELEMS, TILES, TILE = 1024, 32, 256
W_MIN, W_MAX = G.MIN_WIDTH, G.MAX_WIDTH
SUM_ROW = W_MAX + 1
SUMS, ROWS = 3 * SUM_ROW, FL.ROWS
NO_SUM, NO_COST = 0xFFFFFFFF, 1 << 56
PLANE_ROW = FL.PLANE_ROW
NCANDS = FL.NCANDS + len(ELEMS)
MAX_LEN = F.MAX_LEN
_BITLEN16 = np.frexp(np.arange(65536, dtype=np.float64))[1].astype(np.uint8)


def wmax(n):
    return min(W_MAX, n // 2)


def tile_starts(n):
    w = wmax(n)
    return [w + t * (n - w - TILE) // (TILES - 1) for t in range(TILES)]


def width_word(word):
    """a width word as the plane probe uses it: outside 2 .. 65536 there is no candidate"""
    word = int(word) & 0xFFFFFFFF
    return word if W_MIN <= word <= W_MAX else 0


def _bitlen32(m):
    """the bit lengths of the uint32 values m, by 16-bit table"""
    hi = m >> np.uint32(16)
    return np.where(hi > 0, _BITLEN16[hi] + np.uint8(16), _BITLEN16[m & np.uint32(0xFFFF)])


def _pair_bits(d, elem):
    """bitlen(fold(d)) of the differences d modulo 2^(8 elem), as small unsigned integers.  With s the difference as a signed
    number the fold is 2 s or -2 s - 1, whose bit length is that of m = s ^ (s >> (8 elem - 1)) plus one, and 0 for s = 0."""
    if elem == 2:
        return _FOLD_BITS16[d]
    t = d.dtype.type
    m = d ^ (t(0) - (d >> t(8 * elem - 1)))
    if elem == 4:
        bl = _bitlen32(m)
    else:
        hi = (m >> t(32)).astype(np.uint32)
        bl = np.where(hi > 0, _bitlen32(hi) + np.uint8(32), _bitlen32(m.astype(np.uint32)))
    return bl + (d != 0)


_FOLD_BITS16 = _BITLEN16[((np.arange(65536) << 1) ^ (0 - (np.arange(65536) >> 15))) & 0xFFFF]


def elem_sums(x, elem, chunk=1024):
    """uint32[65537]: S_e of the counted bytes x, by sliding windows over chunks of widths, in the elements' own unsigned arithmetic"""
    row = np.full(SUM_ROW, NO_SUM, np.uint32)
    v = x.view("<u%d" % elem)
    n = v.size
    if n < MIN_ELEMS:
        return row
    wm = wmax(n)
    acc = np.zeros(wm + 1, np.int64)
    for b in tile_starts(n):
        tgt = v[b:b + TILE]
        for lo in range(W_MIN, wm + 1, chunk):
            hi = min(lo + chunk, wm + 1)                          # widths lo .. hi - 1
            h = v[b - (hi - 1):b + TILE - lo]                     # position p is element b - (hi - 1) + p
            win = np.lib.stride_tricks.sliding_window_view(h, TILE)[::-1]     # (reversed: row i is width lo + i)
            acc[lo:hi] += _pair_bits(tgt[None, :] - win, elem).sum(axis=1, dtype=np.int64)
    row[W_MIN:wm + 1] = acc[W_MIN:]
    return row


def naive_sums(seg, elem):
    """S_e by the definition, a double loop over widths and targets in Python integers: for small segments"""
    x = FL._counted(seg)
    v = [int(a) for a in x.view("<u%d" % elem)]
    n, mask = len(v), (1 << 8 * elem) - 1
    row = [NO_SUM] * SUM_ROW
    if n < MIN_ELEMS:
        return row
    starts = tile_starts(n)
    for w in range(W_MIN, wmax(n) + 1):
        s = 0
        for b in starts:
            for j in range(TILE):
                d = (v[b + j] - v[b + j - w]) & mask
                s += (((d << 1) ^ (0 - (d >> (8 * elem - 1)))) & mask).bit_length()
        row[w] = s
    return row


def sums(seg):
    """uint32[3 * 65537]: the sums row of one segment"""
    x = FL._counted(seg)
    return np.concatenate([elem_sums(x, e) for e in ELEMS])


def winners(S):
    """(w_2, w_4, w_8) from a sums row"""
    out = []
    for k in range(len(ELEMS)):
        row = np.asarray(S[k * SUM_ROW:(k + 1) * SUM_ROW], np.uint32)
        w = int(np.argmin(row))                                   # (the first of equal sums)
        out.append(w if row[w] != NO_SUM else 0)
    return tuple(out)


def grid_planes(seg, widths):
    """int64[14, 256]: the rows of one segment at the width words (w_2, w_4, w_8)"""
    x = FL._counted(seg)
    rows = np.zeros((ROWS, 256), np.int64)
    for e, w in zip(ELEMS, widths):
        w = width_word(w)
        if not w or not x.size:
            continue
        f = G.grid_delta_shuffle(x, e, w, 1).reshape(e, -1)
        for j in range(e):
            rows[PLANE_ROW[e] + j] = np.bincount(f[j], minlength=256)
    return rows


def grid_costs(rows, widths):
    """the three costs of a segment's 14 rows at the width words"""
    return [sum(F.plane_cost(h) for h in rows[PLANE_ROW[e]:PLANE_ROW[e] + e]) if width_word(w) else NO_COST for e, w in zip(ELEMS, widths)]


def probe(seg):
    """(sums row, winners, rows, three costs) of one segment, what the two device probes give"""
    S = sums(seg)
    w = winners(S)
    rows = grid_planes(seg, w)
    return S, w, rows, grid_costs(rows, w)


def cands(lags, widths):
    """the thirteen candidates as (elem, delta, lag, fold, width)"""
    return [c + (0,) for c in FL.cands(lags)] + [(e, 1, 1, 1, w) for e, w in zip(ELEMS, widths)]


def pick(cost):
    p = 0
    for i in range(1, NCANDS):
        if F.MARGIN_NUM * cost[i] < F.MARGIN_DEN * cost[p]:
            p = i
    return p


def rule(seg):
    """(pick, thirteen costs, lags, widths) of a segment"""
    _, lags, _, c3 = FL.probe(seg)
    _, widths, _, g3 = probe(seg)
    c = F.costs(F.probe(seg)) + c3 + g3
    return pick(c), c, lags, widths


def picked(seg):
    """(elem, delta, lag, fold, width) of the candidate the rule gives a segment"""
    p, _, lags, widths = rule(seg)
    return cands(lags, widths)[p]


# ----------------------------------------------------------------------------------------------------------------------
# format version 14: version 13 whose frame word may also name the 2-D predictor.  Bit 31 clear: filter_lag_model's word; bit 31
# set: elem | width << 8 | fold << 30 | 1 << 31 with elem 2, 4 or 8, width 2 .. 65536 and bits 25 .. 29 zero.
# ----------------------------------------------------------------------------------------------------------------------
VERSION = 14
READS = frozenset(("sparse", "ans", "auto", "filter", "filter_lag", "filter_grid"))      # what a plan with the setting on speaks
NO_FILTER = FL.NO_FILTER + (0,)
WORD_GRID, WORD_FOLD = 1 << 31, 1 << 30


def frame_word(cand):
    e, d, l, f, w = cand
    if w:
        return e | w << 8 | f << 30 | WORD_GRID
    return FL.frame_word((e, d, l, f))


def word_format(word):
    """the candidate (elem, delta, lag, fold, width) whose filter a frame with this header word went through, or None where the
    word is not legal under version 14"""
    if not word & WORD_GRID:
        c = FL.word_format(word)
        return None if c is None else c + (0,)
    e, w = word & 0xFF, word >> 8 & 0x1FFFF
    if word >> 25 & 31 or e not in ELEMS or not W_MIN <= w <= W_MAX:
        return None
    return (e, 1, 1, word >> 30 & 1, w)


def filter_frame(a, cand):
    if cand[4]:
        return G.grid_delta_shuffle(a, cand[0], cand[4], cand[3])
    return FL.filter_frame(a, cand[:4])


def unfilter_frame(a, cand):
    if cand[4]:
        return G.ungrid_delta_unshuffle(a, cand[0], cand[4], cand[3])
    return FL.unfilter_frame(a, cand[:4])


def picks_of(data, block_len, rows):
    """the candidate the rule picks for every frame"""
    a = M._u8(data).reshape(-1)
    return [picked(a[pos:pos + nb * bl][:MAX_LEN]) for pos, nb, bl in F.cut(a.size, block_len, rows)]


def last_filters(picks):
    """glcContainerLastFilters: a lag or grid candidate counts among all frames only"""
    return FL.last_filters([c[:4] if not c[4] else None for c in picks])


def last_lag_filters(picks):
    return FL.last_lag_filters([c[:4] for c in picks if not c[4]])


def last_grid_filters(picks):
    """glcContainerLastGridFilters: the frames that took the grid candidate of elem 2, 4 and 8, and their sum"""
    n = [sum(1 for c in picks if c[4] and c[0] == e) for e in ELEMS]
    return tuple(n) + (sum(n),)


def write(data, block_len, rows, picks=None):
    """The version-14 container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode,
    filter-auto, filter-lag and filter-grid on makes it.  `picks` (one candidate per frame) forces the filters instead of the rule."""
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    frames = F.cut(a.size, block_len, rows)
    picks = picks_of(a, block_len, rows) if picks is None else list(picks)
    assert len(picks) == len(frames) and all(word_format(frame_word(p)) == tuple(p) for p in picks)
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION, 0, block_len, 0) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    for (pos, nb, bl), p in zip(frames, picks):
        f = filter_frame(a[pos:pos + nb * bl], p)
        fr = bytearray(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, ["rule"] * nb))
        fr[12:16] = struct.pack("<I", frame_word(p))
        out.append(M.retable(bytes(fr), 0))                       # (table_crc covers the word)
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, reads=READS, with_filters=False):
    """decoded bytes of a container as the reader of a plan that speaks `reads` sees it, or ContainerError(what, frame, block).
    READS is a plan with the setting on (versions 1 to 5, 7, 8, 10, 13 and 14); without "filter_grid" version 14 is a
    stream-header failure.  Every other version is filter_lag_model's reader's (grid_model's with "grid"), which refuses a grid
    word as a frame-table failure."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        rest = frozenset(reads) - {"filter_grid"}
        if "grid" in rest:
            out = G.read(buf, reads=rest)
            return (out, None) if with_filters else out
        return FL.read(buf, reads=rest, with_filters=with_filters)
    h = buf[:32]
    magic, _, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20 or flags or elem
            or "filter_grid" not in reads):
        raise M.ContainerError(M.STREAM_HEADER)
    L = len(buf)
    pos, done, fi = 32, 0, 0
    out, filters = [], []
    while done < total:
        if pos + 32 + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        fmagic, nb, bl, word, P, _, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        cand = word_format(word)
        if (fmagic != M.MAGIC_FRAME or cand is None or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * M.raw_words(bl)):
            raise M.ContainerError(M.FRAME_TABLE, fi)
        fb = 32 + 4 * M.tables_layout(nb, bl)["words"] + 4 * M._pad2(P)
        if pos + fb + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        out.append(unfilter_frame(F._frame_blocks(buf, pos, nb, bl, P, fi), cand))      # (version 8's frame)
        filters.append(word)
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > L:
        raise M.ContainerError(M.TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != M.MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != L:
        raise M.ContainerError(M.STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:
        raise M.ContainerError(M.DECODED_CRC)
    return (data, filters) if with_filters else data


def grid_needed_blocks(elem, width, nb, bl, a, b):
    """sorted block indices of a grid frame that bytes [a, b) of it need: range_model's delta frame with the start rounded down to
    the band of this frame's width instead of the run"""
    if a == b:
        return []
    Fb = nb * bl
    q = Fb // elem
    i0, i1 = a // elem, min(q, -(-b // elem))
    ranges = []
    if i0 < i1:
        i0 = G.range_first(i0, width)
        ranges += [(j * q + i0, j * q + i1) for j in range(elem)]
    if b > q * elem:
        ranges.append((q * elem, Fb))
    out = set()
    for lo, hi in ranges:
        if lo < hi:
            out.update(range(lo // bl, (hi - 1) // bl + 1))
    return sorted(out)


def range_stats(frames, words, offset, count):
    """(frames overlapped, needed blocks summed) of a read of [offset, offset + count) over frames [(nb, bl)] whose header words
    are `words`: a grid frame rounds to its own band, every other frame is filter_lag_model's"""
    nf = nblk = 0
    pos, end = 0, offset + count
    for (nb, bl), word in zip(frames, words):
        lo, hi = max(offset, pos), min(end, pos + nb * bl)
        if count and lo < hi:
            if word & WORD_GRID:
                nf += 1
                nblk += len(grid_needed_blocks(word & 0xFF, word >> 8 & 0x1FFFF, nb, bl, lo - pos, hi - pos))
            else:
                f, k = FL.range_stats([(nb, bl)], [word], lo - pos, hi - lo)
                nf += f
                nblk += k
        pos += nb * bl
    return nf, nblk


def refusal_cases(c14):
    """[(name, container, (what, frame, block), reads)] from the valid version-14 container c14: what the reader of a plan that
    speaks `reads` answers.  c14 needs a grid frame that is not the first and a frame of two or more blocks."""
    lay = M.layout(c14)
    words = F.frame_words(c14)
    none = (M.STREAM_HEADER, -1, -1)
    fi = next(i for i, w in enumerate(words) if i and w & WORD_GRID)          # a grid frame behind the first
    e, _, _, fold, width = word_format(words[fi])
    cases = [("version 14 with the delta flag in the stream header", M.with_header(c14, VERSION, 1, 0), none),
             ("version 14 with elem 4 in the stream header", M.with_header(c14, VERSION, 0, 4), none),
             ("version 14 with a grid word as the stream header's word 3", M.with_header(c14, VERSION, 0, e | width << 8), none),
             ("version 15", M.with_header(c14, 15, 0, 0), none)]
    word = lambda el=e, w=width, f=fold, extra=0: el | w << 8 | f << 30 | WORD_GRID | extra
    bad = [("bit %d" % b, word(extra=1 << b)) for b in range(25, 30)]
    bad += [("elem %d" % el, word(el=el)) for el in (0, 1, 3, 5, 6, 7, 16, 0x82)]
    bad += [("width 0", word(w=0)), ("width 1", word(w=1)), ("width 65537", word(w=65537)), ("width 0x1FFFF", word(w=0x1FFFF))]
    for name, w in bad:
        cases.append(("grid word: " + name, F.with_frame_word(c14, fi, w), (M.FRAME_TABLE, fi, -1)))
    other = width + 1 if width < W_MAX else width - 1
    cases += [("grid word changed, table CRC not", F.with_frame_word(c14, fi, word(w=other), recrc=False), (M.FRAME_TABLE, fi, -1)),
              ("a legal but wrong width: only crc_all sees it", F.with_frame_word(c14, fi, word(w=other)), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong fold: only crc_all sees it", F.with_frame_word(c14, fi, word(f=fold ^ 1)), (M.DECODED_CRC, -1, -1))]
    first = next(i for i, w in enumerate(words) if w & WORD_GRID)
    cases = [c + (READS,) for c in cases]
    cases += [("a grid word under a version-13 header", M.with_header(c14, FL.VERSION, 0, 0), (M.FRAME_TABLE, first, -1), READS),
              ("a grid word under a version-10 header", M.with_header(c14, F.VERSION, 0, 0),
               (M.FRAME_TABLE, next(i for i, w in enumerate(words) if w >> 16 > 1), -1), READS)]      # (a lag word in front of it fails first)
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    s, en, _ = fr["records"][1]
    flipped = bytearray(c14)
    flipped[(s + en) // 2] ^= 0x20
    cases += [("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1), READS),
              ("cut inside the last frame", c14[:lay["trailer"] - 8], (M.TRUNCATED, len(words) - 1, -1), READS)]
    cases += [("version 14 to a version-13 plan", c14, none, FL.READS), ("version 14 to a version-12 plan", c14, none, G.READS),
              ("version 14 to a version-10 plan", c14, none, F.READS), ("version 14 to a plan with no mode on", c14, none, frozenset())]
    return cases, lay
