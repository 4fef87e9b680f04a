"""Pure Python + numpy model of the lag probe and of the rule that lets filter-auto pick the delta's lag per segment (INTEGRATION.md
4b "Filter: auto with lag"; csrc/lag_probe.hip, csrc/lag_rule.h), built from lag_model, filter_auto_model and auto_model.

  A segment of L bytes; only its first P = L - L % 8 bytes x[0 .. P) are counted.  x_e[i] are its elements of e = 2, 4, 8 bytes and
  f_{e,l}[i] the output element of lag_model._lag_delta(x, e, l, fold = 1): the lagged delta at lag l = 1 .. 16 with runs of 2048
  elements, the fold applied, run heads included.
    sums     S[e][l] = sum_i bitlen(f_{e,l}[i]), bitlen(0) = 0, bitlen(v) = floor(log2 v) + 1: 48 sums, row (log2 e - 1) * 16 + l - 1
    winners  win_e = the l with the smallest S[e][l], ties to the smallest l; P = 0 gives (1, 1, 1)
    planes   E_e[j][v] = elements whose f_{e,win_e}[i] has byte j equal to v: 14 rows of 256 counts, E_2 first
    costs    filter_auto_model.plane_cost summed over the planes of E_2, of E_4, of E_8
  The walk: ten candidates, the seven of filter_auto_model.CANDS in their order, then (2, win_2, fold), (4, win_4, fold) and
  (8, win_8, fold); pick = 0 and candidate i replaces the pick exactly when 33 * cost[i] < 32 * cost[pick]."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import filter_auto_model as F
import lag_model as G

ELEMS = M.ELEMS                                                   # (2, 4, 8)
MAX_LAG = G.MAX_LAG
SUMS, ROWS = 3 * MAX_LAG, 14
PLANE_ROW = {2: 0, 4: 2, 8: 6}
NCANDS = len(F.CANDS) + len(ELEMS)
MAX_LEN = F.MAX_LEN


def _counted(seg):
    x = np.ascontiguousarray(M._u8(seg).reshape(-1))
    return x[:x.size - x.size % 8]


def sum_row(elem, lag):
    return ELEMS.index(elem) * MAX_LAG + lag - 1


def clamp(word):
    """a lag word as the plane probe uses it"""
    return ((int(word) - 1) & 15) + 1


def folded(x, elem, lag):
    """f_{elem,lag} of the counted bytes x (a multiple of 8) as unsigned integers of elem bytes"""
    return G._lag_delta(x, elem, lag, 1).view("<u%d" % elem)


def bitlen_sum(f):
    """sum of the bit lengths of the unsigned integers f, exactly: the exponent frexp gives an integer below 2^53 is its bit length
    (0 for 0), so 64-bit values go as two halves"""
    bl = lambda v: np.frexp(v.astype(np.float64))[1].astype(np.int64)
    if f.dtype.itemsize < 8:
        return int(bl(f).sum())
    hi, lo = bl(f >> np.uint64(32)), bl(f & np.uint64(0xFFFFFFFF))
    return int(np.where(hi > 0, hi + 32, lo).sum())


def sums(seg):
    """the 48 sums of one segment, as Python integers"""
    x = _counted(seg)
    return [bitlen_sum(folded(x, e, l)) for e in ELEMS for l in range(1, MAX_LAG + 1)]


def winners(S):
    """(win_2, win_4, win_8) from the 48 sums"""
    out = []
    for k in range(len(ELEMS)):
        row = [int(v) for v in S[k * MAX_LAG:(k + 1) * MAX_LAG]]
        out.append(row.index(min(row)) + 1)
    return tuple(out)


def lag_planes(seg, lags):
    """int64[14, 256]: the rows E_2, E_4, E_8 of one segment at the lags (l_2, l_4, l_8)"""
    x = _counted(seg)
    rows = np.zeros((ROWS, 256), np.int64)
    for e, l in zip(ELEMS, lags):
        f = folded(x, e, clamp(l)).view(np.uint8).reshape(-1, e)
        for j in range(e):
            rows[PLANE_ROW[e] + j] = np.bincount(f[:, j], minlength=256)
    return rows


def lag_costs(rows):
    """the three costs of a segment's 14 rows"""
    return [sum(F.plane_cost(h) for h in rows[PLANE_ROW[e]:PLANE_ROW[e] + e]) for e in ELEMS]


def probe(seg):
    """(sums, winners, rows, three costs) of one segment, what the two device probes give"""
    S = sums(seg)
    w = winners(S)
    rows = lag_planes(seg, w)
    return S, w, rows, lag_costs(rows)


def cands(lags):
    """the ten candidates as (elem, delta, lag, fold)"""
    return [(e, d, 1, 0) for e, d in F.CANDS] + [(e, 1, l, 1) for e, l in zip(ELEMS, lags)]


def pick(cost):
    """the index of the candidate the rule picks from the ten costs"""
    p = 0
    for i in range(1, NCANDS):
        if F.MARGIN_NUM * cost[i] < F.MARGIN_DEN * cost[p]:
            p = i
    return p


def rule(seg):
    """(pick, ten costs, winners) of a segment"""
    _, w, _, c3 = probe(seg)
    c = F.costs(F.probe(seg)) + c3
    return pick(c), c, w


def picked(seg):
    """(elem, delta, lag, fold) of the candidate the rule gives a segment"""
    p, _, w = rule(seg)
    return cands(w)[p]


# ----------------------------------------------------------------------------------------------------------------------
# format version 13: version 10 whose frame word may also name the lagged, folded delta -- elem | flags << 16 with flags 0, 1 or
# version 11's 1 | fold << 1 | (lag - 1) << 8.  A candidate is (elem, delta, lag, fold); (1, 0, 1, 0) is no filter.
# ----------------------------------------------------------------------------------------------------------------------
VERSION = 13
READS = frozenset(("sparse", "ans", "auto", "filter", "filter_lag"))      # what a plan with the setting on speaks
NO_FILTER = (1, 0, 1, 0)


def frame_word(cand):
    e, d, l, f = cand
    if not d:
        return 0 if e == 1 else e
    return e | (M.FLAG_DELTA if (l, f) == (1, 0) else G.flags_of(l, f)) << 16


def word_format(word):
    """the candidate (elem, delta, lag, fold) whose filter a frame with this header word went through, or None where the word is
    not legal.  The whole family of version 11's flags is, (lag > 1, fold 0) included; the writer makes only fold = 1 lag words."""
    elem, flags = word & 0xFFFF, word >> 16
    if elem == 0:
        return NO_FILTER if flags == 0 else None
    if elem not in ELEMS:
        return None
    if flags in (0, M.FLAG_DELTA):
        return (elem, flags, 1, 0)
    if G.flags_legal(flags):
        return (elem, 1) + G.lag_fold_of(G.VERSION, flags)
    return None


def filter_frame(a, cand):
    e, d, l, f = cand
    if e == 1:
        return M._u8(a).reshape(-1)
    return G.lag_delta_shuffle(a, e, l, f) if d else M.shuffle(a, e)     # ((1, 0) is container_model.delta_shuffle)


def unfilter_frame(a, cand):
    e, d, l, f = cand
    if e == 1:
        return M._u8(a).reshape(-1)
    return G.unlag_delta_unshuffle(a, e, l, f) if d else M.unshuffle(a, e)


def picks_of(data, block_len, rows):
    """the candidate the rule picks for every frame"""
    a = M._u8(data).reshape(-1)
    return [picked(a[pos:pos + nb * bl][:MAX_LEN]) for pos, nb, bl in F.cut(a.size, block_len, rows)]


def last_filters(picks):
    """what glcContainerLastFilters reports of a compress with these picks: a lag candidate counts among all frames only"""
    seven = [(e, d, 1, 0) for e, d in F.CANDS]
    return tuple(picks.count(c) for c in seven) + (len(picks),)


def last_lag_filters(picks):
    """what glcContainerLastLagFilters reports: the frames that took the lag candidate of elem 2, 4 and 8, and their sum"""
    n = [sum(1 for c in picks if c[0] == e and c[3] == 1) for e in ELEMS]
    return tuple(n) + (sum(n),)


def write(data, block_len, rows, picks=None):
    """The version-13 container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode,
    filter-auto and filter-lag on makes it.  `picks` (one candidate per frame) forces the filters instead of the rule."""
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
    READS is a plan with the setting on (versions 1 to 5, 7, 8, 10 and 13); without "filter_lag" version 13 is a stream-header
    failure.  Every other version is filter_auto_model's reader (lag_model's with "lag"), which refuses a lag word under version 10
    as a frame-table failure."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        rest = frozenset(reads) - {"filter_lag"}
        out = G.read(buf, reads=rest) if "lag" in rest else F.read(buf, reads=rest) if "filter" in rest else U.read(buf, reads=rest)
        return (out, None) if with_filters else out
    h = buf[:32]
    magic, _, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20 or flags or elem
            or "filter_lag" not in reads):
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


def range_stats(frames, words, offset, count):
    """(frames overlapped, needed blocks summed) of a read of [offset, offset + count) over frames [(nb, bl)] whose header words
    are `words`: a lag frame needs what a delta frame needs (the rounding to 2048 elements), so range_model is asked with the
    delta flag alone"""
    return F.range_stats(frames, [(w & 0xFFFF) | (w >> 16 & M.FLAG_DELTA) << 16 for w in words], offset, count)


def refusal_cases(c13):
    """[(name, container, (what, frame, block), reads)] from the valid version-13 container c13: what the reader of a plan that
    speaks `reads` answers.  c13 needs a lag frame that is not the first and a frame of two or more blocks."""
    lay = M.layout(c13)
    words = F.frame_words(c13)
    none = (M.STREAM_HEADER, -1, -1)
    fi = next(i for i, w in enumerate(words) if i and w >> 16 > 1)            # a lag frame behind the first
    elem, flags = words[fi] & 0xFFFF, words[fi] >> 16
    lag, fold = G.lag_fold_of(G.VERSION, flags)
    cases = [("version 13 with the delta flag in the stream header", M.with_header(c13, VERSION, 1, 0), none),
             ("version 13 with elem 4 in the stream header", M.with_header(c13, VERSION, 0, 4), none),
             ("version 13 with a lag word's flags and elem in the stream header", M.with_header(c13, VERSION, flags, elem), none),
             ("version 14", M.with_header(c13, 14, 0, 0), none)]
    word = lambda fl, e=elem: e | fl << 16
    for name, w in (("a lag field with elem 0", word(flags, 0)), ("bit 2, the grid's flag", word(flags | 4)), ("bit 7", word(flags | 0x80)),
                    ("bit 12", word(flags | 0x1000)), ("bit 15", word(flags | 0x8000)), ("elem 3", word(flags, 3)), ("elem 16", word(flags, 16)),
                    ("elem 1", word(flags, 1)), ("flags 2 alone, without bit 0", word(2)), ("the lag field without bit 0", word(flags & ~1))):
        cases.append(("frame word: " + name, F.with_frame_word(c13, fi, w), (M.FRAME_TABLE, fi, -1)))
    other = lag + 1 if lag < MAX_LAG else lag - 1
    cases += [("frame word changed, table CRC not", F.with_frame_word(c13, fi, word(G.flags_of(other, fold)), recrc=False), (M.FRAME_TABLE, fi, -1)),
              ("a legal but wrong lag: only crc_all sees it", F.with_frame_word(c13, fi, word(G.flags_of(other, fold))), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong fold: only crc_all sees it", F.with_frame_word(c13, fi, word(G.flags_of(lag if lag > 1 else 2, fold ^ 1))), (M.DECODED_CRC, -1, -1))]
    first = next(i for i, w in enumerate(words) if w >> 16 > 1)
    cases.append(("a lag word under a version-10 header", M.with_header(c13, F.VERSION, 0, 0), (M.FRAME_TABLE, first, -1)))
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    T = M.tables_layout(fr["nb"], fr["blk_len"])

    def poke(kind, b):
        x = bytearray(c13)
        off = fr["tables"][0] + 4 * (T["kind"] + b)
        x[off:off + 4] = struct.pack("<I", kind)
        return M.retable(bytes(x), fr["start"])

    cases += [("kind 4 under version 13", poke(4, 1), (M.FRAME_TABLE, multi, 1)), ("kind 6 under version 13", poke(6, 0), (M.FRAME_TABLE, multi, 0))]
    s, e, _ = fr["records"][1]
    flipped = bytearray(c13)
    flipped[(s + e) // 2] ^= 0x20
    cases.append(("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1)))
    cases.append(("cut inside the last frame", c13[:lay["trailer"] - 8], (M.TRUNCATED, len(words) - 1, -1)))
    cases = [c + (READS,) for c in cases]
    cases += [("version 13 to a version-10 plan", c13, none, F.READS), ("version 13 to a version-11 plan", c13, none, G.READS),
              ("version 13 to the auto mode's plan", c13, none, U.READS_AUTO), ("version 13 to a plan with no mode on", c13, none, frozenset())]
    return cases, lay
