"""Pure Python + numpy model of the byte probe and of the rule that lets filter-auto find the byte predictor's lag and row stride
per segment (INTEGRATION.md 4b "Filter: auto with bytes"; csrc/byte_probe.hip, csrc/byte_rule.h), built from filter_grid_model and
byte_delta_model.

  A segment of L bytes x[i]; only its first P = L - L % 8 bytes are counted.  P < 1024: no byte candidate, both costs NO_COST.
    lag sums     A[l] = sum over i < P of m((x[i] - p) mod 256), l = 1 .. 16, p = x[i - l] where i mod 2048 >= l and 0 elsewhere,
                 m(d) = d below 128 and 255 - d otherwise.  Sixteen sums; the winner is the smallest, ties to the smallest l.
    stride sums  filter_grid_model's sample at element size 1: Wmax = min(65536, P // 2), 32 tiles of 256 targets,
                 S[W] = sum of bitlen(fold((x[i] - x[i - W]) mod 256)) for W = 17 .. Wmax: a row of 65537 words, 0xFFFFFFFF where
                 W is no candidate.  The winner is the smallest, ties to the smallest W; 0 without a candidate.
    planes       two rows of 256 counts: the histograms of byte_delta_model.byte_delta(x, lag, 0) and (x, lag, stride)
    costs        filter_auto_model.plane_cost of each row; NO_COST where there is no candidate
  The walk: fifteen candidates, filter_grid_model's thirteen in their order, then byte (lag, 0), then byte (lag, stride).  Among
  the first thirteen candidate i replaces the pick exactly when 33 * cost[i] < 32 * cost[pick]; a byte candidate replaces a pick
  of one plane (candidate 0 or byte (lag, 0)) under the same margin and a pick of more planes exactly when cost[i] < cost[pick]:
  the margin guards against the bias towards more planes, and a byte candidate has fewer (csrc/byte_rule.h).

A candidate here is filter_grid_model's (elem, delta, lag, fold, width); a byte candidate is (1, 1, lag, 0, stride)."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import byte_delta_model as BD
import container_model as M
import filter_auto_model as F
import filter_grid_model as Q
import filter_lag_model as FL

MIN_LEN, LAGS, RUN = 1024, BD.MAX_LAG, BD.RUN
S_MIN, S_MAX = 17, BD.MAX_STRIDE
SUM_ROW = S_MAX + 1
NO_SUM, NO_COST = Q.NO_SUM, Q.NO_COST
NCANDS = Q.NCANDS + 2
MAX_LEN = F.MAX_LEN
_FOLD_BITS8 = np.array([(((d << 1) ^ (0 - (d >> 7))) & 0xFF).bit_length() for d in range(256)], np.uint8)


def lag_clamp(word):
    return ((int(word) - 1) & 15) + 1


def stride_word(word):
    """a stride word as the plane probe uses it: outside 17 .. 65536 there is no candidate"""
    word = int(word) & 0xFFFFFFFF
    return word if S_MIN <= word <= S_MAX else 0


def lag_sums(seg):
    """the sixteen sums A[l] of one segment, as Python integers"""
    x = FL._counted(seg)
    i = np.arange(x.size)
    out = []
    for l in range(1, LAGS + 1):
        p = np.zeros_like(x)
        p[l:] = x[:x.size - l] if x.size > l else x[:0]
        p[i % RUN < l] = 0
        d = x - p
        out.append(int(np.where(d < 128, d, np.uint8(255) - d).sum(dtype=np.int64)))
    return out


def naive_lag_sums(seg):
    x = [int(v) for v in FL._counted(seg)]
    out = []
    for l in range(1, LAGS + 1):
        s = 0
        for i, v in enumerate(x):
            d = (v - (x[i - l] if i % RUN >= l else 0)) & 255
            s += d if d < 128 else 255 - d
        out.append(s)
    return out


def stride_sums(seg, chunk=1024):
    """uint32[65537]: S of one segment, by sliding windows over chunks of strides"""
    x = FL._counted(seg)
    row = np.full(SUM_ROW, NO_SUM, np.uint32)
    n = x.size
    if n < MIN_LEN:
        return row
    wm = Q.wmax(n)
    acc = np.zeros(wm + 1, np.int64)
    for b in Q.tile_starts(n):
        tgt = x[b:b + Q.TILE]
        for lo in range(S_MIN, wm + 1, chunk):
            hi = min(lo + chunk, wm + 1)                          # strides lo .. hi - 1
            h = x[b - (hi - 1):b + Q.TILE - lo]
            win = np.lib.stride_tricks.sliding_window_view(h, Q.TILE)[::-1]     # (reversed: row i is stride lo + i)
            acc[lo:hi] += _FOLD_BITS8[tgt[None, :] - win].sum(axis=1, dtype=np.int64)
    row[S_MIN:wm + 1] = acc[S_MIN:]
    return row


def naive_stride_sums(seg):
    x = [int(v) for v in FL._counted(seg)]
    row = [NO_SUM] * SUM_ROW
    if len(x) < MIN_LEN:
        return row
    starts = Q.tile_starts(len(x))
    for w in range(S_MIN, Q.wmax(len(x)) + 1):
        row[w] = sum(int(_FOLD_BITS8[(x[b + j] - x[b + j - w]) & 255]) for b in starts for j in range(Q.TILE))
    return row


def winners(Asums, S):
    """(lag, stride) from the sixteen lag sums and a stride row"""
    S = np.asarray(S, np.uint32)
    w = int(np.argmin(S))
    return int(np.argmin(np.asarray(Asums, np.uint64))) + 1, (w if S[w] != NO_SUM else 0)


def byte_planes(seg, words):
    """int64[2, 256]: the rows of one segment at the (lag, stride) words"""
    x = FL._counted(seg)
    rows = np.zeros((2, 256), np.int64)
    if x.size < MIN_LEN:
        return rows
    lag, stride = lag_clamp(words[0]), stride_word(words[1])
    rows[0] = np.bincount(BD.byte_delta(x, lag, 0), minlength=256)
    if stride:
        rows[1] = np.bincount(BD.byte_delta(x, lag, stride), minlength=256)
    return rows


def byte_costs(seg, rows, words):
    n = FL._counted(seg).size
    return [F.plane_cost(rows[0]) if n >= MIN_LEN else NO_COST, F.plane_cost(rows[1]) if n >= MIN_LEN and stride_word(words[1]) else NO_COST]


def probe(seg):
    """(lag sums, stride row, (lag, stride), rows, two costs) of one segment, what the two device probes give"""
    a, S = lag_sums(seg), stride_sums(seg)
    w = winners(a, S)
    rows = byte_planes(seg, w)
    return a, S, w, rows, byte_costs(seg, rows, w)


def cands(lags, widths, lag, stride):
    """the fifteen candidates as (elem, delta, lag, fold, width)"""
    return Q.cands(lags, widths) + [(1, 1, lag, 0, 0), (1, 1, lag, 0, stride)]


def pick(cost):
    p = Q.pick(cost[:Q.NCANDS])
    for i in range(Q.NCANDS, NCANDS):
        one_plane = p == 0 or p >= Q.NCANDS
        if (F.MARGIN_NUM * cost[i] < F.MARGIN_DEN * cost[p]) if one_plane else cost[i] < cost[p]:
            p = i
    return p


def rule(seg):
    """(pick, fifteen costs, lags, widths, (lag, stride)) of a segment"""
    _, c13, lags, widths = Q.rule(seg)
    _, _, w, _, b2 = probe(seg)
    c = list(c13) + b2
    return pick(c), c, lags, widths, w


def picked(seg):
    p, _, lags, widths, (lag, stride) = rule(seg)
    return cands(lags, widths, lag, stride)[p]


# ----------------------------------------------------------------------------------------------------------------------
# format version 16: version 14 whose frame word may also name the byte predictor.  A byte word is
# 1 | stride << 8 | (lag - 1) << 25 | 1 << 31: the low byte 1, stride 0 or 2 .. 65536, lag 1 .. 16, bits 29 and 30 zero.
# ----------------------------------------------------------------------------------------------------------------------
VERSION = 16
READS = frozenset(("sparse", "ans", "auto", "filter", "filter_lag", "filter_grid", "filter_byte"))      # a plan with the setting on
NO_FILTER = Q.NO_FILTER
WORD_TOP = Q.WORD_GRID


def is_byte(cand):
    return cand[0] == 1 and cand[1] == 1


def frame_word(cand):
    if is_byte(cand):
        return 1 | cand[4] << 8 | (cand[2] - 1) << 25 | WORD_TOP
    return Q.frame_word(cand)


def is_byte_word(word):
    return bool(word & WORD_TOP) and word & 0xFF == 1


def word_format(word):
    """the candidate whose filter a frame with this header word went through, or None where the word is not legal under version 16"""
    if not is_byte_word(word):
        return Q.word_format(word)
    stride = word >> 8 & 0x1FFFF
    if word >> 29 & 3 or not (stride == 0 or BD.MIN_STRIDE <= stride <= BD.MAX_STRIDE):
        return None
    return (1, 1, (word >> 25 & 15) + 1, 0, stride)


def filter_frame(a, cand):
    return BD.byte_delta(a, cand[2], cand[4]) if is_byte(cand) else Q.filter_frame(a, cand)


def unfilter_frame(a, cand):
    return BD.unbyte_delta(a, cand[2], cand[4]) if is_byte(cand) else Q.unfilter_frame(a, cand)


def picks_of(data, block_len, rows):
    a = M._u8(data).reshape(-1)
    return [picked(a[pos:pos + nb * bl][:MAX_LEN]) for pos, nb, bl in F.cut(a.size, block_len, rows)]


def last_filters(picks):
    """glcContainerLastFilters: a lag, grid or byte candidate counts among all frames only"""
    return FL.last_filters([c[:4] if not c[4] and not is_byte(c) else None for c in picks])


def last_lag_filters(picks):
    return FL.last_lag_filters([c[:4] for c in picks if not c[4] and not is_byte(c)])


def last_grid_filters(picks):
    return Q.last_grid_filters([c for c in picks if not is_byte(c)])


def last_byte_filters(picks):
    """glcContainerLastByteFilters: the frames that took byte (lag, 0), byte (lag, stride), and their sum"""
    n = [sum(1 for c in picks if is_byte(c) and not c[4]), sum(1 for c in picks if is_byte(c) and c[4])]
    return tuple(n) + (sum(n),)


def write(data, block_len, rows, picks=None, on=True):
    """The version-16 container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode,
    filter-auto, filter-lag, filter-grid and filter-byte on makes it; on = False: the setting off, filter_grid_model's version 14.
    `picks` (one candidate per frame) forces the filters instead of the rule."""
    a = M._u8(data).reshape(-1)
    if not on:
        return Q.write(a, block_len, rows, picks)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    frames = F.cut(a.size, block_len, rows)
    picks = picks_of(a, block_len, rows) if picks is None else [tuple(p) for p in picks]
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
    READS is a plan with the setting on (versions 1 to 5, 7, 8, 10, 13, 14 and 16); without "filter_byte" version 16 is a
    stream-header failure.  Every other version is filter_grid_model's reader's (byte_delta_model's with "byte"), which refuses a
    byte word as a frame-table failure."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        rest = frozenset(reads) - {"filter_byte"}
        if "byte" in rest:
            out = BD.read(buf, reads=rest)
            return (out, None) if with_filters else out
        return Q.read(buf, reads=rest, with_filters=with_filters)
    h = buf[:32]
    magic, _, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20 or flags or elem
            or "filter_byte" not in reads):
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
    are `words`: a byte frame is decoded from the run or the band of its own stride that holds the first byte
    (byte_delta_model.range_blocks), every other frame is filter_grid_model's"""
    nf = nblk = 0
    pos, end = 0, offset + count
    for (nb, bl), word in zip(frames, words):
        lo, hi = max(offset, pos), min(end, pos + nb * bl)
        if count and lo < hi:
            if is_byte_word(word):
                nf += 1
                nblk += len(BD.range_blocks(lo - pos, hi - pos, word >> 8 & 0x1FFFF, nb, bl))
            else:
                f, k = Q.range_stats([(nb, bl)], [word], lo - pos, hi - lo)
                nf += f
                nblk += k
        pos += nb * bl
    return nf, nblk


def refusal_cases(c16):
    """[(name, container, (what, frame, block), reads)] from the valid version-16 container c16: what the reader of a plan that
    speaks `reads` answers.  c16 needs a strided byte frame that is not the first, a byte frame in front of every grid and lag
    frame, a grid frame and a frame of two or more blocks."""
    lay = M.layout(c16)
    words = F.frame_words(c16)
    none = (M.STREAM_HEADER, -1, -1)
    fi = next(i for i, w in enumerate(words) if i and is_byte_word(w) and w >> 8 & 0x1FFFF)
    _, _, lag, _, stride = word_format(words[fi])
    gi = next(i for i, w in enumerate(words) if w & WORD_TOP and not is_byte_word(w))
    first = next(i for i, w in enumerate(words) if is_byte_word(w))
    word = lambda l=lag, s=stride, extra=0: 1 | s << 8 | (l - 1) << 25 | WORD_TOP | extra
    cases = [("version 16 with the delta flag in the stream header", M.with_header(c16, VERSION, 1, 0), none),
             ("version 16 with elem 1 in the stream header", M.with_header(c16, VERSION, 0, 1), none),
             ("version 16 with a byte word as the stream header's word 3", M.with_header(c16, VERSION, 0, 1 | stride << 8), none),
             ("version 16 with version 15's header words", M.with_header(c16, VERSION, BD.flags_of(lag, stride), BD.word3_of(stride)), none),
             ("version 17", M.with_header(c16, 17, 0, 0), none)]
    bad = [("bit 29", word(extra=1 << 29)), ("bit 30", word(extra=1 << 30)), ("stride 1", word(s=1)), ("stride 65537", word(s=65537)),
           ("stride 0x1FFFF", word(s=0x1FFFF)), ("the low byte 0", word() & ~1), ("the low byte 3", word() | 2), ("the low byte 0x81", word() | 0x80)]
    for name, w in bad:
        cases.append(("byte word: " + name, F.with_frame_word(c16, fi, w), (M.FRAME_TABLE, fi, -1)))
    cases.append(("byte word without bit 31", F.with_frame_word(c16, fi, word() & ~WORD_TOP), (M.FRAME_TABLE, fi, -1)))
    cases += [("grid word: bit %d" % b, F.with_frame_word(c16, gi, words[gi] | 1 << b), (M.FRAME_TABLE, gi, -1)) for b in range(25, 30)]
    other_lag = lag + 1 if lag < LAGS else lag - 1
    cases += [("byte word changed, table CRC not", F.with_frame_word(c16, fi, word(s=stride + 1), recrc=False), (M.FRAME_TABLE, fi, -1)),
              ("a legal but wrong stride: only crc_all sees it", F.with_frame_word(c16, fi, word(s=stride + 1)), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong lag: only crc_all sees it", F.with_frame_word(c16, fi, word(l=other_lag)), (M.DECODED_CRC, -1, -1)),
              ("stride 0 for a strided frame: only crc_all sees it", F.with_frame_word(c16, fi, word(s=0)), (M.DECODED_CRC, -1, -1))]
    cases = [c + (READS,) for c in cases]
    cases += [("a byte word under a version-14 header", M.with_header(c16, Q.VERSION, 0, 0), (M.FRAME_TABLE, first, -1), READS),
              ("a byte word under a version-13 header", M.with_header(c16, FL.VERSION, 0, 0), (M.FRAME_TABLE, first, -1), READS),
              ("a byte word under a version-10 header", M.with_header(c16, F.VERSION, 0, 0), (M.FRAME_TABLE, first, -1), READS)]
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    s, en, _ = fr["records"][1]
    flipped = bytearray(c16)
    flipped[(s + en) // 2] ^= 0x20
    cases += [("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1), READS),
              ("cut inside the last frame", c16[:lay["trailer"] - 8], (M.TRUNCATED, len(words) - 1, -1), READS)]
    cases += [("version 16 to a version-14 plan", c16, none, Q.READS), ("version 16 to a version-13 plan", c16, none, FL.READS),
              ("version 16 to a version-10 plan", c16, none, F.READS), ("version 16 to a byte-delta plan", c16, none, BD.READS),
              ("version 16 to a plan with no mode on", c16, none, frozenset())]
    return cases, lay
