"""Pure Python + numpy model of the filter probe and of the rule that picks a frame's byte-plane filter from it (INTEGRATION.md 4b
"filter: auto"; csrc/filter_probe.hip, csrc/filter_rule.h), built from the parts of container_model and auto_model.

  A segment of L bytes; only its first P = L - L % 8 bytes x[0 .. P) are counted.  The probe is 22 histograms of 256 counts:
    rows 0..7    A_k[v]    = positions p < P with p % 8 == k and x[p] == v
    rows 8..9    D_2[j][v], rows 10..13 D_4[j][v], rows 14..21 D_8[j][v] = elements i < P / e whose delta d_e[i] has byte j equal to v,
                 d_e the delta of container_model.delta_shuffle: restarts every 2048 elements, counted from the segment's start
  The candidates (elem, delta), in the order the rule walks them: CANDS; (1, 0) is no filter.  Plane j of (e, 0) is the sum of
  the A_k with k = j modulo e, plane j of (e, 1) is D_e[j].  A plane's cost is sum_s H[s] * COST[q(s)] with
  q(s) = clamp(H[s] * 4096 // N, 1, 4096), N = sum H and COST the table of auto_model: the bits, in 1/256 bit, of the plane's
  bytes at their own frequencies rounded down to 12 bits.  A candidate's cost is the sum over its planes.
  The rule: pick = 0; candidate i replaces the pick exactly when 33 * cost[i] < 32 * cost[pick].  (The minimum alone would pick
  elem 8 on float32 and elem 4 on text: more planes never raise an empirical entropy.)"""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import sparse_model as S

CANDS = ((1, 0), (2, 0), (2, 1), (4, 0), (4, 1), (8, 0), (8, 1))
ROWS = 22
DELTA_ROW = {2: 8, 4: 10, 8: 14}
MARGIN_NUM, MARGIN_DEN = 33, 32
MAX_LEN = 1 << 31


def probe(seg):
    """int64[22, 256]: the rows of the probe of one segment"""
    x = np.ascontiguousarray(M._u8(seg).reshape(-1))
    x = x[:x.size - x.size % 8]
    rows = np.zeros((ROWS, 256), np.int64)
    for k in range(8):
        rows[k] = np.bincount(x[k::8], minlength=256)
    for e in M.ELEMS:
        d = M._delta(x, e).reshape(-1, e)
        for j in range(e):
            rows[DELTA_ROW[e] + j] = np.bincount(d[:, j], minlength=256)
    return rows


def planes(rows, cand):
    """the histograms of the planes of candidate `cand` (an index into CANDS): int64[elem, 256]"""
    e, delta = CANDS[cand]
    rows = np.asarray(rows, np.int64)
    if delta:
        return rows[DELTA_ROW[e]:DELTA_ROW[e] + e]
    return np.stack([rows[j:8:e].sum(axis=0) for j in range(e)])


def plane_cost(h):
    """the cost of one plane from its 256 counts, on Python integers"""
    h = [int(v) for v in h]
    n = sum(h)
    return sum(v * int(U.COST[min(max(v * 4096 // n, 1), 4096)]) for v in h if v)


def costs(rows):
    """the seven costs of a probed segment"""
    return [sum(plane_cost(h) for h in planes(rows, c)) for c in range(len(CANDS))]


def pick(cost):
    """the index of the candidate the rule picks from the seven costs"""
    p = 0
    for i in range(1, len(CANDS)):
        if MARGIN_NUM * cost[i] < MARGIN_DEN * cost[p]:
            p = i
    return p


def rule(seg):
    """(pick, costs) of a segment"""
    c = costs(probe(seg))
    return pick(c), c


def inputs(n, seed=1):
    """the twelve inputs of the "filter: when" table, n bytes each: name -> uint8 array"""
    import datagen
    import series_datagen
    import typed_datagen
    rng = np.random.default_rng(seed)
    out = {}
    for k in typed_datagen.KINDS:
        out[k] = np.frombuffer(typed_datagen.typed_bytes(k, n), np.uint8)
    for k in series_datagen.KINDS:
        out[k] = np.ascontiguousarray(series_datagen.series_bytes(k, n))
    out["noise"] = rng.integers(0, 256, n, dtype=np.uint8)
    out["zeros"] = np.zeros(n, np.uint8)
    out["scattered"] = ((rng.random(n) < 0.1) * rng.integers(1, 256, n)).astype(np.uint8)       # 90 % zeros
    out["text"] = np.ascontiguousarray(datagen.text_bytes_fast(n))
    return out


def fixed_sizes(data, block_len, rows):
    """the bytes of the version-8 container (the auto mode on) of `data` under each of the seven fixed filters"""
    return [len(U.write(data, block_len, rows, elem=e, delta=bool(d))) for e, d in CANDS]


# ----------------------------------------------------------------------------------------------------------------------
# format version 10: version 8's frames, each with its own filter named in word 3 of its header (byte 12): elem | flags << 16
# ----------------------------------------------------------------------------------------------------------------------
VERSION = 10
READS = frozenset(("sparse", "ans", "auto", "filter"))            # what a plan with the setting on speaks


def frame_word(cand):
    e, d = CANDS[cand]
    return (0 if e == 1 else e) | (d << 16)


def word_format(word):
    """the Format whose filter a frame with this header word went through, or None where the word is not legal"""
    elem, flags = word & 0xFFFF, word >> 16
    if (elem == 0 and flags == 0) or (elem in M.ELEMS and flags in (0, M.FLAG_DELTA)):
        return M.Format(VERSION, flags, elem, flags == M.FLAG_DELTA, A.ANS)
    return None


def cut(n, block_len, rows):
    """[(pos, nb, bl)]: the frames a writer of block_len and rows cuts n bytes into"""
    out, pos = [], 0
    while pos < n:
        left = n - pos
        nb, bl = (min(rows, left // block_len), block_len) if left >= block_len else (1, left)
        out.append((pos, nb, bl))
        pos += nb * bl
    return out


def picks_of(data, block_len, rows):
    """the candidate the rule picks for every frame"""
    a = M._u8(data).reshape(-1)
    return [rule(a[pos:pos + nb * bl][:MAX_LEN])[0] for pos, nb, bl in cut(a.size, block_len, rows)]


def last_filters(picks):
    """what glcContainerLastFilters reports of a compress with these picks"""
    return tuple(picks.count(c) for c in range(len(CANDS))) + (len(picks),)


def write(data, block_len, rows, picks=None):
    """The version-10 container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode and
    filter-auto on makes it.  `picks` (one candidate index per frame) forces the filters instead of the rule."""
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    frames = cut(a.size, block_len, rows)
    picks = picks_of(a, block_len, rows) if picks is None else list(picks)
    assert len(picks) == len(frames)
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION, 0, block_len, 0) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    for (pos, nb, bl), p in zip(frames, picks):
        f = M.filter_frame(a[pos:pos + nb * bl], word_format(frame_word(p)))
        fr = bytearray(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, ["rule"] * nb))
        fr[12:16] = struct.pack("<I", frame_word(p))
        out.append(M.retable(bytes(fr), 0))                       # (table_crc covers the word)
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def frame_words(buf):
    """the header word 3 of every frame of a valid container"""
    return [struct.unpack("<I", bytes(buf[f["start"] + 12:f["start"] + 16]))[0] for f in M.layout(buf)["frames"]]


def read(buf, reads=READS, with_filters=False):
    """decoded bytes of a container as the reader of a plan with the setting on sees it (versions 1 to 5, 7, 8 and 10), or
    ContainerError(what, frame, block).  `reads` without "filter" is any other plan: version 10 is a stream-header failure to it.
    Versions below 10 are auto_model's reader; it refuses a non-zero frame word as a frame-table failure as ever."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        return U.read(buf, reads=frozenset(reads) - {"filter"})
    h = buf[:32]
    magic, _, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20 or flags or elem
            or "filter" not in reads):
        raise M.ContainerError(M.STREAM_HEADER)
    L = len(buf)
    pos, done, fi = 32, 0, 0
    out, filters = [], []
    while done < total:
        if pos + 32 + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        fmagic, nb, bl, word, P, _, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        fmt = word_format(word)
        if (fmagic != M.MAGIC_FRAME or fmt is None or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * M.raw_words(bl)):
            raise M.ContainerError(M.FRAME_TABLE, fi)
        fb = 32 + 4 * M.tables_layout(nb, bl)["words"] + 4 * M._pad2(P)
        if pos + fb + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        blocks = _frame_blocks(buf, pos, nb, bl, P, fi)
        out.append(M.unfilter_frame(blocks, fmt))
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


def _frame_blocks(buf, pos, nb, bl, P, fi):
    """the filtered bytes of the frame at pos, whose header has passed its range checks: the table CRC, every block's field checks
    and record CRC (the lowest (what, block) of the frame is reported), then the blocks decoded and compared with crc_raw --
    version 8's frame, check for check (auto_model.read)"""
    T = M.tables_layout(nb, bl)
    tb = buf[pos + 32: pos + 32 + 4 * T["words"]]
    if zlib.crc32(buf[pos:pos + 24] + tb) != struct.unpack("<I", buf[pos + 24:pos + 28])[0]:
        raise M.ContainerError(M.FRAME_TABLE, fi)
    W = np.frombuffer(tb, dtype=np.uint32)
    po = W[T["pay_off"]:T["pay_off"] + 2 * (nb + 1)].view(np.uint64).astype(np.int64)
    pay = np.frombuffer(buf[pos + 32 + 4 * T["words"]: pos + 32 + 4 * T["words"] + 4 * P], dtype=np.uint32)
    nsub, mw = T["nsub"], S.mask_words(bl)
    field = lambda name, b, n=1: W[T[name] + n * b: T[name] + n * (b + 1)]
    bad = []
    for b in range(nb):
        kind, idx, lo, hi = int(W[T["kind"] + b]), int(W[T["bwt"] + b]), int(po[b]), int(po[b + 1])
        eo, hist = field("enc_off", b, nsub), field("hist", b, 256)
        wrong = kind not in U.AUTO_KINDS or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
        if not wrong and kind == M.RAW:
            wrong = hi - lo != M.raw_words(bl)
        elif not wrong and kind == S.SPARSE:
            wrong = S.check_sparse_fields(idx, eo, hist, pay, lo, hi, bl)
        elif not wrong and kind == A.ANS:
            wrong = A.check_ans_fields(idx, eo, hist, pay, lo, hi, bl)
        elif not wrong and kind == M.HUFF0:
            wrong = idx != 0 or int(hist.astype(np.uint64).sum()) != bl or bool(eo.any()) or hi - lo != M.h0_words(hist)
        elif not wrong:
            wrong = (idx >= bl or hi - lo > nsub * (M.MAX_WORDS + 1)
                     or any(int(eo[s]) >= hi - lo or (s and eo[s] <= eo[s - 1]) for s in range(nsub)))
        if wrong:
            bad.append((M.FRAME_TABLE, b))
        elif zlib.crc32(pay[lo:hi].tobytes()) != int(W[T["crc_rec"] + b]):
            bad.append((M.RECORD_CRC, b))
    if bad:
        what, b = min(bad)
        raise M.ContainerError(what, fi, b)
    blocks = []
    for b in range(nb):
        kind, idx, lo, hi = int(W[T["kind"] + b]), int(W[T["bwt"] + b]), int(po[b]), int(po[b + 1])
        hist = field("hist", b, 256)
        if kind == M.RAW:
            blk = pay[lo:hi].view(np.uint8)[:bl]
        elif kind == S.SPARSE:
            mask = pay[lo:lo + mw]
            klen = S.klen_of(mask, bl)
            blk = S.join(idx, mask, M.h0_decode(hist, pay[lo + mw:hi], klen)[0] if klen else np.zeros(0, np.uint8), bl)
        elif kind == A.ANS:
            blk = A.decode_record(hist, pay[lo:hi], bl)
        elif kind == M.HUFF0:
            blk = M.h0_decode(hist, pay[lo:hi], bl)[0]
        else:
            blk = M.O.decompress(idx, hist, field("enc_off", b, nsub), pay[lo:hi], bl)
        if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):
            raise M.ContainerError(M.DECODED_CRC, fi, b)
        blocks.append(blk)
    return np.concatenate(blocks)


# ----------------------------------------------------------------------------------------------------------------------
# range reads: range_model's needed blocks with every frame's own filter
# ----------------------------------------------------------------------------------------------------------------------
def range_stats(frames, words, offset, count):
    """(frames overlapped, needed blocks summed) of a read of [offset, offset + count) over frames [(nb, bl)] whose header words
    are `words` (version 5 takes every filter triple, so range_model's closed form is asked under it)"""
    import range_model
    nf = nblk = 0
    pos, end = 0, offset + count
    for (nb, bl), word in zip(frames, words):
        lo, hi = max(offset, pos), min(end, pos + nb * bl)
        if count and lo < hi:
            nf += 1
            nblk += len(range_model.needed_blocks(5, word >> 16, word & 0xFFFF, nb, bl, lo - pos, hi - pos))
        pos += nb * bl
    return nf, nblk


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 10, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def with_frame_word(c, fi, word, recrc=True):
    """c with header word 3 of frame fi replaced (and, by default, the frame's table CRC recomputed)"""
    start = M.layout(c)["frames"][fi]["start"]
    x = bytearray(c)
    x[start + 12:start + 16] = struct.pack("<I", word)
    return M.retable(bytes(x), start) if recrc else bytes(x)


def refusal_cases(c10):
    """[(name, container, (what, frame, block), reads)] from the valid version-10 container c10: what the reader of a plan that
    speaks `reads` answers -- READS, a plan with the setting on, for every case but the last two, which are c10 itself to a reader
    without the setting (the auto mode's reader, and a plan with no mode on).  c10 needs at least two frames, a delta frame that is not the first and whose neighbour has another filter, and
    a frame of two or more blocks."""
    lay = M.layout(c10)
    words = frame_words(c10)
    none = (M.STREAM_HEADER, -1, -1)
    fi = next(i for i, w in enumerate(words) if i and w >> 16)               # a delta frame behind the first
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    cases = [("version 10 with elem 4 in the stream header", M.with_header(c10, VERSION, 0, 4), none),
             ("version 10 with the delta flag in the stream header", M.with_header(c10, VERSION, 1, 0), none),
             ("version 10 with the delta flag and elem 8 in the stream header", M.with_header(c10, VERSION, 1, 8), none),
             ("version 10 with flags 2", M.with_header(c10, VERSION, 2, 0), none),
             ("version 11", M.with_header(c10, 11, 0, 0), none),
             ("version 9", M.with_header(c10, 9, 0, 0), none),
             ("version 6", M.with_header(c10, 6, 0, 0), none),
             ("version 0", M.with_header(c10, 0, 0, 0), none)]
    for name, word in (("elem 3", 3), ("flags 2", 4 | 2 << 16), ("flags 1 with elem 0", 1 << 16), ("elem 16", 16), ("elem 1", 1),
                       ("a high flag bit", 4 | 0x8001 << 16), ("elem 4 + 65536 * 0 + 256", 4 | 256)):
        cases.append(("frame word: " + name, with_frame_word(c10, fi, word), (M.FRAME_TABLE, fi, -1)))
    other = 2 if words[fi] & 0xFFFF != 2 else 4
    cases += [("frame word changed, table CRC not", with_frame_word(c10, fi, other, recrc=False), (M.FRAME_TABLE, fi, -1)),
              ("a legal but wrong frame word: only crc_all sees it", with_frame_word(c10, fi, other), (M.DECODED_CRC, -1, -1)),
              ("the delta dropped from a frame word", with_frame_word(c10, fi, words[fi] & 0xFFFF), (M.DECODED_CRC, -1, -1))]
    # under the header of an older version the first non-zero frame word is refused
    first = next(i for i, w in enumerate(words) if w)
    cases += [("a non-zero frame word under a version-8 header", M.with_header(c10, U.VERSION, 0, 0), (M.FRAME_TABLE, first, -1)),
              ("a non-zero frame word under a version-5 header", M.with_header(c10, 5, 0, 0), (M.FRAME_TABLE, first, -1))]
    fr = lay["frames"][multi]
    T = M.tables_layout(fr["nb"], fr["blk_len"])

    def poke(kind, b):
        x = bytearray(c10)
        off = fr["tables"][0] + 4 * (T["kind"] + b)
        x[off:off + 4] = struct.pack("<I", kind)
        return M.retable(bytes(x), fr["start"])

    cases += [("kind 4 under version 10", poke(4, 1), (M.FRAME_TABLE, multi, 1)), ("kind 6 under version 10", poke(6, 0), (M.FRAME_TABLE, multi, 0))]
    s, e, _ = fr["records"][1]
    flipped = bytearray(c10)
    flipped[(s + e) // 2] ^= 0x20
    cases.append(("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1)))
    cases.append(("cut inside the last frame", c10[:lay["trailer"] - 8], (M.TRUNCATED, len(words) - 1, -1)))
    bad_trailer = bytearray(c10)
    bad_trailer[lay["trailer"] + 4:lay["trailer"] + 8] = struct.pack("<I", len(words) + 1)
    t12 = bytes(bad_trailer[lay["trailer"]:lay["trailer"] + 12])
    bad_trailer[lay["trailer"] + 12:lay["trailer"] + 16] = struct.pack("<I", zlib.crc32(t12))
    cases.append(("the trailer counts another frame", bytes(bad_trailer), (M.STREAM_HEADER, len(words), -1)))
    cases = [c + (READS,) for c in cases]
    cases += [("version 10 to a reader without the setting: the auto mode's", c10, none, U.READS_AUTO),
              ("version 10 to a reader without the setting: no mode on", c10, none, frozenset())]
    return cases, lay
