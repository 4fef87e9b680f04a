"""Pure Python + numpy model of the BWT container, every format version: the second, independent
implementation of the format.  BWT records come from the oracle (oracle_lib.compress / decompress), order-0 records from numpy
and hd_table_model, CRCs from zlib.crc32.  Also the CRC algebra the device kernel uses (raw CRCs, shifts by x^(8n) mod P, granule
rows), written out so that it can be checked against zlib.

A stream is a header, frames and a trailer; a frame is a 32-byte header, tables and a payload.  The stream header's triple
(version, flags, elem) sets the only two things that vary between versions (FORMATS below):
  * the filter every frame's nb * blk_len bytes go through, as ONE segment, before the frame's blocks are cut from them: none,
    the byte-plane shuffle, or delta + shuffle, over elements of `elem` bytes.  crc_raw[b] is the CRC of block b of the filtered
    frame; the trailer's crc_all is the CRC of the original input, which only the unfiltered output can be compared with;
  * the highest legal record kind: 1 (BWT + Huffman, raw), or 2 (also the order-0 Huffman record).
A kind-2 block stores hist[256] = its byte counts in the frame tables (bwt_index 0, enc_off zeros); the table is not stored, it is
hd_table_model.build_table(hist) (package-merge, <= 11 bits, canonical by (length, symbol)); the record is the codes of the
block's bytes packed MSB-first into 32-bit units, zero bits after the last code, one zero pad unit -- exactly
ceil(sum hist * lens / 32) + 1 words, which the reader checks before it decodes anything.  The delta: with x[i] element i of a
frame as a little-endian unsigned integer, d[i] = x[i] where i % RUN == 0, else x[i] - x[i - 1] modulo 2^(8 elem)."""
import struct
import zlib
from collections import namedtuple

import numpy as np

import hd_table_model as H
import oracle_lib as O

MAGIC_STREAM, MAGIC_FRAME, MAGIC_END = b"GLCB", b"GLCF", b"GLCE"
HUFF, RAW, HUFF0 = 0, 1, 2
CODEC_BWT, CODEC_HUFF0 = 0, 1
ELEMS = (2, 4, 8)
FLAG_DELTA = 1
RUN = 2048
HUFF_BLOCK, MAX_WORDS = 4096, 1536
STREAM_HEADER, FRAME_TABLE, RECORD_CRC, DECODED_CRC, TRUNCATED, CAPACITY = 1, 2, 3, 4, 5, 6

# ----------------------------------------------------------------------------------------------------------------------
# CRC algebra (reflected CRC-32/IEEE; bit 31 of a register is x^0)
# ----------------------------------------------------------------------------------------------------------------------
POLY = 0xEDB88320


def multmodp(a, b):
    p = 0
    for i in range(32):
        if (a >> (31 - i)) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


X2N = []
_p = 1 << 30
for _k in range(32):
    X2N.append(_p)
    _p = multmodp(_p, _p)


def x8n(n):
    """x^(8 n) mod P"""
    p, k = 1 << 31, 3
    while n:
        if n & 1:
            p = multmodp(X2N[k & 31], p)
        n >>= 1
        k += 1
    return p


def shift(r, nbytes):
    """what feeding nbytes zero bytes does to a raw register"""
    return multmodp(x8n(nbytes), r)


def combine(crc1, crc2, len2):
    """zlib.crc32(A + B) from crc32(A), crc32(B) and len(B)"""
    return shift(crc1, len2) ^ crc2


_T0 = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (POLY if _c & 1 else 0)
    _T0.append(_c)


def raw_crc(data, r=0):
    """the register after feeding data, from r, without the complements"""
    for b in bytes(data):
        r = _T0[(r ^ b) & 255] ^ (r >> 8)
    return r


def crc_from_raw(raw, n):
    return raw ^ shift(0xFFFFFFFF, n) ^ 0xFFFFFFFF


def crc_chunked(buf, off, length, chunk):
    """The kernel's decomposition: address-aligned granules of 16 bytes up to E16 = (p + L) & ~15, laid out as rows of
    `chunk` // 16 columns from a virtual start before p (bytes before p are zeros); column accumulators
    acc = shift(acc, row) ^ crc0(granule), a tree over the columns, the tail bytes serially, then the complements.
    `buf` is a bytes-like object; `off` plays the role of the address (its value mod 16 is the alignment)."""
    mv = memoryview(bytes(buf))
    p, end = off, off + length
    e16 = end & ~15
    cols = chunk // 16
    r = 0
    if e16 > p:
        g0 = p & ~15
        nrows = ((e16 - g0) // 16 + cols - 1) // cols
        a0 = e16 - nrows * chunk
        accs = [0] * cols
        for row in range(nrows):
            for c in range(cols):
                a = a0 + row * chunk + 16 * c
                g = bytearray(16)
                for k in range(16):
                    if a + k >= p:
                        g[k] = mv[a + k]
                accs[c] = shift(accs[c], chunk) ^ raw_crc(g)
        # tree over the columns: column c is followed by 16 (cols - 1 - c) bytes of its row
        for c in range(cols):
            r ^= shift(accs[c], 16 * (cols - 1 - c))
    tail0 = e16 if e16 > p else p
    r = raw_crc(mv[tail0:end], r)
    return crc_from_raw(r, length)


def fold_block_crcs(crcs, blk_len):
    c = 0
    for v in crcs:
        c = combine(c, v, blk_len)
    return c


# ----------------------------------------------------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------------------------------------------------
def _pad2(n):
    return n + (n & 1)


def tables_layout(nb, blk_len):
    """word offsets of the sections of a frame's tables and their total"""
    nsub = (blk_len + HUFF_BLOCK - 1) // HUFF_BLOCK
    a, e = _pad2(nb), _pad2(nb * nsub)
    t = dict(nsub=nsub, kind=0, bwt=a, crc_raw=2 * a, crc_rec=3 * a, hist=4 * a)
    t["enc_off"] = t["hist"] + 256 * nb
    t["pay_off"] = t["enc_off"] + e
    t["words"] = t["pay_off"] + 2 * (nb + 1)
    return t


def raw_words(blk_len):
    return (blk_len + 3) // 4


def bound(length, block_len):
    """glcContainerBound"""
    frames = (length + block_len - 1) // block_len
    return 32 + 16 + length + frames * (32 + 4 * tables_layout(1, block_len)["words"] + 7)


class ContainerError(ValueError):
    def __init__(self, what, frame=-1, block=-1):
        super().__init__("container refused: what=%d frame=%d block=%d" % (what, frame, block))
        self.what, self.frame, self.block = what, frame, block


# ----------------------------------------------------------------------------------------------------------------------
# the format rule: which stream headers are legal, and what each one means
# ----------------------------------------------------------------------------------------------------------------------
Format = namedtuple("Format", "version flags elem delta max_kind")       # elem 0: no filter; delta: delta + shuffle, else shuffle
FORMATS = {(1, 0): ((0,), RAW), (2, 0): (ELEMS, RAW), (3, 0): ((0,) + ELEMS, HUFF0), (4, FLAG_DELTA): (ELEMS, HUFF0)}


def stream_format(version, flags, elem):
    """the Format of a header triple, or None where the triple is not legal"""
    elems, max_kind = FORMATS.get((version, flags), ((), RAW))
    return Format(version, flags, elem, flags == FLAG_DELTA, max_kind) if elem in elems else None


def writer_format(elem=0, codec=0, delta=False, kinds=None):
    """the header a writer plan of these settings makes: the lowest version that can say them (elem 1 is no filter)"""
    elem = 0 if elem == 1 else elem
    version = 4 if delta else 3 if codec == CODEC_HUFF0 or kinds is not None else 2 if elem else 1
    fmt = stream_format(version, FLAG_DELTA if delta else 0, elem)
    assert fmt is not None and codec in (CODEC_BWT, CODEC_HUFF0)
    return fmt


# ----------------------------------------------------------------------------------------------------------------------
# the filters
# ----------------------------------------------------------------------------------------------------------------------
def _u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8)


def shuffle(data, elem):
    """out[j * q + i] = in[i * elem + j] over the q = len // elem whole elements; the last len % elem bytes stay in place"""
    a = _u8(data).reshape(-1)
    assert elem in ELEMS
    m = a.size - a.size % elem
    return np.concatenate([a[:m].reshape(-1, elem).T.reshape(-1), a[m:]])


def unshuffle(data, elem):
    a = _u8(data).reshape(-1)
    assert elem in ELEMS
    m = a.size - a.size % elem
    return np.concatenate([a[:m].reshape(elem, -1).T.reshape(-1), a[m:]])


def _delta(a, elem):
    """the whole elements of `a` replaced by their differences within runs of RUN elements; the last len % elem bytes as they are"""
    m = a.size - a.size % elem
    x = a[:m].view("<u%d" % elem)
    d = x.copy()
    d[1:] -= x[:-1]                                            # (unsigned: wraps modulo 2^(8 elem))
    d[::RUN] = x[::RUN]
    return np.concatenate([d.view(np.uint8), a[m:]])


def _undelta(a, elem):
    m = a.size - a.size % elem
    d = a[:m].view("<u%d" % elem)
    x = np.empty_like(d)
    for r in range(0, d.size, RUN):
        x[r:r + RUN] = np.cumsum(d[r:r + RUN], dtype=d.dtype)
    return np.concatenate([x.view(np.uint8), a[m:]])


def delta_shuffle(data, elem):
    """out[j * q + i] = byte j of d[i] over the q = len // elem whole elements; the last len % elem bytes stay in place"""
    assert elem in ELEMS
    return shuffle(_delta(np.ascontiguousarray(_u8(data).reshape(-1)), elem), elem)


def undelta_unshuffle(data, elem):
    assert elem in ELEMS
    return _undelta(np.ascontiguousarray(unshuffle(data, elem)), elem)


def filter_frame(frame, fmt):
    """a frame's bytes as its blocks are cut from them (element numbering restarts with the frame)"""
    return frame if not fmt.elem else (delta_shuffle if fmt.delta else shuffle)(frame, fmt.elem)


def unfilter_frame(frame, fmt):
    return frame if not fmt.elem else (undelta_unshuffle if fmt.delta else unshuffle)(frame, fmt.elem)


# ----------------------------------------------------------------------------------------------------------------------
# the order-0 record, written and read in numpy alone (a bit scatter and a table walk), independent of the library's host encoder
# ----------------------------------------------------------------------------------------------------------------------
def h0_words(hist, lens=None):
    """words of the record of a block with these byte counts: ceil(bits / 32) + 1 (the pad unit)"""
    if lens is None:
        lens, _ = H.build_table(hist)
    bits = int((np.asarray(hist, np.uint64) * lens.astype(np.uint64)).sum())
    return (bits + 31) // 32 + 1


def h0_encode(blk):
    """(hist u32[256], record words u32) of one block"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    hist = np.bincount(blk, minlength=256).astype(np.uint32)
    lens, codes = H.build_table(hist)
    ln = lens[blk].astype(np.int64)
    cd = codes[blk].astype(np.int64)
    nwords = h0_words(hist, lens)
    end = np.cumsum(ln)
    start = end - ln
    bits = np.zeros(32 * nwords, dtype=np.uint8)
    for j in range(H.MAX_LEN):                                  # bit j of a code (MSB first) goes to position start + j
        m = ln > j
        bits[start[m] + j] = (cd[m] >> (ln[m] - 1 - j)) & 1
    return hist, np.packbits(bits).view(">u4").astype(np.uint32)


def h0_decode(hist, words, n):
    """n symbols of a record by walking the 2048-entry decoder table; returns (bytes, bits consumed)"""
    lens, codes = H.build_table(hist)
    t = H.decoder_table(lens, codes).reshape(2048, 2)
    tl, ts = t[:, 0].astype(np.int64), t[:, 1]
    tl[tl == 0] = 1                                             # prefixes no codeword reaches: never met in a valid record
    bits = np.unpackbits(np.asarray(words, np.uint32).astype(">u4").view(np.uint8)).astype(np.int64)
    nb = bits.size
    bits = np.concatenate([bits, np.zeros(H.MAX_LEN, np.int64)])
    win = np.zeros(nb, dtype=np.int64)                          # the next 11 bits at every bit position
    for j in range(H.MAX_LEN):
        win = (win << 1) | bits[j:j + nb]
    step = (np.arange(nb) + tl[win]).tolist()
    pos, p = [], 0
    for _ in range(n):
        if p >= nb:
            raise ContainerError(DECODED_CRC)                   # (cannot happen behind the reader's field checks)
        pos.append(p)
        p = step[p]
    return ts[win[np.asarray(pos, dtype=np.int64)]].astype(np.uint8) if n else np.zeros(0, np.uint8), p


# ----------------------------------------------------------------------------------------------------------------------
# writer
# ----------------------------------------------------------------------------------------------------------------------
def encode_block(blk, codec=HUFF):
    """(kind, bwt_index, hist, enc_off, record words) of one block by the codec named as a kind: 0 = the BWT codec, raw when it
    fails or 4 * words >= blk_len; 1 = raw; 2 = order-0 Huffman, raw when 4 * words >= blk_len"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    nsub = (blk.size + HUFF_BLOCK - 1) // HUFF_BLOCK
    if codec == HUFF:
        r = O.compress(blk)
        if r["rc"] == 0 and 4 * r["size"] < blk.size:
            return HUFF, r["bwt_index"], r["hist"], np.asarray(r["offsets"], np.uint32), np.asarray(r["words"], np.uint32)
    elif codec == HUFF0:
        hist, words = h0_encode(blk)
        if 4 * words.size < blk.size:
            return HUFF0, 0, hist, np.zeros(nsub, np.uint32), words
    else:
        assert codec == RAW
    padded = np.zeros(4 * raw_words(blk.size), dtype=np.uint8)
    padded[:blk.size] = blk
    return RAW, 0, np.zeros(256, np.uint32), np.zeros(nsub, np.uint32), padded.view(np.uint32)


def _frame(blocks, blk_len, kinds):
    nb = len(blocks)
    T = tables_layout(nb, blk_len)
    W = np.zeros(T["words"], dtype=np.uint32)
    recs, pay_off = [], [0]
    for b, blk in enumerate(blocks):
        kind, idx, hist, eo, words = encode_block(blk, kinds[b])
        W[T["kind"] + b] = kind
        W[T["bwt"] + b] = idx
        W[T["crc_raw"] + b] = zlib.crc32(blk.tobytes())
        W[T["crc_rec"] + b] = zlib.crc32(words.tobytes())
        W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)] = hist
        W[T["enc_off"] + T["nsub"] * b: T["enc_off"] + T["nsub"] * (b + 1)] = eo
        recs.append(words)
        pay_off.append(pay_off[-1] + words.size)
    W[T["pay_off"]: T["pay_off"] + 2 * (nb + 1)] = np.asarray(pay_off, dtype=np.uint64).view(np.uint32)
    P = pay_off[-1]
    hdr24 = MAGIC_FRAME + struct.pack("<III", nb, blk_len, 0) + struct.pack("<Q", P)
    tables = W.tobytes()
    table_crc = zlib.crc32(hdr24 + tables)
    payload = b"".join(w.tobytes() for w in recs) + (b"\0\0\0\0" if P & 1 else b"")
    return hdr24 + struct.pack("<II", table_crc, 0) + tables + payload


def write(data, block_len, rows, elem=0, codec=0, delta=False, kinds=None):
    """The container of `data` (bytes / uint8 array) as a writer plan of n = block_len, `rows` rows, filter element size `elem`
    (0 or 1: none), container codec `codec` and delta mode `delta` (elem 2, 4 or 8) makes it: every block coded by the plan's
    codec.  `kinds` (a sequence over the stream's blocks, cycled; each 0, 1 or 2) forces the codec of each block instead -- 0 the
    BWT codec, 1 raw, 2 order-0, every one still under its raw rule -- and so builds the mixed containers no GPU writer makes
    but every reader of version 3 or later accepts."""
    fmt = writer_format(elem, codec, delta, kinds)
    a = _u8(data).reshape(-1)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    n = a.size
    hdr24 = MAGIC_STREAM + struct.pack("<HHII", fmt.version, fmt.flags, block_len, fmt.elem) + struct.pack("<Q", n)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    pos, frames, nblk = 0, 0, 0
    while pos < n:
        left = n - pos
        if left >= block_len:
            nb, bl = min(rows, left // block_len), block_len
        else:
            nb, bl = 1, left
        f = filter_frame(a[pos:pos + nb * bl], fmt)
        per = [HUFF0 if codec == CODEC_HUFF0 else HUFF] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(_frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        pos += nb * bl
        nblk += nb
        frames += 1
    t12 = MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


# ----------------------------------------------------------------------------------------------------------------------
# reader: the checks in the order the device path makes them
# ----------------------------------------------------------------------------------------------------------------------
def read(buf, with_kinds=False, max_version=4):
    """decoded bytes of a container, or ContainerError(what, frame, block).  max_version = k is the reader of format version k:
    a later version is a stream-header failure to it."""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise ContainerError(TRUNCATED)
    h = buf[:32]
    magic, ver, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    fmt = stream_format(ver, flags, elem)
    if (magic != MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or fmt is None or ver > max_version):
        raise ContainerError(STREAM_HEADER)
    pos, done, fi = 32, 0, 0
    out, kinds = [], []
    while done < total:
        if pos + 32 + 16 > L:
            raise ContainerError(TRUNCATED, fi)
        fmagic, nb, bl, fz, P, tcrc, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        if (fmagic != MAGIC_FRAME or fz or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * raw_words(bl)):
            raise ContainerError(FRAME_TABLE, fi)
        T = tables_layout(nb, bl)
        fb = 32 + 4 * T["words"] + 4 * _pad2(P)
        if pos + fb + 16 > L:
            raise ContainerError(TRUNCATED, fi)
        tb = buf[pos + 32: pos + 32 + 4 * T["words"]]
        if zlib.crc32(buf[pos:pos + 24] + tb) != tcrc:
            raise ContainerError(FRAME_TABLE, fi)
        W = np.frombuffer(tb, dtype=np.uint32)
        po = W[T["pay_off"]:T["pay_off"] + 2 * (nb + 1)].view(np.uint64).astype(np.int64)
        pay = np.frombuffer(buf[pos + 32 + 4 * T["words"]: pos + 32 + 4 * T["words"] + 4 * P], dtype=np.uint32)
        nsub = T["nsub"]
        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            wrong = kind > fmt.max_kind or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
            if not wrong and kind == RAW:
                wrong = hi - lo != raw_words(bl)
            elif not wrong and kind == HUFF0:                  # the counts are the block's, nothing else is set, and the
                wrong = (int(W[T["bwt"] + b]) != 0 or int(hist.astype(np.uint64).sum()) != bl or bool(eo.any())   # record has
                         or hi - lo != h0_words(hist))         # exactly the words the table of those counts asks for
            elif not wrong:
                wrong = (int(W[T["bwt"] + b]) >= bl or hi - lo > nsub * (MAX_WORDS + 1)
                         or any(int(eo[s]) >= hi - lo or (s and eo[s] <= eo[s - 1]) for s in range(nsub)))
            if wrong:
                bad.append((FRAME_TABLE, b))
            elif zlib.crc32(pay[lo:hi].tobytes()) != int(W[T["crc_rec"] + b]):
                bad.append((RECORD_CRC, b))
        if bad:
            what, b = min(bad)
            raise ContainerError(what, fi, b)
        blocks = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            if kind == RAW:
                blk = pay[lo:hi].view(np.uint8)[:bl]
            elif kind == HUFF0:
                blk, used = h0_decode(hist, pay[lo:hi], bl)
                assert (used + 31) // 32 + 1 == hi - lo        # decoding blk_len symbols consumes the record exactly
            else:
                blk = O.decompress(int(W[T["bwt"] + b]), hist, W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):      # (of the FILTERED frame's block)
                raise ContainerError(DECODED_CRC, fi, b)
            blocks.append(blk)
            kinds.append(kind)
        out.append(unfilter_frame(np.concatenate(blocks), fmt))           # the frame is one segment
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > L:
        raise ContainerError(TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != L:
        raise ContainerError(STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:                  # only this sees a legal but wrong elem or flag: the ORIGINAL bytes
        raise ContainerError(DECODED_CRC)
    return (data, kinds) if with_kinds else data


# ----------------------------------------------------------------------------------------------------------------------
# for tests that corrupt a valid container: where its parts are, and the refusal cases of the formats
# ----------------------------------------------------------------------------------------------------------------------
def layout(buf):
    """byte ranges of a valid container's parts: a list of frames, each a dict with 'start', 'tables' (start, end), 'payload'
    start, 'records' [(start, end, kind)] in bytes, and the trailer's start"""
    buf = bytes(buf)
    pos, frames = 32, []
    total = struct.unpack("<Q", buf[16:24])[0]
    done = 0
    while done < total:
        nb, bl, P = _frame_shape(buf, pos)
        T = tables_layout(nb, bl)
        W = np.frombuffer(buf[pos + 32: pos + 32 + 4 * T["words"]], dtype=np.uint32)
        po = W[T["pay_off"]:T["pay_off"] + 2 * (nb + 1)].view(np.uint64)
        ps = pos + 32 + 4 * T["words"]
        frames.append(dict(start=pos, nb=nb, blk_len=bl, tables=(pos + 32, ps), payload=ps,
                           records=[(ps + 4 * int(po[b]), ps + 4 * int(po[b + 1]), int(W[T["kind"] + b])) for b in range(nb)]))
        pos = ps + 4 * _pad2(P)
        done += nb * bl
    return dict(frames=frames, trailer=pos)


def _frame_shape(buf, frame_start):
    """(nb, blk_len, payload words) a frame header names"""
    nb, bl, _, P = struct.unpack("<IIIQ", bytes(buf[frame_start + 4:frame_start + 24]))
    return nb, bl, P


def retable(buf, frame_start):
    """`buf` with the table CRC of the frame at byte `frame_start` recomputed: for tests that change a table field and want
    only the field checks to see it"""
    b = bytearray(buf)
    nb, bl, _ = _frame_shape(b, frame_start)
    T = tables_layout(nb, bl)
    crc = zlib.crc32(bytes(b[frame_start:frame_start + 24]) + bytes(b[frame_start + 32:frame_start + 32 + 4 * T["words"]]))
    b[frame_start + 24:frame_start + 28] = struct.pack("<I", crc)
    return bytes(b)


def with_header(c, version, flags, elem):
    """c with the version, flags and element-size words of its stream header rewritten and the header CRC recomputed"""
    h = c[:4] + struct.pack("<HHII", version, flags, struct.unpack("<I", c[8:12])[0], elem) + c[16:24]
    return h + struct.pack("<II", zlib.crc32(h), 0) + c[32:]


def corrupted_cases(c, x, n, rows, elem):
    """[(container, (what, frame, block))] and the layout: what the version-3 reader refuses, made from the valid version-3
    container c of x (writer n, rows, elem != 0, at least two frames, a kind-2 block that is not the last in frame 1)"""
    lay = layout(c)
    fr = lay["frames"][1]
    T = tables_layout(fr["nb"], fr["blk_len"])
    t0 = fr["tables"][0]
    k2 = [b for b, r in enumerate(fr["records"]) if r[2] == HUFF0][0]

    def poke(word_off, value, recrc=True):
        b = bytearray(c)
        b[t0 + 4 * word_off:t0 + 4 * word_off + 4] = struct.pack("<I", value)
        return retable(bytes(b), fr["start"]) if recrc else bytes(b)

    def resize(delta):
        """record k2 one word shorter / longer: the payload offsets behind it move, the payload keeps its size"""
        b = bytearray(c)
        W = np.frombuffer(bytes(b[t0:t0 + 4 * T["words"]]), np.uint32).copy()
        po = W[T["pay_off"]:T["pay_off"] + 2 * (fr["nb"] + 1)].view(np.uint64)
        if k2 + 1 < fr["nb"]:
            po[k2 + 1] += np.uint64(delta) if delta > 0 else np.uint64(0)
            if delta < 0:
                po[k2 + 1] -= np.uint64(-delta)
        else:
            return None
        b[t0:t0 + 4 * T["words"]] = W.tobytes()
        return retable(bytes(b), fr["start"])

    hist0 = struct.unpack("<I", c[t0 + 4 * (T["hist"] + 256 * k2):t0 + 4 * (T["hist"] + 256 * k2) + 4])[0]
    s, e, _ = fr["records"][k2]
    flipped = bytearray(c)
    flipped[(s + e) // 2] ^= 0x20
    v2 = write(x, n, rows, elem)
    lay2 = layout(v2)
    t2 = lay2["frames"][1]["tables"][0]
    kind2_in_v2 = bytearray(v2)
    kind2_in_v2[t2:t2 + 4] = struct.pack("<I", 2)
    cases = [(retable(bytes(kind2_in_v2), lay2["frames"][1]["start"]), (2, 1, 0)),      # kind 2 under a version-2 header
             (poke(T["kind"] + k2, 3), (2, 1, k2)),                                            # kind 3
             (poke(T["hist"] + 256 * k2, hist0 + 1), (2, 1, k2)),                              # the counts do not sum to blk_len
             (poke(T["bwt"] + k2, 1), (2, 1, k2)),
             (poke(T["enc_off"] + T["nsub"] * k2, 1), (2, 1, k2)),
             (poke(T["kind"] + k2, 3, recrc=False), (2, 1, -1)),                               # the table CRC sees it first
             (bytes(flipped), (3, 1, k2)),
             (with_header(c, 3, 0, 3), (1, -1, -1)), (with_header(c, 3, 0, 16), (1, -1, -1)), (with_header(c, 4, 0, elem), (1, -1, -1)),
             (with_header(c, 3, 0, 2 if elem != 2 else 4), (4, -1, -1))]                      # a legal but wrong elem: only crc_all
    for delta in (-1, 1):
        r = resize(delta)
        if r is not None:
            cases.append((r, (2, 1, k2)))
    return cases, lay


def refusal_cases(c4, c3, elem):
    """[(container, (what, frame, block))]: the refusal matrix of format version 4, made from the valid version-4 container c4 and
    the version-3 container c3 (shuffle only) of one input with the same plan shape and element size, at least two frames"""
    other = 2 if elem != 2 else 4
    lay = layout(c4)
    s, e, _ = lay["frames"][1]["records"][0]
    flipped = bytearray(c4)
    flipped[(s + e) // 2] ^= 0x20
    cases = [(with_header(c4, 4, f, elem), (1, -1, -1)) for f in (0, 2, 3, 0x8001, 0xFFFF)]      # flags 0 stays refused
    cases += [(with_header(c4, 4, 1, el), (1, -1, -1)) for el in (0, 1, 3, 16)]
    cases += [(with_header(c4, v, 1, elem), (1, -1, -1)) for v in (1, 2, 3, 5)]                  # the flag under another version
    cases += [(with_header(c3, 4, 1, elem), (4, -1, -1)),       # a version-3 container relabelled: every block passes, crc_all fails
              (with_header(c4, 3, 0, elem), (4, -1, -1)),       # ... and the reverse
              (with_header(c4, 4, 1, other), (4, -1, -1)),      # a legal but wrong elem
              (bytes(flipped), (3, 1, 0))]
    return cases, lay
