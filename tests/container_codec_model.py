"""Pure Python + numpy model of the container's order-0 Huffman codec (format version 3), on top of the
version-1 and version-2 models (tests/container_model.py, tests/container_filter_model.py: their layout, CRC helpers, shuffle
and BWT block coder are used as they are).

Version 3 differs from version 2 in three places: the stream header says `version = 3` and its element-size word may also be 0
(no filter); a block's kind may be 2, an ORDER-0 HUFFMAN RECORD; and the raw rule of that codec is rule (b) alone.  A kind-2
block stores hist[256] = its byte counts in the frame tables (bwt_index 0, enc_off zeros); the table is not stored, it is
hd_table_model.build_table(hist) (package-merge, <= 11 bits, canonical by (length, symbol)); the record is the codes of the
block's bytes packed MSB-first into 32-bit units, zero bits after the last code, one zero pad unit -- so it has exactly
ceil(sum hist * lens / 32) + 1 words, which the reader checks before it decodes anything.  The record is written and read here
in numpy alone (a bit scatter and a table walk), independent of the library's host encoder."""
import struct
import zlib

import numpy as np

import container_filter_model as F
import container_model as M
import hd_table_model as H
import oracle_lib as O
from container_model import ContainerError  # noqa: F401  (the same error class and codes for all versions)

VERSION_CODEC = 3
HUFF0 = 2
CODEC_BWT, CODEC_HUFF0 = 0, 1
ELEMS3 = (0, 2, 4, 8)


# ----------------------------------------------------------------------------------------------------------------------
# the order-0 record
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
            raise ContainerError(M.DECODED_CRC)                 # (cannot happen behind the reader's field checks)
        pos.append(p)
        p = step[p]
    return ts[win[np.asarray(pos, dtype=np.int64)]].astype(np.uint8) if n else np.zeros(0, np.uint8), p


def _raw_record(blk):
    nsub = (blk.size + M.HUFF_BLOCK - 1) // M.HUFF_BLOCK
    padded = np.zeros(4 * M.raw_words(blk.size), dtype=np.uint8)
    padded[:blk.size] = blk
    return M.RAW, 0, np.zeros(256, np.uint32), np.zeros(nsub, np.uint32), padded.view(np.uint32)


def encode_block(blk, codec):
    """(kind, bwt_index, hist, enc_off, record words) of one block; codec 0 = the BWT codec's rule and record, 1 = raw,
    2 = order-0 Huffman with its raw rule: raw when 4 * words >= blk_len"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    if codec == M.HUFF:
        return M.encode_block(blk)
    if codec == M.RAW:
        return _raw_record(blk)
    assert codec == HUFF0
    hist, words = h0_encode(blk)
    if 4 * words.size >= blk.size:
        return _raw_record(blk)
    nsub = (blk.size + M.HUFF_BLOCK - 1) // M.HUFF_BLOCK
    return HUFF0, 0, hist, np.zeros(nsub, np.uint32), words


# ----------------------------------------------------------------------------------------------------------------------
# writer
# ----------------------------------------------------------------------------------------------------------------------
def _frame(blocks, blk_len, codecs):
    nb = len(blocks)
    T = M.tables_layout(nb, blk_len)
    W = np.zeros(T["words"], dtype=np.uint32)
    recs, pay_off = [], [0]
    for b, blk in enumerate(blocks):
        kind, idx, hist, eo, words = encode_block(blk, codecs[b])
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
    hdr24 = M.MAGIC_FRAME + struct.pack("<III", nb, blk_len, 0) + struct.pack("<Q", P)
    tables = W.tobytes()
    payload = b"".join(w.tobytes() for w in recs) + (b"\0\0\0\0" if P & 1 else b"")
    return hdr24 + struct.pack("<II", zlib.crc32(hdr24 + tables), 0) + tables + payload


def write(data, block_len, rows, elem=0, codec=0, kinds=None):
    """The container of `data` as a writer plan of n = block_len, `rows` rows, shuffle element size `elem` and container codec
    `codec` makes it.  codec 0 without `kinds`: version 1 / 2, byte for byte container_filter_model.write.  codec 1: version 3,
    every block coded by the order-0 codec.  `kinds` (a sequence over the stream's blocks, cycled; each 0, 1 or 2) forces the
    codec of each block -- 0 the BWT codec, 1 raw, 2 order-0, every one still under its raw rule -- and so builds the mixed
    version-3 containers no GPU writer makes but every reader accepts."""
    if codec == CODEC_BWT and kinds is None:
        return F.write(data, block_len, rows, elem)
    if elem == 1:
        elem = 0
    assert elem in ELEMS3 and codec in (CODEC_BWT, CODEC_HUFF0)
    a = F._u8(data).reshape(-1)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    n = a.size
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION_CODEC, 0, block_len, elem) + struct.pack("<Q", n)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    pos, frames, nblk = 0, 0, 0
    while pos < n:                                             # (frames are cut exactly as in version 1)
        left = n - pos
        if left >= block_len:
            nb, bl = min(rows, left // block_len), block_len
        else:
            nb, bl = 1, left
        f = a[pos:pos + nb * bl]
        if elem:
            f = F.shuffle(f, elem)
        per = [HUFF0 if codec == CODEC_HUFF0 else M.HUFF] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(_frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        pos += nb * bl
        nblk += nb
        frames += 1
    t12 = M.MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


# ----------------------------------------------------------------------------------------------------------------------
# reader: the checks in the order the device path makes them
# ----------------------------------------------------------------------------------------------------------------------
def read(buf, with_kinds=False):
    """decoded bytes of a container of version 1, 2 or 3, or ContainerError(what, frame, block)"""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, z0, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if magic != M.MAGIC_STREAM or z0 or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20:
        raise ContainerError(M.STREAM_HEADER)
    if ver != VERSION_CODEC:
        return F.read(buf, with_kinds)                         # (kind 2 is a frame-table failure there)
    if elem not in ELEMS3:
        raise ContainerError(M.STREAM_HEADER)
    pos, done, fi = 32, 0, 0
    out, kinds = [], []
    while done < total:
        if pos + 32 + 16 > L:
            raise ContainerError(M.TRUNCATED, fi)
        fmagic, nb, bl, fz, P, tcrc, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        if (fmagic != M.MAGIC_FRAME or fz or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * M.raw_words(bl)):
            raise ContainerError(M.FRAME_TABLE, fi)
        T = M.tables_layout(nb, bl)
        fb = 32 + 4 * T["words"] + 4 * M._pad2(P)
        if pos + fb + 16 > L:
            raise ContainerError(M.TRUNCATED, fi)
        tb = buf[pos + 32: pos + 32 + 4 * T["words"]]
        if zlib.crc32(buf[pos:pos + 24] + tb) != tcrc:
            raise ContainerError(M.FRAME_TABLE, fi)
        W = np.frombuffer(tb, dtype=np.uint32)
        po = W[T["pay_off"]:T["pay_off"] + 2 * (nb + 1)].view(np.uint64).astype(np.int64)
        pay = np.frombuffer(buf[pos + 32 + 4 * T["words"]: pos + 32 + 4 * T["words"] + 4 * P], dtype=np.uint32)
        nsub = T["nsub"]
        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            wrong = kind > HUFF0 or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == HUFF0:                  # the counts are the block's, nothing else is set, and the
                wrong = (int(W[T["bwt"] + b]) != 0 or int(hist.astype(np.uint64).sum()) != bl or bool(eo.any())   # record has
                         or hi - lo != h0_words(hist))         # exactly the words the table of those counts asks for
            elif not wrong:
                wrong = (int(W[T["bwt"] + b]) >= bl or hi - lo > nsub * (M.MAX_WORDS + 1)
                         or any(int(eo[s]) >= hi - lo or (s and eo[s] <= eo[s - 1]) for s in range(nsub)))
            if wrong:
                bad.append((M.FRAME_TABLE, b))
            elif zlib.crc32(pay[lo:hi].tobytes()) != int(W[T["crc_rec"] + b]):
                bad.append((M.RECORD_CRC, b))
        if bad:
            what, b = min(bad)
            raise ContainerError(what, fi, b)
        blocks = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            if kind == M.RAW:
                blk = pay[lo:hi].view(np.uint8)[:bl]
            elif kind == HUFF0:
                blk, used = h0_decode(hist, pay[lo:hi], bl)
                assert (used + 31) // 32 + 1 == hi - lo        # decoding blk_len symbols consumes the record exactly
            else:
                blk = O.decompress(int(W[T["bwt"] + b]), hist, W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):      # (of the SHUFFLED frame's block when elem != 0)
                raise ContainerError(M.DECODED_CRC, fi, b)
            blocks.append(blk)
            kinds.append(kind)
        frame = np.concatenate(blocks)
        out.append(F.unshuffle(frame, elem) if elem else frame)
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > L:
        raise ContainerError(M.TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != M.MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != L:
        raise ContainerError(M.STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:
        raise ContainerError(M.DECODED_CRC)
    return (data, kinds) if with_kinds else data


def retable(buf, frame_start):
    """`buf` with the table CRC of the frame at byte `frame_start` recomputed: for tests that change a table field and want
    only the field checks to see it"""
    b = bytearray(buf)
    _, nb, bl, _, _, _, _ = struct.unpack("<4sIIIQII", bytes(b[frame_start:frame_start + 32]))
    T = M.tables_layout(nb, bl)
    crc = zlib.crc32(bytes(b[frame_start:frame_start + 24]) + bytes(b[frame_start + 32:frame_start + 32 + 4 * T["words"]]))
    b[frame_start + 24:frame_start + 28] = struct.pack("<I", crc)
    return bytes(b)


def with_header(c, version, elem):
    """c with the version and element-size words of its stream header rewritten and the header CRC recomputed"""
    h = c[:4] + struct.pack("<HHII", version, 0, struct.unpack("<I", c[8:12])[0], elem) + c[16:24]
    return h + struct.pack("<II", zlib.crc32(h), 0) + c[32:]


def corrupted_cases(c, x, n, rows, elem):
    """[(container, (what, frame, block))] and the layout: what the version-3 reader refuses, made from the valid version-3
    container c of x (writer n, rows, elem != 0, at least two frames, a kind-2 block that is not the last in frame 1)"""
    lay = M.layout(c)
    fr = lay["frames"][1]
    T = M.tables_layout(fr["nb"], fr["blk_len"])
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
    v2 = F.write(x, n, rows, elem)
    lay2 = M.layout(v2)
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
             (with_header(c, 3, 3), (1, -1, -1)), (with_header(c, 3, 16), (1, -1, -1)), (with_header(c, 4, elem), (1, -1, -1)),
             (with_header(c, 3, 2 if elem != 2 else 4), (4, -1, -1))]                         # a legal but wrong elem: only crc_all
    for delta in (-1, 1):
        r = resize(delta)
        if r is not None:
            cases.append((r, (2, 1, k2)))
    return cases, lay
