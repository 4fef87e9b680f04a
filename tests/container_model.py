"""Pure Python + numpy model of the BWT container: the second, independent implementation of the format.
Huffman records come from the oracle (oracle_lib.compress / decompress), CRCs from zlib.crc32.  Also the CRC algebra the
device kernel uses (raw CRCs, shifts by x^(8n) mod P, granule rows), written out so that it can be checked against zlib."""
import struct
import zlib

import numpy as np

import oracle_lib as O

MAGIC_STREAM, MAGIC_FRAME, MAGIC_END = b"GLCB", b"GLCF", b"GLCE"
VERSION = 1
HUFF, RAW = 0, 1
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
# writer
# ----------------------------------------------------------------------------------------------------------------------
def encode_block(blk):
    """(kind, bwt_index, hist, enc_off, record words) of one block, by the raw rule"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    nsub = (blk.size + HUFF_BLOCK - 1) // HUFF_BLOCK
    r = O.compress(blk)
    if r["rc"] != 0 or 4 * r["size"] >= blk.size:
        padded = np.zeros(4 * raw_words(blk.size), dtype=np.uint8)
        padded[:blk.size] = blk
        return RAW, 0, np.zeros(256, np.uint32), np.zeros(nsub, np.uint32), padded.view(np.uint32)
    return HUFF, r["bwt_index"], r["hist"], np.asarray(r["offsets"], np.uint32), np.asarray(r["words"], np.uint32)


def _frame(blocks, blk_len):
    nb = len(blocks)
    T = tables_layout(nb, blk_len)
    W = np.zeros(T["words"], dtype=np.uint32)
    recs, pay_off = [], [0]
    for b, blk in enumerate(blocks):
        kind, idx, hist, eo, words = encode_block(blk)
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


def write(data, block_len, rows):
    """the container of `data` (bytes / uint8 array) as a writer plan of n = block_len and `rows` rows makes it"""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, np.uint8)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    n = a.size
    hdr24 = MAGIC_STREAM + struct.pack("<HHII", VERSION, 0, block_len, 0) + struct.pack("<Q", n)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    pos, frames = 0, 0
    while pos < n:
        left = n - pos
        if left >= block_len:
            nb, bl = min(rows, left // block_len), block_len
        else:
            nb, bl = 1, left
        out.append(_frame([a[pos + i * bl: pos + (i + 1) * bl] for i in range(nb)], bl))
        pos += nb * bl
        frames += 1
    t12 = MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


# ----------------------------------------------------------------------------------------------------------------------
# reader: the checks in the order the device path makes them
# ----------------------------------------------------------------------------------------------------------------------
def read(buf, with_kinds=False):
    """decoded bytes of a container, or ContainerError(what, frame, block)"""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise ContainerError(TRUNCATED)
    h = buf[:32]
    magic, ver, z0, block_len, z1, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if magic != MAGIC_STREAM or ver != VERSION or z0 or z1 or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20:
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
        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            nsub = T["nsub"]
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            if (kind > RAW or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
                    or (kind == RAW and hi - lo != raw_words(bl))
                    or (kind == HUFF and (int(W[T["bwt"] + b]) >= bl or hi - lo > nsub * (MAX_WORDS + 1)
                                          or any(int(eo[s]) >= hi - lo or (s and eo[s] <= eo[s - 1]) for s in range(nsub))))):
                bad.append((FRAME_TABLE, b))
            elif zlib.crc32(pay[lo:hi].tobytes()) != int(W[T["crc_rec"] + b]):
                bad.append((RECORD_CRC, b))
        if bad:
            what, b = min(bad)
            raise ContainerError(what, fi, b)
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            if kind == RAW:
                blk = pay[lo:hi].view(np.uint8)[:bl]
            else:
                nsub = T["nsub"]
                blk = O.decompress(int(W[T["bwt"] + b]), W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)],
                                   W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):
                raise ContainerError(DECODED_CRC, fi, b)
            out.append(blk)
            kinds.append(kind)
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > L:
        raise ContainerError(TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != L:
        raise ContainerError(STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:
        raise ContainerError(DECODED_CRC)
    return (data, kinds) if with_kinds else data


def layout(buf):
    """byte ranges of a valid container's parts, for tests that corrupt one of them: a list of frames, each a dict with
    'start', 'tables' (start, end), 'payload' start, 'records' [(start, end, kind)] in bytes"""
    buf = bytes(buf)
    pos, frames = 32, []
    total = struct.unpack("<Q", buf[16:24])[0]
    done = 0
    while done < total:
        _, nb, bl, _, P, _, _ = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        T = tables_layout(nb, bl)
        W = np.frombuffer(buf[pos + 32: pos + 32 + 4 * T["words"]], dtype=np.uint32)
        po = W[T["pay_off"]:T["pay_off"] + 2 * (nb + 1)].view(np.uint64)
        ps = pos + 32 + 4 * T["words"]
        frames.append(dict(start=pos, nb=nb, blk_len=bl, tables=(pos + 32, ps), payload=ps,
                           records=[(ps + 4 * int(po[b]), ps + 4 * int(po[b + 1]), int(W[T["kind"] + b])) for b in range(nb)]))
        pos = ps + 4 * _pad2(P)
        done += nb * bl
    return dict(frames=frames, trailer=pos)
