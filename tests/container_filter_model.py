"""Pure Python + numpy model of the BWT container's byte-plane shuffle filter (format version 2), on top
of the version-1 model (tests/container_model.py, whose frame writer, layout and CRC helpers are used as they are).

Version 2 differs from version 1 in three places: the stream header says `version = 2` and carries the element size (2, 4 or 8)
in the word behind block_len; every frame's nb * blk_len input bytes are shuffled as ONE segment before the frame's blocks are
cut from them (so crc_raw[b] is the CRC of block b of the shuffled frame); the trailer's crc_all is still the CRC of the
original input, which the reader can only compare after it has unshuffled every frame."""
import struct
import zlib

import numpy as np

import container_model as M
import oracle_lib as O
from container_model import ContainerError  # noqa: F401  (the same error class and codes for both versions)

VERSION_SHUFFLE = 2
ELEMS = (2, 4, 8)


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


def write(data, block_len, rows, elem=0):
    """the container of `data` as a writer plan of n = block_len, `rows` rows and shuffle element size `elem` makes it
    (elem 0 or 1: no filter, version 1, byte for byte container_model.write)"""
    if elem in (0, 1):
        return M.write(data, block_len, rows)
    assert elem in ELEMS
    a = _u8(data).reshape(-1)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    n = a.size
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION_SHUFFLE, 0, block_len, elem) + struct.pack("<Q", n)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    pos, frames = 0, 0
    while pos < n:                                             # (frames are cut exactly as in version 1)
        left = n - pos
        if left >= block_len:
            nb, bl = min(rows, left // block_len), block_len
        else:
            nb, bl = 1, left
        f = shuffle(a[pos:pos + nb * bl], elem)
        out.append(M._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl))
        pos += nb * bl
        frames += 1
    t12 = M.MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def header_elem(buf):
    """the element size a valid stream header names (0 for version 1)"""
    return struct.unpack("<I", bytes(buf[12:16]))[0]


def read(buf, with_kinds=False):
    """decoded bytes of a container of either version, or ContainerError(what, frame, block); the checks in the order the
    device path makes them (container_model.read's, with the unshuffle in front of the crc_all comparison)"""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, z0, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if magic != M.MAGIC_STREAM or z0 or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20:
        raise ContainerError(M.STREAM_HEADER)
    if not ((ver == M.VERSION and elem == 0) or (ver == VERSION_SHUFFLE and elem in ELEMS)):
        raise ContainerError(M.STREAM_HEADER)
    if ver == M.VERSION:
        return M.read(buf, with_kinds)
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
            if (kind > M.RAW or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
                    or (kind == M.RAW and hi - lo != M.raw_words(bl))
                    or (kind == M.HUFF and (int(W[T["bwt"] + b]) >= bl or hi - lo > nsub * (M.MAX_WORDS + 1)
                                            or any(int(eo[s]) >= hi - lo or (s and eo[s] <= eo[s - 1]) for s in range(nsub))))):
                bad.append((M.FRAME_TABLE, b))
            elif zlib.crc32(pay[lo:hi].tobytes()) != int(W[T["crc_rec"] + b]):
                bad.append((M.RECORD_CRC, b))
        if bad:
            what, b = min(bad)
            raise ContainerError(what, fi, b)
        blocks = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            if kind == M.RAW:
                blk = pay[lo:hi].view(np.uint8)[:bl]
            else:
                blk = O.decompress(int(W[T["bwt"] + b]), W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)],
                                   W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):      # (of the SHUFFLED frame's block)
                raise ContainerError(M.DECODED_CRC, fi, b)
            blocks.append(blk)
            kinds.append(kind)
        out.append(unshuffle(np.concatenate(blocks), elem))                # the frame is one segment
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > L:
        raise ContainerError(M.TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != M.MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != L:
        raise ContainerError(M.STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:                  # only this sees a wrong elem: it covers the ORIGINAL bytes
        raise ContainerError(M.DECODED_CRC)
    return (data, kinds) if with_kinds else data
