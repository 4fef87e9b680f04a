"""Pure Python + numpy model of the delta mode of the container's typed-data filter (format version 4), on
top of the models of versions 1 to 3 (tests/container_model.py, container_filter_model.py, container_codec_model.py: their
layout, CRC helpers, shuffle, block coders and frame writer are used as they are).

Version 4 differs from version 3 in two places.  The stream header says `version = 4` and the u16 behind it, zero in versions 1
to 3, holds flags = 1 (bit 0: delta; any other value is refused), with an element size of 2, 4 or 8.  Every frame's nb * blk_len
input bytes go through delta + shuffle as ONE segment before the frame's blocks are cut: with x[i] element i as a little-endian
unsigned integer, d[i] = x[i] where i % RUN == 0, else x[i] - x[i - 1] modulo 2^(8 elem); the shuffle of version 2 is then applied
to d.  Frames, tables, records of all three kinds, the trailer and every check are version 3's; crc_raw[b] is the CRC of block b
of the filtered frame, crc_all that of the original input."""
import struct
import zlib

import numpy as np

import container_codec_model as K
import container_filter_model as F
import container_model as M
import oracle_lib as O
from container_model import ContainerError  # noqa: F401  (the same error class and codes for all versions)

VERSION_DELTA = 4
FLAG_DELTA = 1
RUN = 2048
ELEMS = F.ELEMS


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
    return F.shuffle(_delta(np.ascontiguousarray(F._u8(data).reshape(-1)), elem), elem)


def undelta_unshuffle(data, elem):
    assert elem in ELEMS
    return _undelta(np.ascontiguousarray(F.unshuffle(data, elem)), elem)


def write(data, block_len, rows, elem=0, codec=0, delta=False, kinds=None):
    """The container of `data` as a writer plan of n = block_len, `rows` rows, shuffle element size `elem`, container codec
    `codec` and delta mode `delta` makes it.  delta off: versions 1 to 3, byte for byte container_codec_model.write.  delta on
    (elem 2, 4 or 8): version 4, every block coded by the plan's codec, or as `kinds` forces (see container_codec_model.write)."""
    if not delta:
        return K.write(data, block_len, rows, elem, codec, kinds)
    assert elem in ELEMS and codec in (K.CODEC_BWT, K.CODEC_HUFF0)
    a = F._u8(data).reshape(-1)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    n = a.size
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION_DELTA, FLAG_DELTA, block_len, elem) + struct.pack("<Q", n)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    pos, frames, nblk = 0, 0, 0
    while pos < n:                                             # (frames are cut exactly as in version 1)
        left = n - pos
        if left >= block_len:
            nb, bl = min(rows, left // block_len), block_len
        else:
            nb, bl = 1, left
        f = delta_shuffle(a[pos:pos + nb * bl], elem)          # element numbering restarts with the frame
        per = [K.HUFF0 if codec == K.CODEC_HUFF0 else M.HUFF] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(K._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        pos += nb * bl
        nblk += nb
        frames += 1
    t12 = M.MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, with_kinds=False):
    """decoded bytes of a container of version 1, 2, 3 or 4, or ContainerError(what, frame, block); the checks in the order the
    device path makes them"""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if ver != VERSION_DELTA:
        return K.read(buf, with_kinds)                         # (which refuses flags != 0)
    if (magic != M.MAGIC_STREAM or flags != FLAG_DELTA or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or elem not in ELEMS):
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
        for b in range(nb):                                    # the field checks of version 3
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            wrong = kind > K.HUFF0 or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == K.HUFF0:
                wrong = (int(W[T["bwt"] + b]) != 0 or int(hist.astype(np.uint64).sum()) != bl or bool(eo.any())
                         or hi - lo != K.h0_words(hist))
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
            elif kind == K.HUFF0:
                blk, used = K.h0_decode(hist, pay[lo:hi], bl)
                assert (used + 31) // 32 + 1 == hi - lo
            else:
                blk = O.decompress(int(W[T["bwt"] + b]), hist, W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):      # (of the FILTERED frame's block)
                raise ContainerError(M.DECODED_CRC, fi, b)
            blocks.append(blk)
            kinds.append(kind)
        out.append(undelta_unshuffle(np.concatenate(blocks), elem))       # the frame is one segment
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > L:
        raise ContainerError(M.TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != M.MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != L:
        raise ContainerError(M.STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:                  # only this sees a wrong elem or a wrong flag: the ORIGINAL bytes
        raise ContainerError(M.DECODED_CRC)
    return (data, kinds) if with_kinds else data


def with_header(c, version, flags, elem):
    """c with the version, flags and element-size words of its stream header rewritten and the header CRC recomputed"""
    h = c[:4] + struct.pack("<HHII", version, flags, struct.unpack("<I", c[8:12])[0], elem) + c[16:24]
    return h + struct.pack("<II", zlib.crc32(h), 0) + c[32:]


def refusal_cases(c4, c3, elem):
    """[(container, (what, frame, block))]: the refusal matrix of format version 4, made from the valid version-4 container c4 and
    the version-3 container c3 (shuffle only) of one input with the same plan shape and element size, at least two frames"""
    other = 2 if elem != 2 else 4
    lay = M.layout(c4)
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
