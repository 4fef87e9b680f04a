"""Pure Python + numpy model of the 2-D (row-stride) predictor of the container's typed-data filter (csrc/grid.hip) and of format
version 12 (INTEGRATION.md 4b "Delta: grid"), built from the parts of lag_model, auto_model and container_model.

  x[i]: element i of a segment as a little-endian unsigned integer of elem = 2, 4 or 8 bytes, arithmetic modulo 2^(8 elem),
  RUN = 2048, W the row width in elements, 2 <= W <= 65536, P = 2048 ceil(W / 64) the period (a band: about 32 rows), fold 0 or 1:
    v[i] = x[i] where i mod P < W, else x[i] - x[i - W]             (the top row of a band has no row above inside the band)
    d[i] = v[i] where i mod RUN == 0, else v[i] - v[i - 1]          (the plain delta's restart)
    f[i] = d[i], or with the fold (d[i] << 1) ^ (0 - (d[i] >> (8 elem - 1)))
    out[j q + i] = byte j of f[i], q = len // elem; the last len % elem bytes in place
  So the transform is lag_model's at (1, fold) over v, and the inverse is lag_model's inverse at (1, fold), which gives v, followed
  by x[i] = v[i] + x[i - W] for i mod P >= W down every band.  Bands are independent and runs nest inside bands, so the range form
  takes a `first` that is a multiple of P.

Version 12 is version 8's stream (auto_model: kinds 1, 2, 3, 5 per block from the auto rule, frame word 0) whose frames went through
this filter as one segment each; the header's flags are 1 | fold << 1 | 4 and its word 3 is elem | width << 8.  The reader of a plan
with the setting on speaks versions 1 to 5, 7, 8 and 12."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import filter_auto_model as F
import lag_model as L

VERSION = 12
RUN = M.RUN
MIN_WIDTH, MAX_WIDTH = 2, 65536
FLAG_FOLD, FLAG_GRID = 2, 4
READS = frozenset(("sparse", "ans", "auto", "grid"))              # what a plan with the setting on speaks


def period(width):
    return RUN * ((width + 63) // 64)


# ----------------------------------------------------------------------------------------------------------------------
# the transform
# ----------------------------------------------------------------------------------------------------------------------
def _check(elem, width, fold):
    assert elem in M.ELEMS and MIN_WIDTH <= width <= MAX_WIDTH and fold in (0, 1)


def _split(data, elem):
    a = np.ascontiguousarray(M._u8(data).reshape(-1))
    m = a.size - a.size % elem
    return a[:m].view("<u%d" % elem), a[m:]


def _vdiff(x, width):
    """v of x: the row above subtracted wherever it lies in the same band"""
    v = x.copy()
    i = np.flatnonzero(np.arange(x.size) % period(width) >= width)
    v[i] = x[i] - x[i - width]
    return v


def _vsum(v, width):
    """x of v, band by band: the running sum down every column of a band's rows"""
    P = period(width)
    x = np.empty_like(v)
    for b in range(0, v.size, P):
        band = v[b:b + P]
        rows = -(-band.size // width)
        pad = np.zeros(rows * width, v.dtype)
        pad[:band.size] = band
        x[b:b + P] = np.cumsum(pad.reshape(rows, width), axis=0, dtype=v.dtype).reshape(-1)[:band.size]
    return x


def grid_delta_shuffle(data, elem, width, fold):
    _check(elem, width, fold)
    x, tail = _split(data, elem)
    return L.lag_delta_shuffle(np.concatenate([_vdiff(x, width).view(np.uint8), tail]), elem, 1, fold)


def ungrid_delta_unshuffle(data, elem, width, fold):
    _check(elem, width, fold)
    v, tail = _split(L.unlag_delta_unshuffle(data, elem, 1, fold), elem)
    return np.concatenate([_vsum(v, width).view(np.uint8), tail])


def ungrid_delta_unshuffle_range(data, elem, width, fold, first, count):
    """the bytes of elements [first, first + count) of ungrid_delta_unshuffle(data, ...), from the plane runs alone; first % P == 0"""
    _check(elem, width, fold)
    assert first % period(width) == 0
    v = np.ascontiguousarray(L.unlag_delta_unshuffle_range(data, elem, 1, fold, first, count)).view("<u%d" % elem)
    return _vsum(v, width).view(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# format version 12
# ----------------------------------------------------------------------------------------------------------------------
def flags_of(fold):
    return M.FLAG_DELTA | fold << 1 | FLAG_GRID


def word3_of(elem, width):
    return elem | width << 8


def flags_legal(flags):
    return flags & ~FLAG_FOLD == M.FLAG_DELTA | FLAG_GRID


def format_legal(version, flags, word3):
    """the whole format rule, as the library's format_legal() over the header's words: lag_model's for every other version (word 3
    is the element size there, whole), and version 12's family, whose word 3 is elem | width << 8"""
    if version == VERSION:
        return flags_legal(flags) and (word3 & 255) in M.ELEMS and MIN_WIDTH <= word3 >> 8 <= MAX_WIDTH
    return L.format_legal(version, flags, word3)


def write(data, block_len, rows, elem, width, fold, kinds=None):
    """The container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode, the shuffle at
    `elem`, the delta and the grid setting (width, fold) makes it: version 12."""
    _check(elem, width, fold)
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION, flags_of(fold), block_len, word3_of(elem, width)) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    nblk = 0
    frames = F.cut(a.size, block_len, rows)
    for pos, nb, bl in frames:
        f = grid_delta_shuffle(a[pos:pos + nb * bl], elem, width, fold)
        per = ["rule"] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        nblk += nb
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, reads=READS):
    """decoded bytes of a container as the reader of a plan that speaks `reads` sees it, or ContainerError(what, frame, block).
    READS is a plan with the setting on (versions 1 to 5, 7, 8 and 12); without "grid" version 12 is a stream-header failure; every
    other version is lag_model's reader's.  Width and fold come from the stream header."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        return L.read(buf, reads=frozenset(reads) - {"grid"})
    h = buf[:32]
    magic, _, flags, block_len, word3, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or not format_legal(ver, flags, word3) or "grid" not in reads):
        raise M.ContainerError(M.STREAM_HEADER)
    elem, width, fold = word3 & 255, word3 >> 8, flags >> 1 & 1
    Lb = len(buf)
    pos, done, fi = 32, 0, 0
    out = []
    while done < total:
        if pos + 32 + 16 > Lb:
            raise M.ContainerError(M.TRUNCATED, fi)
        fmagic, nb, bl, word, P, _, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        if (fmagic != M.MAGIC_FRAME or word or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * M.raw_words(bl)):
            raise M.ContainerError(M.FRAME_TABLE, fi)
        fb = 32 + 4 * M.tables_layout(nb, bl)["words"] + 4 * M._pad2(P)
        if pos + fb + 16 > Lb:
            raise M.ContainerError(M.TRUNCATED, fi)
        out.append(ungrid_delta_unshuffle(F._frame_blocks(buf, pos, nb, bl, P, fi), elem, width, fold))     # (version 8's frame)
        pos += fb
        done += nb * bl
        fi += 1
    if pos + 16 > Lb:
        raise M.ContainerError(M.TRUNCATED, fi)
    emagic, frames, crc_all, tcrc = struct.unpack("<4sIII", buf[pos:pos + 16])
    if emagic != M.MAGIC_END or frames != fi or tcrc != zlib.crc32(buf[pos:pos + 12]) or pos + 16 != Lb:
        raise M.ContainerError(M.STREAM_HEADER, fi)
    data = np.concatenate(out) if out else np.zeros(0, np.uint8)
    if zlib.crc32(data.tobytes()) != crc_all:
        raise M.ContainerError(M.DECODED_CRC)
    return data


def range_first(i, width):
    """the element a range read that needs element i starts its inverse at: the start of i's band"""
    return i - i % period(width)


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 12, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c12, c11):
    """[(name, container, (what, frame, block), reads)] from the valid version-12 container c12 and a valid version-11 one: what the
    reader of a plan that speaks `reads` answers.  c12 needs a frame of two or more blocks."""
    lay = M.layout(c12)
    _, flags, _, word3 = struct.unpack("<HHII", c12[4:16])
    elem, width = word3 & 255, word3 >> 8
    none = (M.STREAM_HEADER, -1, -1)
    hdr = lambda fl, w3=word3: M.with_header(c12, VERSION, fl, w3)
    cases = [("flags without bit 2", hdr(flags & ~FLAG_GRID), none),
             ("flags with bit 3", hdr(flags | 8), none),
             ("flags with bit 0 clear", hdr(flags & ~1), none),
             ("a non-zero lag field", hdr(flags | 2 << L.LAG_SHIFT), none),
             ("flags with bit 15 set", hdr(flags | 0x8000), none),
             ("width 0", hdr(flags, word3_of(elem, 0)), none),
             ("width 1", hdr(flags, word3_of(elem, 1)), none),
             ("width 65537", hdr(flags, word3_of(elem, 65537)), none),
             ("elem 3", hdr(flags, word3_of(3, width)), none),
             ("elem 0", hdr(flags, word3_of(0, width)), none),
             ("version 8 with this word 3", M.with_header(c12, U.VERSION, 1, word3), none),
             ("version 11 with these words", M.with_header(c12, L.VERSION, flags, word3), none),
             ("version 13", M.with_header(c12, 13, flags, word3), none)]
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    x = bytearray(c12)
    x[fr["start"] + 12:fr["start"] + 16] = struct.pack("<I", elem)
    cases.append(("a non-zero frame word", M.retable(bytes(x), fr["start"]), (M.FRAME_TABLE, multi, -1)))
    s, e, _ = fr["records"][1]
    flipped = bytearray(c12)
    flipped[(s + e) // 2] ^= 0x20
    cases.append(("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1)))
    other = width + 1 if width < MAX_WIDTH else width - 1
    cases += [("a legal but wrong width: only crc_all sees it", hdr(flags, word3_of(elem, other)), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong fold: only crc_all sees it", hdr(flags ^ FLAG_FOLD), (M.DECODED_CRC, -1, -1)),
              ("cut inside the last frame", c12[:lay["trailer"] - 8], (M.TRUNCATED, len(lay["frames"]) - 1, -1))]
    cases = [c + (READS,) for c in cases]
    cases += [("version 12 to a lag plan", c12, none, L.READS),
              ("version 12 to an auto plan", c12, none, U.READS_AUTO),
              ("version 12 to a filter-auto plan", c12, none, F.READS),
              ("version 12 to a plain plan", c12, none, frozenset()),
              ("version 11 to a grid plan", c11, none, READS)]
    return cases, lay
