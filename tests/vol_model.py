"""Pure Python + numpy model of the 3-D (plane-stride) predictor of the container's typed-data filter (csrc/vol.hip) and of format
version 17 (INTEGRATION.md 4b "Delta: volume"), built on grid_model (and through it lag_model, auto_model and container_model).

  x[i]: element i of a segment as a little-endian unsigned integer of elem = 2, 4 or 8 bytes, arithmetic modulo 2^(8 elem),
  RUN = 2048, W the row width, 2 <= W <= 65536, P = 2048 ceil(W / 64), S the plane stride in elements, W < S <= 2^24, and the slab
  Q = P ceil(16 S / P) (about 16 planes, a multiple of P):
    w[i] = x[i] where i mod Q < S, else x[i] - x[i - S]             (the first plane of a slab has nothing behind it inside the slab)
    then grid_model's transform of w at (W, fold)
  The inverse is grid_model's inverse, which gives w, followed by x[i] = w[i] + x[i - S] for i mod Q >= S up every slab.  Slabs are
  independent, bands nest inside slabs and runs inside bands, so the range form takes a `first` that is a multiple of Q.  With
  S >= q no element has a plane behind it and the bytes are grid_model's.

Version 17 is version 12's stream whose frames went through this filter: the header's flags are 1 | fold << 1 | 4 | 8, its word 3 is
elem | width << 8, its word 7 is S (every other version keeps word 7 at 0) and its word 6 is the CRC-32 of words 0..5 followed by
word 7.  The reader of a plan with the setting on speaks versions 1 to 5, 7, 8, 12 and 17."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import filter_auto_model as F
import grid_model as G
import lag_model as L

VERSION = 17
RUN = M.RUN
MAX_PLANE = 1 << 24
PLANES = 16
FLAG_VOL = 8
READS = frozenset(("sparse", "ans", "auto", "grid", "vol"))       # what a plan with the setting on speaks


def slab(width, plane):
    P = G.period(width)
    return P * -(-PLANES * plane // P)


def plane_ok(width, plane):
    return width < plane <= MAX_PLANE


# ----------------------------------------------------------------------------------------------------------------------
# the transform
# ----------------------------------------------------------------------------------------------------------------------
def _check(elem, width, plane, fold):
    G._check(elem, width, fold)
    assert plane_ok(width, plane)


def _zdiff(x, width, plane):
    """w of x: the plane behind subtracted wherever it lies in the same slab"""
    w = x.copy()
    i = np.flatnonzero(np.arange(x.size) % slab(width, plane) >= plane)
    w[i] = x[i] - x[i - plane]
    return w


def _zsum(w, width, plane):
    """x of w, slab by slab: the running sum along every column of a slab's planes"""
    Q = slab(width, plane)
    x = np.empty_like(w)
    for b in range(0, w.size, Q):
        s = w[b:b + Q]
        n = -(-s.size // plane)
        pad = np.zeros(n * plane, w.dtype)
        pad[:s.size] = s
        x[b:b + Q] = np.cumsum(pad.reshape(n, plane), axis=0, dtype=w.dtype).reshape(-1)[:s.size]
    return x


def vol_delta_shuffle(data, elem, width, plane, fold):
    _check(elem, width, plane, fold)
    x, tail = G._split(data, elem)
    return G.grid_delta_shuffle(np.concatenate([_zdiff(x, width, plane).view(np.uint8), tail]), elem, width, fold)


def unvol_delta_unshuffle(data, elem, width, plane, fold):
    _check(elem, width, plane, fold)
    w, tail = G._split(G.ungrid_delta_unshuffle(data, elem, width, fold), elem)
    return np.concatenate([_zsum(w, width, plane).view(np.uint8), tail])


def unvol_delta_unshuffle_range(data, elem, width, plane, fold, first, count):
    """the bytes of elements [first, first + count) of unvol_delta_unshuffle(data, ...), from the plane runs alone; first % Q == 0"""
    _check(elem, width, plane, fold)
    assert first % slab(width, plane) == 0
    w = np.ascontiguousarray(G.ungrid_delta_unshuffle_range(data, elem, width, fold, first, count)).view("<u%d" % elem)
    return _zsum(w, width, plane).view(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# format version 17
# ----------------------------------------------------------------------------------------------------------------------
def flags_of(fold):
    return G.flags_of(fold) | FLAG_VOL


def flags_legal(flags):
    return flags & ~G.FLAG_FOLD == M.FLAG_DELTA | G.FLAG_GRID | FLAG_VOL


def format_legal(version, flags, word3, word7=0):
    """the whole format rule over the header's words: version 17's family -- word 3 elem | width << 8, word 7 the plane stride --
    and for every other version grid_model's with word 7 at 0"""
    if version == VERSION:
        return flags_legal(flags) and (word3 & 255) in M.ELEMS and G.MIN_WIDTH <= word3 >> 8 <= G.MAX_WIDTH and plane_ok(word3 >> 8, word7)
    return word7 == 0 and G.format_legal(version, flags, word3)


def header_crc(h):
    """word 6 of the 32 header bytes h as version 17 counts it: the CRC-32 of words 0..5 followed by word 7"""
    return zlib.crc32(h[:24] + h[28:32])


def with_header(c, version, flags, word3, word7):
    """container c under another stream header, the CRC made good under the rule of the version it now names"""
    h = bytearray(c[:32])
    h[4:8] = struct.pack("<HH", version, flags)
    h[12:16] = struct.pack("<I", word3)
    h[28:32] = struct.pack("<I", word7)
    h[24:28] = struct.pack("<I", header_crc(bytes(h)) if version == VERSION else zlib.crc32(bytes(h[:24])))
    return bytes(h) + c[32:]


def write(data, block_len, rows, elem, width, plane, fold, kinds=None):
    """The container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode, the shuffle at
    `elem`, the delta, the grid setting (width, fold) and the volume setting `plane` makes it: version 17."""
    _check(elem, width, plane, fold)
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION, flags_of(fold), block_len, G.word3_of(elem, width)) + struct.pack("<Q", a.size)
    w7 = struct.pack("<I", plane)
    out = [hdr24 + struct.pack("<I", zlib.crc32(hdr24 + w7)) + w7]
    nblk = 0
    frames = F.cut(a.size, block_len, rows)
    for pos, nb, bl in frames:
        f = vol_delta_shuffle(a[pos:pos + nb * bl], elem, width, plane, fold)
        per = ["rule"] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        nblk += nb
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, reads=READS):
    """decoded bytes of a container as the reader of a plan that speaks `reads` sees it, or ContainerError(what, frame, block).
    READS is a plan with the setting on (versions 1 to 5, 7, 8, 12 and 17); without "vol" version 17 is a stream-header failure;
    every other version is grid_model's reader's (which wants word 7 at 0).  Width, plane and fold come from the stream header."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        return G.read(buf, reads=frozenset(reads) - {"vol"})
    h = buf[:32]
    magic, _, flags, block_len, word3, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, word7 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or hcrc != header_crc(h) or not 1 <= block_len <= 1 << 20
            or not format_legal(ver, flags, word3, word7) or "vol" not in reads):
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
        out.append(unvol_delta_unshuffle(F._frame_blocks(buf, pos, nb, bl, P, fi), elem, width, word7, fold))   # (version 8's frame)
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


def range_first(i, width, plane):
    """the element a range read that needs element i starts its inverse at: the start of i's slab"""
    return i - i % slab(width, plane)


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 17, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c17, c12):
    """[(name, container, (what, frame, block), reads)] from the valid version-17 container c17 and a valid version-12 one: what the
    reader of a plan that speaks `reads` answers."""
    lay = M.layout(c17)
    _, flags, _, word3 = struct.unpack("<HHII", c17[4:16])
    plane = struct.unpack("<I", c17[28:32])[0]
    elem, width = word3 & 255, word3 >> 8
    _, f12, _, w12 = struct.unpack("<HHII", c12[4:16])
    none = (M.STREAM_HEADER, -1, -1)
    hdr = lambda fl=flags, w3=word3, w7=plane: with_header(c17, VERSION, fl, w3, w7)
    stale = bytearray(c17)
    stale[28:32] = struct.pack("<I", plane + 1)                  # (word 6 left as it was: the CRC covers word 7)
    old_crc = bytearray(c17)
    old_crc[24:28] = struct.pack("<I", zlib.crc32(c17[:24]))     # (the CRC of words 0..5 alone, as every other version counts it)
    cases = [("flags without bit 3", hdr(flags & ~FLAG_VOL), none),
             ("flags without bit 2", hdr(flags & ~G.FLAG_GRID), none),
             ("flags with bit 0 clear", hdr(flags & ~1), none),
             ("flags with bit 4", hdr(flags | 16), none),
             ("a non-zero lag field", hdr(flags | 2 << L.LAG_SHIFT), none),
             ("plane 0", hdr(w7=0), none),
             ("plane == width", hdr(w7=width), none),
             ("plane 2^24 + 1", hdr(w7=MAX_PLANE + 1), none),
             ("width 1", hdr(w3=G.word3_of(elem, 1)), none),
             ("width 65537", hdr(w3=G.word3_of(elem, 65537)), none),
             ("elem 3", hdr(w3=G.word3_of(3, width)), none),
             ("elem 1", hdr(w3=G.word3_of(1, width)), none),
             ("word 7 changed under the old CRC", bytes(stale), none),
             ("word 6 over words 0..5 alone", bytes(old_crc), none),
             ("version 12 with a non-zero word 7", with_header(c12, G.VERSION, f12, w12, plane), none),
             ("version 8 with a non-zero word 7", with_header(c17, U.VERSION, 1, elem, plane), none),
             ("version 12 with the volume flag", with_header(c17, G.VERSION, flags, word3, 0), none),
             ("version 18", with_header(c17, 18, flags, word3, plane), none)]
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    x = bytearray(c17)
    x[fr["start"] + 12:fr["start"] + 16] = struct.pack("<I", elem)
    cases.append(("a non-zero frame word", M.retable(bytes(x), fr["start"]), (M.FRAME_TABLE, multi, -1)))
    s, e, _ = fr["records"][1]
    flipped = bytearray(c17)
    flipped[(s + e) // 2] ^= 0x20
    cases.append(("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1)))
    cases += [("a legal but wrong plane: only crc_all sees it", hdr(w7=plane + 1), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong fold: only crc_all sees it", hdr(flags ^ G.FLAG_FOLD), (M.DECODED_CRC, -1, -1)),
              ("cut inside the last frame", c17[:lay["trailer"] - 8], (M.TRUNCATED, len(lay["frames"]) - 1, -1))]
    cases = [c + (READS,) for c in cases]
    cases += [("version 17 to a grid plan", c17, none, G.READS),
              ("version 17 to a lag plan", c17, none, L.READS),
              ("version 17 to an auto plan", c17, none, U.READS_AUTO),
              ("version 17 to a plain plan", c17, none, frozenset())]
    return cases, lay
