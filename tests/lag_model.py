"""Pure Python + numpy model of the lagged, folded delta of the container's typed-data filter (csrc/lag.hip) and of format version
11 (INTEGRATION.md 4b "Delta: lag and fold"), built from the parts of container_model, auto_model, sparse_model and ans_model.

  x[i]: element i of a segment as a little-endian unsigned integer of elem = 2, 4 or 8 bytes, W = 8 elem, RUN = 2048, r = i mod RUN,
  1 <= lag <= 16, fold 0 or 1:
    d[i] = x[i] where r < lag, else x[i] - x[i - lag] (mod 2^W)
    f[i] = d[i], or with the fold (d[i] << 1) ^ (0 - (d[i] >> (W - 1))) (mod 2^W), run heads included
    out[j q + i] = byte j of f[i], q = len // elem; the last len % elem bytes in place
  The inverse gathers f, d = (f >> 1) ^ (0 - (f & 1)), and x[i] = d[i] + d[i - lag] + ... down to the chain's member with r < lag.
  (lag, fold) = (1, 0) is container_model.delta_shuffle.

Version 11 is version 8's stream (auto_model: kinds 1, 2, 3, 5 per block from the auto rule, frame word 0) whose frames went through
this filter; the header's flags are 1 | fold << 1 | (lag - 1) << 8 with elem 2, 4 or 8, and (lag, fold) = (1, 0) is written as
version 8.  The reader of a plan with the setting on speaks versions 1 to 5, 7, 8 and 11."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import filter_auto_model as F
import sparse_model as S

VERSION = 11
RUN = M.RUN
MAX_LAG = 16
FLAG_FOLD, LAG_SHIFT = 2, 8
READS = frozenset(("sparse", "ans", "auto", "lag"))               # what a plan with the setting on speaks


# ----------------------------------------------------------------------------------------------------------------------
# the transform
# ----------------------------------------------------------------------------------------------------------------------
def _fold(d, w):
    return (d << d.dtype.type(1)) ^ (d.dtype.type(0) - (d >> d.dtype.type(w - 1)))


def _unfold(f):
    one = f.dtype.type(1)
    return (f >> one) ^ (f.dtype.type(0) - (f & one))


def _lag_delta(a, elem, lag, fold):
    m = a.size - a.size % elem
    x = a[:m].view("<u%d" % elem)
    d = x.copy()
    d[lag:] -= x[:-lag] if lag < x.size else x[:0]
    head = np.arange(x.size) % RUN < lag
    d[head] = x[head]
    if fold:
        d = _fold(d, 8 * elem)
    return np.concatenate([d.view(np.uint8), a[m:]])


def _sum_runs(d, lag):
    """x[i] = the sum of d over i's chain within its run of RUN elements"""
    x = np.empty_like(d)
    for r in range(0, d.size, RUN):
        run = d[r:r + RUN]
        for c in range(min(lag, run.size)):
            x[r + c:r + RUN:lag] = np.cumsum(run[c::lag], dtype=d.dtype)
    return x


def _unlag_delta(a, elem, lag, fold):
    m = a.size - a.size % elem
    f = a[:m].view("<u%d" % elem)
    x = _sum_runs(_unfold(f) if fold else f, lag)
    return np.concatenate([x.view(np.uint8), a[m:]])


def _check(elem, lag, fold):
    assert elem in M.ELEMS and 1 <= lag <= MAX_LAG and fold in (0, 1)


def lag_delta_shuffle(data, elem, lag, fold):
    _check(elem, lag, fold)
    return M.shuffle(_lag_delta(np.ascontiguousarray(M._u8(data).reshape(-1)), elem, lag, fold), elem)


def unlag_delta_unshuffle(data, elem, lag, fold):
    _check(elem, lag, fold)
    return _unlag_delta(np.ascontiguousarray(M.unshuffle(data, elem)), elem, lag, fold)


def unlag_delta_unshuffle_range(data, elem, lag, fold, first, count):
    """the bytes of elements [first, first + count) of unlag_delta_unshuffle(data, ...), from the plane runs alone; first % RUN == 0"""
    _check(elem, lag, fold)
    a = M._u8(data).reshape(-1)
    q = a.size // elem
    assert first % RUN == 0 and first + count <= q
    planes = np.stack([a[j * q + first: j * q + first + count] for j in range(elem)], axis=1)
    f = np.ascontiguousarray(planes).reshape(-1).view("<u%d" % elem)
    return _sum_runs(_unfold(f) if fold else f, lag).view(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# format version 11
# ----------------------------------------------------------------------------------------------------------------------
def flags_of(lag, fold):
    return M.FLAG_DELTA | fold << 1 | (lag - 1) << LAG_SHIFT


def flags_legal(flags):
    return bool(flags & 1) and not flags & ~0x0F03 and bool(flags & 0x0F02)


def format_legal(version, flags, elem):
    """the whole format rule, as the library's format_legal(): auto_model's table for the versions it knows (with runs_model's 6
    and dedup_model's 9, the same triples as version 5, and version 10's one), and version 11's family"""
    if version == VERSION:
        return flags_legal(flags) and elem in M.ELEMS
    if version == 10:
        return flags == 0 and elem == 0
    if version in (6, 9):
        version = 5
    return U.stream_format(version, flags, elem) is not None


def lag_fold_of(version, flags):
    return ((flags >> LAG_SHIFT & 15) + 1, flags >> 1 & 1) if version == VERSION else (1, 0)


def writer_version(lag, fold):
    """the lowest version that can say what the writer does"""
    return VERSION if (lag, fold) != (1, 0) else U.VERSION


def write(data, block_len, rows, elem, lag, fold, kinds=None):
    """The container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode, the shuffle at
    `elem`, the delta and the delta-lag setting (lag, fold) makes it: version 11, or version 8 byte for byte at (1, 0)."""
    _check(elem, lag, fold)
    if (lag, fold) == (1, 0):
        return U.write(data, block_len, rows, elem, True, kinds)
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION, flags_of(lag, fold), block_len, elem) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    nblk = 0
    frames = F.cut(a.size, block_len, rows)
    for pos, nb, bl in frames:
        f = lag_delta_shuffle(a[pos:pos + nb * bl], elem, lag, fold)
        per = ["rule"] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        nblk += nb
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, reads=READS):
    """decoded bytes of a container as the reader of a plan that speaks `reads` sees it, or ContainerError(what, frame, block).
    READS is a plan with the setting on (versions 1 to 5, 7, 8 and 11); without "lag" version 11 is a stream-header failure;
    with "filter" the reader is filter_auto_model's.  Lag and fold come from the stream header."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        rest = frozenset(reads) - {"lag"}
        return F.read(buf, reads=rest) if "filter" in rest else U.read(buf, reads=rest)
    h = buf[:32]
    magic, _, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or not format_legal(ver, flags, elem) or "lag" not in reads):
        raise M.ContainerError(M.STREAM_HEADER)
    lag, fold = lag_fold_of(ver, flags)
    L = len(buf)
    pos, done, fi = 32, 0, 0
    out = []
    while done < total:
        if pos + 32 + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        fmagic, nb, bl, word, P, _, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        if (fmagic != M.MAGIC_FRAME or word or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * M.raw_words(bl)):
            raise M.ContainerError(M.FRAME_TABLE, fi)
        fb = 32 + 4 * M.tables_layout(nb, bl)["words"] + 4 * M._pad2(P)
        if pos + fb + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        out.append(unlag_delta_unshuffle(F._frame_blocks(buf, pos, nb, bl, P, fi), elem, lag, fold))     # (version 8's frame)
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
    return data


def kinds_of(buf):
    """the record kind of every block of a valid container, in order"""
    return [k for fr in M.layout(buf)["frames"] for _, _, k in fr["records"]]


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 11, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c11):
    """[(name, container, (what, frame, block), reads)] from the valid version-11 container c11: what the reader of a plan that
    speaks `reads` answers.  c11 needs a frame of two or more blocks."""
    lay = M.layout(c11)
    _, flags, _, elem = struct.unpack("<HHII", c11[4:16])
    lag, fold = lag_fold_of(VERSION, flags)
    none = (M.STREAM_HEADER, -1, -1)
    hdr = lambda fl, e=elem: M.with_header(c11, VERSION, fl, e)
    cases = [("flags with bit 0 clear", hdr(flags & ~1), none),
             ("flags with bit 2 set", hdr(flags | 4), none),
             ("flags with bit 7 set", hdr(flags | 0x80), none),
             ("flags with bit 12 set", hdr(flags | 0x1000), none),
             ("flags with bit 15 set", hdr(flags | 0x8000), none),
             ("the lag field set under elem 0", hdr(flags_of(3, 0), 0), none),
             ("the fold under elem 0", hdr(flags_of(1, 1), 0), none),
             ("elem 3", hdr(flags, 3), none), ("elem 16", hdr(flags, 16), none),
             ("(11, flags 1): what version 8 says", hdr(1), none),
             ("(11, flags 0)", hdr(0), none),
             ("version 12", M.with_header(c11, 12, flags, elem), none),
             ("version 8 with these flags", M.with_header(c11, U.VERSION, flags, elem), none),
             ("version 10 with these flags", M.with_header(c11, 10, flags, elem), none)]
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    T = M.tables_layout(fr["nb"], fr["blk_len"])

    def poke(kind, b):
        x = bytearray(c11)
        off = fr["tables"][0] + 4 * (T["kind"] + b)
        x[off:off + 4] = struct.pack("<I", kind)
        return M.retable(bytes(x), fr["start"])

    cases += [("kind 4 under version 11", poke(4, 1), (M.FRAME_TABLE, multi, 1)), ("kind 6 under version 11", poke(6, 0), (M.FRAME_TABLE, multi, 0))]
    x = bytearray(c11)
    x[fr["start"] + 12:fr["start"] + 16] = struct.pack("<I", elem)
    cases.append(("a non-zero frame word", M.retable(bytes(x), fr["start"]), (M.FRAME_TABLE, multi, -1)))
    s, e, _ = fr["records"][1]
    flipped = bytearray(c11)
    flipped[(s + e) // 2] ^= 0x20
    cases.append(("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1)))
    other = lag + 1 if lag < MAX_LAG else lag - 1
    cases += [("a legal but wrong lag: only crc_all sees it", hdr(flags_of(other, fold)), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong fold: only crc_all sees it", hdr(flags_of(lag if lag > 1 or not fold else 2, fold ^ 1)), (M.DECODED_CRC, -1, -1))]
    cases.append(("cut inside the last frame", c11[:lay["trailer"] - 8], (M.TRUNCATED, len(lay["frames"]) - 1, -1)))
    cases = [c + (READS,) for c in cases]
    cases += [("version 11 to a plan without the setting: the auto mode's", c11, none, U.READS_AUTO),
              ("version 11 to a filter-auto plan", c11, none, F.READS),
              ("version 11 to a plan with no mode on", c11, none, frozenset())]
    return cases, lay
