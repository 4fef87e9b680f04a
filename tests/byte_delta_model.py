"""Pure Python + numpy model of the container's byte predictor for 8-bit sample data (csrc/byte_delta.hip) and of format version 15
(INTEGRATION.md 4b "Delta: bytes"), built from the parts of auto_model, filter_auto_model and container_model.

  x: the bytes of a segment of any length, arithmetic modulo 256, RUN = 2048, 1 <= lag <= 16 (the channel count), stride 0 (none)
  or 2 <= stride <= 65536 (the row length in bytes, channels * width), P = 2048 ceil(stride / 64) the period (grid_model's):
    v[i] = x[i] where stride == 0 or i mod P < stride, else x[i] - x[i - stride]
    d[i] = v[i] where i mod RUN < lag, else v[i] - v[i - lag]
    out[i] = d[i]: same length, same positions; no planes, no tail, no fold
  The inverse sums d down every chain (i, i - lag, ...) of a run, which gives v, and then x[i] = v[i] + x[i - stride] for
  i mod P >= stride up every band.  Runs nest in bands, so the range form takes a `first` that is a multiple of RUN at stride 0 and
  of P otherwise.

Version 15 is version 8's stream (auto_model: kinds 1, 2, 3, 5 per block from the auto rule, frame word 0) whose frames went through
this transform as one segment each; the header's flags are 1 | (stride ? 4 : 0) | (lag - 1) << 8 and its word 3 is 1 | stride << 8.
The reader of a plan with the setting on speaks versions 1 to 5, 7, 8 and 15."""
import struct
import zlib

import numpy as np

import ans_model as A
import auto_model as U
import container_model as M
import filter_auto_model as F

VERSION = 15
RUN = M.RUN
MAX_LAG = 16
MIN_STRIDE, MAX_STRIDE = 2, 65536
FLAG_STRIDE, LAG_SHIFT = 4, 8
READS = frozenset(("sparse", "ans", "auto", "byte"))              # what a plan with the setting on speaks


def period(stride):
    return RUN * ((stride + 63) // 64)


def step(stride):
    """what a range read starts at a multiple of: the run, with a stride the band"""
    return period(stride) if stride else RUN


# ----------------------------------------------------------------------------------------------------------------------
# the transform
# ----------------------------------------------------------------------------------------------------------------------
def _check(lag, stride):
    assert 1 <= lag <= MAX_LAG and (stride == 0 or MIN_STRIDE <= stride <= MAX_STRIDE)


def _bytes(data):
    return np.ascontiguousarray(M._u8(data).reshape(-1))


def _back(x, dist, keep):
    """x with x[i - dist] subtracted wherever keep[i]"""
    v = x.copy()
    i = np.flatnonzero(keep)
    v[i] = x[i] - x[i - dist]
    return v


def _sum_runs(d, lag):
    """v[i] = the sum of d over i's chain within its run of RUN bytes"""
    v = np.empty_like(d)
    for r in range(0, d.size, RUN):
        run = d[r:r + RUN]
        for c in range(min(lag, run.size)):
            v[r + c:r + RUN:lag] = np.cumsum(run[c::lag], dtype=np.uint8)
    return v


def _vsum(v, stride):
    """x of v, band by band: the running sum down every column of a band's rows"""
    if not stride:
        return v
    P = period(stride)
    x = np.empty_like(v)
    for b in range(0, v.size, P):
        band = v[b:b + P]
        rows = -(-band.size // stride)
        pad = np.zeros(rows * stride, np.uint8)
        pad[:band.size] = band
        x[b:b + P] = np.cumsum(pad.reshape(rows, stride), axis=0, dtype=np.uint8).reshape(-1)[:band.size]
    return x


def byte_delta(data, lag, stride):
    _check(lag, stride)
    x = _bytes(data)
    i = np.arange(x.size)
    v = _back(x, stride, i % period(stride) >= stride) if stride else x
    return _back(v, lag, i % RUN >= lag)


def unbyte_delta(data, lag, stride):
    _check(lag, stride)
    return _vsum(_sum_runs(_bytes(data), lag), stride)


def unbyte_delta_range(data, lag, stride, first, count):
    """bytes [first, first + count) of unbyte_delta(data, ...), from those bytes of data alone; first % step(stride) == 0"""
    _check(lag, stride)
    d = _bytes(data)
    assert first % step(stride) == 0 and first + count <= d.size
    return _vsum(_sum_runs(d[first:first + count], lag), stride)


# ----------------------------------------------------------------------------------------------------------------------
# format version 15
# ----------------------------------------------------------------------------------------------------------------------
def flags_of(lag, stride):
    return M.FLAG_DELTA | (FLAG_STRIDE if stride else 0) | (lag - 1) << LAG_SHIFT


def word3_of(stride):
    return 1 | stride << 8


def format_legal(flags, word3):
    """version 15's family over the header's flags and word 3"""
    stride = word3 >> 8
    return ((word3 & 255) == 1 and (stride == 0 or MIN_STRIDE <= stride <= MAX_STRIDE) and bool(flags & 1) and not flags & ~0x0F05
            and bool(flags & FLAG_STRIDE) == (stride != 0))


def lag_stride_of(flags, word3):
    return (flags >> LAG_SHIFT & 15) + 1, word3 >> 8


def write(data, block_len, rows, lag, stride, kinds=None):
    """The container of `data` as a writer plan of n = block_len, `rows` rows, the order-0 codec, the auto mode and the byte-delta
    setting (lag, stride) makes it: version 15; lag 0 is the setting off, the auto mode's version 8."""
    a = M._u8(data).reshape(-1)
    if lag == 0:
        return U.write(a, block_len, rows, 0, False, kinds)
    _check(lag, stride)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSION, flags_of(lag, stride), block_len, word3_of(stride)) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    nblk = 0
    frames = F.cut(a.size, block_len, rows)
    for pos, nb, bl in frames:
        f = byte_delta(a[pos:pos + nb * bl], lag, stride)
        per = ["rule"] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        nblk += nb
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, reads=READS):
    """decoded bytes of a container as the reader of a plan that speaks `reads` sees it, or ContainerError(what, frame, block).
    READS is a plan with the setting on (versions 1 to 5, 7, 8 and 15); without "byte" version 15 is a stream-header failure; every
    other version is auto_model's reader's.  Lag and stride come from the stream header."""
    buf = bytes(buf)
    if len(buf) < 48:
        raise M.ContainerError(M.TRUNCATED)
    ver = struct.unpack("<H", buf[4:6])[0]
    if ver != VERSION:
        return U.read(buf, reads=frozenset(reads) - {"byte"})
    h = buf[:32]
    magic, _, flags, block_len, word3, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or not format_legal(flags, word3) or "byte" not in reads):
        raise M.ContainerError(M.STREAM_HEADER)
    lag, stride = lag_stride_of(flags, word3)
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
        out.append(unbyte_delta(F._frame_blocks(buf, pos, nb, bl, P, fi), lag, stride))     # (version 8's frame)
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


def range_first(a, stride):
    """the frame byte a range read that needs frame byte a starts its inverse at: the start of a's run or band"""
    return a - a % step(stride)


def range_blocks(a, b, stride, nb, bl):
    """the blocks of a frame of nb blocks of bl bytes a range read of its bytes [a, b) decodes (a < b)"""
    return list(range(range_first(a, stride) // bl, min(nb - 1, (b - 1) // bl) + 1))


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 15, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c15):
    """[(name, container, (what, frame, block), reads)] from the valid version-15 container c15: what the reader of a plan that
    speaks `reads` answers.  c15 needs a frame of two or more blocks."""
    lay = M.layout(c15)
    _, flags, _, word3 = struct.unpack("<HHII", c15[4:16])
    lag, stride = lag_stride_of(flags, word3)
    none = (M.STREAM_HEADER, -1, -1)
    hdr = lambda fl, w3=word3: M.with_header(c15, VERSION, fl, w3)
    cases = [("flags with bit 0 clear", hdr(flags & ~1), none),
             ("the fold bit", hdr(flags | 2), none),
             ("flags with bit 3", hdr(flags | 8), none),
             ("flags with bit 7", hdr(flags | 0x80), none),
             ("flags with bit 12", hdr(flags | 0x1000), none),
             ("flags with bit 15", hdr(flags | 0x8000), none),
             ("bit 2 against the stride", hdr(flags ^ FLAG_STRIDE), none),
             ("stride 1", hdr(flags | FLAG_STRIDE, word3_of(1)), none),
             ("stride 65537", hdr(flags | FLAG_STRIDE, word3_of(65537)), none),
             ("elem 0", hdr(flags, word3 & ~255), none),
             ("elem 2", hdr(flags, word3 & ~255 | 2), none),
             ("(15, 0, 0)", hdr(0, 0), none),
             ("version 8 with these words", M.with_header(c15, U.VERSION, flags, word3), none),
             ("version 12 with these words", M.with_header(c15, 12, flags, word3), none),
             ("version 16", M.with_header(c15, 16, flags, word3), none)]
    multi = next(i for i, f in enumerate(lay["frames"]) if f["nb"] >= 2)
    fr = lay["frames"][multi]
    T = M.tables_layout(fr["nb"], fr["blk_len"])

    def poke(kind, b):
        x = bytearray(c15)
        off = fr["tables"][0] + 4 * (T["kind"] + b)
        x[off:off + 4] = struct.pack("<I", kind)
        return M.retable(bytes(x), fr["start"])

    cases += [("kind 4 under version 15", poke(4, 1), (M.FRAME_TABLE, multi, 1)), ("kind 6 under version 15", poke(6, 0), (M.FRAME_TABLE, multi, 0))]
    x = bytearray(c15)
    x[fr["start"] + 12:fr["start"] + 16] = struct.pack("<I", 1)
    cases.append(("a non-zero frame word", M.retable(bytes(x), fr["start"]), (M.FRAME_TABLE, multi, -1)))
    s, e, _ = fr["records"][1]
    flipped = bytearray(c15)
    flipped[(s + e) // 2] ^= 0x20
    cases.append(("a flipped record bit", bytes(flipped), (M.RECORD_CRC, multi, 1)))
    other_lag = lag + 1 if lag < MAX_LAG else lag - 1
    other_stride = 600 if stride != 600 else 601
    cases += [("a legal but wrong lag: only crc_all sees it", hdr(flags_of(other_lag, stride)), (M.DECODED_CRC, -1, -1)),
              ("a legal but wrong stride: only crc_all sees it", hdr(flags_of(lag, other_stride), word3_of(other_stride)), (M.DECODED_CRC, -1, -1)),
              ("cut inside the last frame", c15[:lay["trailer"] - 8], (M.TRUNCATED, len(lay["frames"]) - 1, -1))]
    cases = [c + (READS,) for c in cases]
    cases += [("version 15 to an auto plan", c15, none, U.READS_AUTO),
              ("version 15 to a lag plan", c15, none, frozenset(("sparse", "ans", "auto", "lag"))),
              ("version 15 to a grid plan", c15, none, frozenset(("sparse", "ans", "auto", "grid"))),
              ("version 15 to a filter-auto plan", c15, none, F.READS),
              ("version 15 to a plain plan", c15, none, frozenset())]
    return cases, lay
