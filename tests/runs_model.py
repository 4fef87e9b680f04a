"""Pure Python + numpy model of the zero-run split, of the zero-run BWT record (kind 4) and of format version 6 of the BWT
container, built from container_model's parts (its CRCs, tables_layout, h0_encode / h0_decode / h0_words,
filter_frame, ContainerError) and oracle_lib's bwt / mtf / ibwt / imtf.

The split, T = 256.  For a segment x[0, n): position i is a RUN START when x[i] = 0 and (i % 256 = 0 or x[i - 1] != 0).  A is the
subsequence of x at the positions that are non-zero or run starts, in order: each run contributes one 0.  B has one byte per run
start, in order: r - 1, where r counts the zero positions from i up to, but not including, the next position that is non-zero,
a multiple of 256, or n.  So 1 <= r <= 256 and no run crosses a tile.  nB = the zeros of A; nA <= n, nB <= n;
(nA - nB) + sum(B[j] + 1) = n.  The join walks A: a non-zero byte is copied, the z-th zero becomes B[z] + 1 zeros.  It is
tolerant: it does not ask for the tile rule, a zero beyond B's end is one zero, output beyond n is dropped, a short output ends
in zeros.

A kind-4 block stores bwt_index as kind 0 does, hist[256] = the byte counts of A (so nA = sum hist, nB = hist[0]) and enc_off
zeros.  Its record: u32 nz; nz words (v << 24) | count, v strictly ascending, count >= 1, the non-zero counts of B; the kind-2
stream of A with the table of hist; when nB > 0 the kind-2 stream of B with the table of B's counts.  The writer's rule: kind 4
unless 4 * words >= blk_len, then raw.  A version-6 frame may hold kinds 0, 1, 2 and 4, not 3.

The reader with the mode on reads versions 1 to 4 and 6; with it off it is sparse_model's reader, to which version 6 is a
stream-header failure.  No single reader takes both 5 and 6."""
import struct
import zlib

import numpy as np

import container_model as M
import sparse_model as S

TILE = 256
RUNS = 4
VERSION = 6
FORMATS = dict(M.FORMATS)
FORMATS.update({(VERSION, 0): ((0,) + M.ELEMS, RUNS), (VERSION, M.FLAG_DELTA): (M.ELEMS, RUNS)})
O = M.O


def stream_format(version, flags, elem):
    elems, max_kind = FORMATS.get((version, flags), ((), M.RAW))
    return M.Format(version, flags, elem, flags == M.FLAG_DELTA, max_kind) if elem in elems else None


def kind_legal(fmt, kind):
    return kind <= fmt.max_kind and not (fmt.version == VERSION and kind == S.SPARSE)


# ----------------------------------------------------------------------------------------------------------------------
# split and join
# ----------------------------------------------------------------------------------------------------------------------
def split(x):
    """(A, B) of one segment"""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    n = x.size
    z = x == 0
    pos = np.arange(n)
    prev_zero = np.concatenate([[False], z[:-1]])
    start = z & ((pos % TILE == 0) | ~prev_zero)
    A = x[~z | start]
    # a run ends in front of the next position that is non-zero or a multiple of TILE, or at n
    stop = ~z | (pos % TILE == 0)
    nxt = np.full(n + 1, n, dtype=np.int64)                   # nxt[i] = the first stop at or behind i
    idx = np.where(stop, pos, n)
    nxt[:n] = np.minimum.accumulate(idx[::-1])[::-1]
    s = pos[start]
    r = nxt[s + 1] - s
    assert r.size == 0 or (r.min() >= 1 and r.max() <= TILE)
    return A, (r - 1).astype(np.uint8)


def join(A, B, n):
    """the segment of n bytes A and B stand for; defined for any A, B and n"""
    A = np.asarray(A, np.uint8).reshape(-1)
    B = np.asarray(B, np.uint8).reshape(-1)
    z = A == 0
    zr = np.cumsum(z) - z                                      # rank of every zero among the zeros
    ln = np.ones(A.size, dtype=np.int64)
    have = z & (zr < B.size)
    ln[have] = B[zr[have]].astype(np.int64) + 1
    pos = np.cumsum(ln) - ln
    out = np.zeros(n, np.uint8)
    w = ~z & (pos < n)
    out[pos[w]] = A[w]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the record
# ----------------------------------------------------------------------------------------------------------------------
def pairs_of(histB):
    v = np.nonzero(histB)[0]
    return ((v.astype(np.uint32) << 24) | np.asarray(histB, np.uint32)[v]).astype(np.uint32)


def runs_words(hist, histB):
    """words of the record of a block with these counts of A and of B"""
    nB = int(np.asarray(histB, np.uint64).sum())
    return 1 + int(np.count_nonzero(histB)) + M.h0_words(hist) + (M.h0_words(histB) if nB else 0)


def encode_block4(blk):
    """(kind, bwt_index, hist of A, enc_off, record words) of one block as a zero-run record, raw when 4 * words >= blk_len"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    nsub = (blk.size + M.HUFF_BLOCK - 1) // M.HUFF_BLOCK
    L, idx = O.bwt(blk)
    A, B = split(O.mtf(L))
    hist, sa = M.h0_encode(A)
    histB = np.bincount(B, minlength=256).astype(np.uint32)
    pr = pairs_of(histB)
    parts = [np.array([pr.size], np.uint32), pr, sa]
    if B.size:
        parts.append(M.h0_encode(B)[1])
    words = np.concatenate(parts).astype(np.uint32)
    assert words.size == runs_words(hist, histB)
    if 4 * words.size >= blk.size:
        return M.encode_block(blk, M.RAW)
    return RUNS, idx, hist, np.zeros(nsub, np.uint32), words


def encode_block(blk, codec):
    """codec 0, 1, 2: container_model's; 4: a zero-run record under its raw rule"""
    return encode_block4(blk) if codec == RUNS else M.encode_block(blk, codec)


def check_runs_fields(idx, eo, hist, pay, lo, hi, bl):
    """the field checks of a kind-4 block in the specified order; True = refused.  nz is read only once the record is known to
    hold it, the pairs only once it is known to hold them."""
    hist = np.asarray(hist, np.uint64)
    if idx >= bl or bool(np.asarray(eo).any()) or int(hist.sum()) < 1:
        return True
    if hi - lo < 1:
        return True
    nz = int(pay[lo])
    if nz > 256 or hi - lo < 1 + nz:
        return True
    pr = pay[lo + 1:lo + 1 + nz].astype(np.int64)
    v, c = pr >> 24, pr & 0xFFFFFF
    if bool((c < 1).any()) or bool((v[1:] <= v[:-1]).any()):
        return True
    if int(c.sum()) != int(hist[0]):
        return True
    if int(hist.sum()) - int(hist[0]) + int((c * (v + 1)).sum()) != bl:
        return True
    histB = np.zeros(256, np.uint32)
    histB[v] = c
    return hi - lo != 1 + nz + M.h0_words(hist.astype(np.uint32)) + (M.h0_words(histB) if int(c.sum()) else 0)


def decode_block4(idx, hist, rec, bl):
    nz = int(rec[0])
    pr = rec[1:1 + nz].astype(np.int64)
    histB = np.zeros(256, np.uint32)
    histB[pr >> 24] = pr & 0xFFFFFF
    nA, nB = int(np.asarray(hist, np.uint64).sum()), int(histB.sum())
    wa = M.h0_words(hist)
    A = M.h0_decode(hist, rec[1 + nz:1 + nz + wa], nA)[0]
    B = M.h0_decode(histB, rec[1 + nz + wa:], nB)[0] if nB else np.zeros(0, np.uint8)
    return O.ibwt(O.imtf(join(A, B, bl)), idx)


# ----------------------------------------------------------------------------------------------------------------------
# writer and reader
# ----------------------------------------------------------------------------------------------------------------------
def _frame(blocks, blk_len, kinds):
    nb = len(blocks)
    T = M.tables_layout(nb, blk_len)
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
    hdr24 = M.MAGIC_FRAME + struct.pack("<III", nb, blk_len, 0) + struct.pack("<Q", P)
    tables = W.tobytes()
    payload = b"".join(w.tobytes() for w in recs) + (b"\0\0\0\0" if P & 1 else b"")
    return hdr24 + struct.pack("<II", zlib.crc32(hdr24 + tables), 0) + tables + payload


def write(data, block_len, rows, elem=0, delta=False, kinds=None):
    """The version-6 container of `data` as a writer plan of n = block_len, `rows` rows, filter element size `elem`, delta mode
    `delta`, the BWT codec and the runs mode on makes it: every block kind 4 under its raw rule.  `kinds` (cycled over the
    stream's blocks; each 0, 1, 2 or 4) forces the codec of each block instead, every one still under its raw rule."""
    elem = 0 if elem == 1 else elem
    fmt = stream_format(VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert fmt is not None
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= 1 << 20 and rows >= 1
    n = a.size
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", fmt.version, fmt.flags, block_len, fmt.elem) + struct.pack("<Q", n)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    pos, frames, nblk = 0, 0, 0
    while pos < n:
        left = n - pos
        nb, bl = (min(rows, left // block_len), block_len) if left >= block_len else (1, left)
        f = M.filter_frame(a[pos:pos + nb * bl], fmt)
        per = [RUNS] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(_frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        pos += nb * bl
        nblk += nb
        frames += 1
    t12 = M.MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def read(buf, with_kinds=False, max_version=VERSION, runs=True):
    """decoded bytes of a container, or ContainerError(what, frame, block).  runs = the reader's runs mode: on, versions 1 to 4
    and 6 up to max_version; off, sparse_model's reader of versions up to min(max_version, 5)."""
    if not runs:
        return S.read(buf, with_kinds, max_version=min(max_version, S.VERSION))
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise M.ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    fmt = stream_format(ver, flags, elem)
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or fmt is None or ver > max_version):
        raise M.ContainerError(M.STREAM_HEADER)
    pos, done, fi = 32, 0, 0
    out, kinds = [], []
    while done < total:
        if pos + 32 + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        fmagic, nb, bl, fz, P, tcrc, fz2 = struct.unpack("<4sIIIQII", buf[pos:pos + 32])
        if (fmagic != M.MAGIC_FRAME or fz or fz2 or nb == 0 or bl == 0 or bl > block_len or (nb > 1 and bl != block_len)
                or nb * bl > total - done or P > nb * M.raw_words(bl)):
            raise M.ContainerError(M.FRAME_TABLE, fi)
        T = M.tables_layout(nb, bl)
        fb = 32 + 4 * T["words"] + 4 * M._pad2(P)
        if pos + fb + 16 > L:
            raise M.ContainerError(M.TRUNCATED, fi)
        tb = buf[pos + 32: pos + 32 + 4 * T["words"]]
        if zlib.crc32(buf[pos:pos + 24] + tb) != tcrc:
            raise M.ContainerError(M.FRAME_TABLE, fi)
        W = np.frombuffer(tb, dtype=np.uint32)
        po = W[T["pay_off"]:T["pay_off"] + 2 * (nb + 1)].view(np.uint64).astype(np.int64)
        pay = np.frombuffer(buf[pos + 32 + 4 * T["words"]: pos + 32 + 4 * T["words"] + 4 * P], dtype=np.uint32)
        nsub = T["nsub"]
        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            idx = int(W[T["bwt"] + b])
            wrong = not kind_legal(fmt, kind) or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == RUNS:
                wrong = check_runs_fields(idx, eo, hist, pay, lo, hi, bl)
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
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            if kind == M.RAW:
                blk = pay[lo:hi].view(np.uint8)[:bl]
            elif kind == RUNS:
                blk = decode_block4(int(W[T["bwt"] + b]), hist, pay[lo:hi], bl)
            elif kind == M.HUFF0:
                blk, used = M.h0_decode(hist, pay[lo:hi], bl)
                assert (used + 31) // 32 + 1 == hi - lo
            else:
                blk = O.decompress(int(W[T["bwt"] + b]), hist, W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            if zlib.crc32(blk.tobytes()) != int(W[T["crc_raw"] + b]):
                raise M.ContainerError(M.DECODED_CRC, fi, b)
            blocks.append(blk)
            kinds.append(kind)
        out.append(M.unfilter_frame(np.concatenate(blocks), fmt))
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
    return (data, kinds) if with_kinds else data


def payload_ratio(data, block_len, kind):
    """input bytes / record bytes over the blocks of `data`, raw rule applied: kind 0 (today's BWT record) or 4"""
    a = M._u8(data).reshape(-1)
    words = 0
    for p in range(0, a.size, block_len):
        words += encode_block(a[p:p + block_len], kind)[4].size
    return a.size / (4.0 * words)


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 6, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c6, elem):
    """[(name, container, (what, frame, block))] from the valid version-6 container c6 (header flags as written): every field
    check of a kind-4 record violated alone, the table CRC recomputed.  It needs, in a frame other than the first, a kind-4 block
    with nz >= 2 that is not the last of its frame."""
    lay = M.layout(c6)
    flags = struct.unpack("<H", c6[6:8])[0]
    for fi, fr in enumerate(lay["frames"]):
        hit = [(b, s, e) for b, (s, e, kind) in enumerate(fr["records"])
               if fi > 0 and kind == RUNS and b + 1 < fr["nb"] and struct.unpack("<I", c6[s:s + 4])[0] >= 2]
        if hit:
            b, s, e = hit[0]
            break
    else:
        raise AssertionError("the container lacks the block the refusal cases need")
    T = M.tables_layout(fr["nb"], fr["blk_len"])
    t0, bl = fr["tables"][0], fr["blk_len"]
    nz = struct.unpack("<I", c6[s:s + 4])[0]
    pairs = list(struct.unpack("<%dI" % nz, c6[s + 4:s + 4 + 4 * nz]))

    def tables(x):
        return np.frombuffer(bytes(x[t0:t0 + 4 * T["words"]]), np.uint32).copy()

    def edit(table_words=(), record_words=(), resize=0, recrc=True):
        """table words {offset: value}, record words {index: value}, the record made `resize` words longer"""
        x = bytearray(c6)
        W = tables(x)
        for off, val in dict(table_words).items():
            W[off] = val
        if resize:
            po = W[T["pay_off"]:T["pay_off"] + 2 * (fr["nb"] + 1)].view(np.uint64)
            po[b + 1] = np.uint64(int(po[b + 1]) + resize)
        for i, val in dict(record_words).items():
            x[s + 4 * i:s + 4 * i + 4] = struct.pack("<I", val)
        x[t0:t0 + 4 * T["words"]] = W.tobytes()
        if recrc:                                             # (the record's own CRC too: only the field check is to see the edit)
            W = tables(x)
            po = W[T["pay_off"]:T["pay_off"] + 2 * (fr["nb"] + 1)].view(np.uint64)
            ps = fr["payload"]
            W[T["crc_rec"] + b] = zlib.crc32(bytes(x[ps + 4 * int(po[b]):ps + 4 * int(po[b + 1])]))
            x[t0:t0 + 4 * T["words"]] = W.tobytes()
            return M.retable(bytes(x), fr["start"])
        return bytes(x)

    W0 = tables(c6)
    h = T["hist"] + 256 * b
    hist = W0[h:h + 256].astype(np.int64)
    other = int(np.nonzero(hist[1:])[0][0]) + 1               # a non-zero byte A holds
    rec_words = (e - s) // 4
    flipped = bytearray(c6)
    flipped[e - 6] ^= 0x20
    at = (M.FRAME_TABLE, fi, b)
    cases = [
        ("1: bwt_index = blk_len", edit({T["bwt"] + b: bl}), at),
        ("2: enc_off set", edit({T["enc_off"] + T["nsub"] * b: 1}), at),
        ("3: the counts of an empty A", edit({h + k: 0 for k in range(256)}), at),
        ("4: an empty record", edit(resize=-rec_words), at),
        ("4: nz = 257", edit(record_words={0: 257}), at),
        ("5: a record shorter than its pairs", edit(resize=-(rec_words - nz)), at),
        ("6: pairs out of order", edit(record_words={1: pairs[1], 2: pairs[0]}), at),
        ("6: a pair with count 0", edit(record_words={1: pairs[0] & 0xFF000000}), at),
        ("7: counts that do not sum to hist[0]", edit({h: int(hist[0]) + 1}), at),
        ("8: runs that do not fill the block", edit({h + other: int(hist[other]) + 1}), at),
        ("9: one word too many", edit(resize=1), at),
        ("9: one word too few", edit(resize=-1), at),
        ("the table CRC sees it first", edit({T["bwt"] + b: bl}, recrc=False), (M.FRAME_TABLE, fi, -1)),
        ("a flipped stream bit", bytes(flipped), (M.RECORD_CRC, fi, b)),
        ("kind 3 under version 6", edit({T["kind"] + b: S.SPARSE}), at),
        ("kind 5", edit({T["kind"] + b: 5}), at),
        ("version 6 with flags 2", M.with_header(c6, VERSION, 2, elem), (M.STREAM_HEADER, -1, -1)),
        ("version 7", M.with_header(c6, 7, flags, elem), (M.STREAM_HEADER, -1, -1)),
        ("cut inside the record", c6[:s + 2], (M.TRUNCATED, fi, -1)),
    ]
    first4 = [(f_i, b_i) for f_i, f in enumerate(lay["frames"]) for b_i, r in enumerate(f["records"]) if r[2] == RUNS][0]
    cases.append(("kind 4 under a version-4 header", M.with_header(c6, 4, flags, elem) if flags else M.with_header(c6, 3, 0, elem),
                  (M.FRAME_TABLE, first4[0], first4[1])))
    if flags == 0 and elem == 0:
        cases.append(("version 6, flags 1, elem 0", M.with_header(c6, VERSION, 1, 0), (M.STREAM_HEADER, -1, -1)))
    return cases, lay
