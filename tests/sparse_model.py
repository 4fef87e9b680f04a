"""Pure Python + numpy model of the sparse order-0 record (kind 3) and of format version 5 of the BWT container (INTEGRATION.md
4b), built from container_model's parts: its CRCs, tables_layout, h0_encode / h0_decode / h0_words, filter_frame, ContainerError.

A block of bl bytes is cut into chunks of 64 bytes (the last may be short).  A kind-3 record is a mask of ceil(nch / 32) words --
bit c % 32 of word c // 32, from the LSB, is 1 where chunk c is KEPT and 0 where every byte of it equals the block's fill byte
(stored in the bwt_index field) -- followed, when any chunk is kept, by the kind-2 stream of K, the kept chunks concatenated;
hist[] counts the bytes of K.  The writer's rule: fill = the most frequent byte (lowest on a tie), every all-fill chunk is elided,
the block is kind 3 when 32 * elided >= nch and kind 2 otherwise, and the raw rule (4 * words >= bl -> kind 1) applies to
whichever was chosen.  The reader takes any fill and any mask that pass the field checks.

The version-5 frame walk repeats container_model.read's; this file's reader takes every version up to max_version."""
import struct
import zlib

import numpy as np

import container_model as M

CHUNK = 64
SPARSE = 3
VERSION = 5
FORMATS = dict(M.FORMATS)
FORMATS.update({(VERSION, 0): ((0,) + M.ELEMS, SPARSE), (VERSION, M.FLAG_DELTA): (M.ELEMS, SPARSE)})


def stream_format(version, flags, elem):
    elems, max_kind = FORMATS.get((version, flags), ((), M.RAW))
    return M.Format(version, flags, elem, flags == M.FLAG_DELTA, max_kind) if elem in elems else None


def nchunks(bl):
    return (bl + CHUNK - 1) // CHUNK


def mask_words(bl):
    return (nchunks(bl) + 31) // 32


def fill_of(blk):
    """the most frequent byte, the lowest value on a tie"""
    return int(np.argmax(np.bincount(np.asarray(blk, np.uint8), minlength=256)))


def klen_of(mask, bl):
    """bytes of K for this mask (its unused bits zero) over a block of bl bytes"""
    nch = nchunks(bl)
    kept = sum(bin(int(w)).count("1") for w in mask)
    last = nch and (int(mask[(nch - 1) // 32]) >> ((nch - 1) % 32)) & 1
    return CHUNK * kept - (CHUNK * nch - bl if last else 0)


def split(blk, fill=None):
    """(fill, mask words u32, K) of one block: every chunk whose bytes all equal fill is elided"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8).reshape(-1)
    if fill is None:
        fill = fill_of(blk)
    bl, nch = blk.size, nchunks(blk.size)
    padded = np.full(nch * CHUNK, fill, np.uint8)
    padded[:bl] = blk
    kept = (padded.reshape(nch, CHUNK) != fill).any(axis=1)
    bits = np.zeros(32 * mask_words(bl), np.uint8)
    bits[:nch] = kept
    mask = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)
    idx = np.arange(nch * CHUNK).reshape(nch, CHUNK)[kept].reshape(-1)
    return fill, mask, blk[idx[idx < bl]]


def join(fill, mask, K, bl):
    """the block of bl bytes a fill byte, a mask and the kept bytes stand for"""
    nch = nchunks(bl)
    bits = np.unpackbits(np.asarray(mask, np.uint32).astype("<u4").view(np.uint8), bitorder="little")[:nch].astype(bool)
    out = np.full(nch * CHUNK, fill, np.uint8)
    idx = np.arange(nch * CHUNK).reshape(nch, CHUNK)[bits].reshape(-1)
    idx = idx[idx < bl]
    assert idx.size == len(K)
    out[idx] = K
    return out[:bl]


def _raw(blk):
    return M.encode_block(blk, M.RAW)


def encode_block3(blk, fill=None):
    """(kind, fill, hist of K, enc_off, record words) of one block as a sparse record, raw when 4 * words >= blk_len"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    nsub = (blk.size + M.HUFF_BLOCK - 1) // M.HUFF_BLOCK
    fill, mask, K = split(blk, fill)
    if K.size:
        hist, stream = M.h0_encode(K)
        words = np.concatenate([mask, stream])
    else:
        hist, words = np.zeros(256, np.uint32), mask
    if 4 * words.size >= blk.size:
        return _raw(blk)
    return SPARSE, fill, hist, np.zeros(nsub, np.uint32), words


def elided(blk):
    fill, mask, _ = split(blk)
    return nchunks(len(blk)) - sum(bin(int(w)).count("1") for w in mask)


def encode_block(blk, codec):
    """codec 0, 1, 2: container_model's; 3: a sparse record whatever the rule says; "rule": what the sparse writer makes --
    kind 3 when 32 * elided >= nch, else kind 2, each under its raw rule"""
    if codec == "rule":
        codec = SPARSE if 32 * elided(blk) >= nchunks(len(blk)) else M.HUFF0
    return encode_block3(blk) if codec == SPARSE else M.encode_block(blk, codec)


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
    """The version-5 container of `data` as a writer plan of n = block_len, `rows` rows, filter element size `elem`, delta mode
    `delta`, the order-0 codec and the sparse mode on makes it.  `kinds` (cycled over the stream's blocks; each 0, 1, 2 or 3)
    forces the codec of each block instead, every one still under its raw rule."""
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
        per = ["rule"] * nb if kinds is None else [kinds[(nblk + i) % len(kinds)] for i in range(nb)]
        out.append(_frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, per))
        pos += nb * bl
        nblk += nb
        frames += 1
    t12 = M.MAGIC_END + struct.pack("<II", frames, zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    return b"".join(out)


def check_sparse_fields(fill, eo, hist, pay, lo, hi, bl):
    """the field checks of a kind-3 block in the device's order; True = refused.  The mask is read only once the record is
    known to hold it."""
    mw, nch = mask_words(bl), nchunks(bl)
    if fill > 255 or bool(np.asarray(eo).any()) or hi - lo < mw:
        return True
    mask = pay[lo:lo + mw]
    if nch % 32 and int(mask[-1]) >> (nch % 32):
        return True
    klen = klen_of(mask, bl)
    if int(np.asarray(hist, np.uint64).sum()) != klen:
        return True
    return hi - lo != mw + (M.h0_words(hist) if klen else 0)


def read(buf, with_kinds=False, max_version=VERSION):
    """decoded bytes of a container of any version up to max_version, or ContainerError(what, frame, block)"""
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
        nsub, mw = T["nsub"], mask_words(bl)
        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            idx = int(W[T["bwt"] + b])
            wrong = kind > fmt.max_kind or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == SPARSE:
                wrong = check_sparse_fields(idx, eo, hist, pay, lo, hi, bl)
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
            elif kind == SPARSE:
                mask = pay[lo:lo + mw]
                klen = klen_of(mask, bl)
                K = M.h0_decode(hist, pay[lo + mw:hi], klen)[0] if klen else np.zeros(0, np.uint8)
                blk = join(int(W[T["bwt"] + b]), mask, K, bl)
            elif kind == M.HUFF0:
                blk, used = M.h0_decode(hist, pay[lo:hi], bl)
                assert (used + 31) // 32 + 1 == hi - lo
            else:
                blk = M.O.decompress(int(W[T["bwt"] + b]), hist, W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
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


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 5, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c5, elem):
    """[(name, container, (what, frame, block))] from the valid version-5 container c5 (header flags as written).  It needs a
    kind-3 block with kept and elided chunks that is not the last of its frame, and a kind-3 block whose last chunk is short,
    with both mask values present (for the unused bits and for the swap that changes klen)."""
    lay = M.layout(c5)
    flags = struct.unpack("<H", c5[6:8])[0]

    def blocks3(pred):
        for fi, fr in enumerate(lay["frames"]):
            for b, (s, e, kind) in enumerate(fr["records"]):
                if kind == SPARSE and pred(fr, b, s, e):
                    return fi, fr, b, s, e
        raise AssertionError("the container lacks the block a refusal case needs")

    def mask_of(fr, s):
        return np.frombuffer(c5[s:s + 4 * mask_words(fr["blk_len"])], np.uint32)

    def mixed(fr, s):
        m, nch = mask_of(fr, s), nchunks(fr["blk_len"])
        kept = sum(bin(int(w)).count("1") for w in m)
        return 0 < kept < nch

    fi, fr, b, s, e = blocks3(lambda fr, b, s, e: b + 1 < fr["nb"] and mixed(fr, s))
    T = M.tables_layout(fr["nb"], fr["blk_len"])
    t0 = fr["tables"][0]

    def poke(word_off, value):
        x = bytearray(c5)
        x[t0 + 4 * word_off:t0 + 4 * word_off + 4] = struct.pack("<I", value)
        return M.retable(bytes(x), fr["start"])

    def resize(d):
        x = bytearray(c5)
        W = np.frombuffer(bytes(x[t0:t0 + 4 * T["words"]]), np.uint32).copy()
        po = W[T["pay_off"]:T["pay_off"] + 2 * (fr["nb"] + 1)].view(np.uint64)
        po[b + 1] = np.uint64(int(po[b + 1]) + d)
        x[t0:t0 + 4 * T["words"]] = W.tobytes()
        return M.retable(bytes(x), fr["start"])

    fill = struct.unpack("<I", c5[t0 + 4 * (T["bwt"] + b):t0 + 4 * (T["bwt"] + b) + 4])[0]
    flipped = bytearray(c5)
    flipped[e - 6] ^= 0x20                                       # inside the stream, behind the mask
    first3 = blocks3(lambda *a: True)
    cases = [("kind 3 under a version-4 header", M.with_header(c5, 4, flags, elem) if flags else M.with_header(c5, 3, 0, elem),
              (M.FRAME_TABLE, first3[0], first3[2])),
             ("version 5 with flags 2", M.with_header(c5, VERSION, 2, elem), (M.STREAM_HEADER, -1, -1)),
             ("version 5 with flags 3", M.with_header(c5, VERSION, 3, elem), (M.STREAM_HEADER, -1, -1)),
             ("version 6", M.with_header(c5, 6, flags, elem), (M.STREAM_HEADER, -1, -1)),
             ("fill 256", poke(T["bwt"] + b, 256), (M.FRAME_TABLE, fi, b)),
             ("enc_off set", poke(T["enc_off"] + T["nsub"] * b, 1), (M.FRAME_TABLE, fi, b)),
             ("one word too many", resize(1), (M.FRAME_TABLE, fi, b)),
             ("one word too few", resize(-1), (M.FRAME_TABLE, fi, b)),
             ("a flipped stream bit", bytes(flipped), (M.RECORD_CRC, fi, b)),
             ("a flipped fill", poke(T["bwt"] + b, fill ^ 1), (M.DECODED_CRC, fi, b)),
             ("cut inside the mask", c5[:s + 2], (M.TRUNCATED, fi, -1))]
    if flags == 0 and elem == 0:
        cases.append(("version 5, flags 1, elem 0", M.with_header(c5, VERSION, 1, 0), (M.STREAM_HEADER, -1, -1)))
    # the short last chunk: a bit past the last chunk set; the last chunk's bit swapped with one of the other value
    fi2, fr2, b2, s2, e2 = blocks3(lambda fr, b, s, e: fr["blk_len"] % CHUNK and nchunks(fr["blk_len"]) % 32 and mixed(fr, s))
    nch, mw = nchunks(fr2["blk_len"]), mask_words(fr2["blk_len"])
    m = mask_of(fr2, s2).copy()
    m[-1] |= np.uint32(1 << (nch % 32))
    x = bytearray(c5)
    x[s2:s2 + 4 * mw] = m.tobytes()
    cases.append(("an unused mask bit set", bytes(x), (M.FRAME_TABLE, fi2, b2)))
    m = mask_of(fr2, s2).copy()
    last = (int(m[-1]) >> ((nch - 1) % 32)) & 1
    other = [c for c in range(nch - 1) if ((int(m[c // 32]) >> (c % 32)) & 1) != last][0]
    m[(nch - 1) // 32] ^= np.uint32(1 << ((nch - 1) % 32))
    m[other // 32] ^= np.uint32(1 << (other % 32))
    x = bytearray(c5)
    x[s2:s2 + 4 * mw] = m.tobytes()
    cases.append(("a kept and an elided bit swapped", bytes(x), (M.FRAME_TABLE, fi2, b2)))
    return cases, lay
