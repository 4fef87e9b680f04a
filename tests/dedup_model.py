"""Pure Python + numpy model of the dedup order-0 record (kind 6) and of format version 9 of the BWT container (INTEGRATION.md 4b,
"dedup"), built from container_model's parts: its CRCs, tables_layout, h0_encode / h0_decode / h0_words, filter_frame, ContainerError.

A block of bl bytes (of the filtered frame) is cut into chunks of 512 bytes (the last may be short); chunk c of block b of a frame
has the frame-wide id b * nch + c.  A kind-6 record is a mask of ceil(nch / 32) words -- bit c % 32 of word c // 32, from the LSB,
is 1 where chunk c is KEPT and 0 where it is ELIDED -- then one u32 per elided chunk, the id of its SOURCE chunk, then, when any
chunk is kept, the kind-2 stream of K, the kept chunks concatenated; hist[] counts the bytes of K and bwt_index is the lowest
block a source lies in.  The writer's rule: every chunk gets the 64-bit hash chunk_hashes() defines, cand(g) is the smallest id of
the frame with g's hash, and g is elided, with source cand(g), exactly when cand(g) < g and the two chunks agree in length and in
every byte; a block with E elided chunks is kind 6 when 15 * E >= mask words and kind 2 otherwise, each under the raw rule
(4 * words >= bl -> kind 1).  The reader takes any sources that pass the field checks.

The version-9 frame walk repeats container_model.read's; this file's reader takes versions 1 to 4 and 9, up to max_version."""
import struct
import zlib

import numpy as np

import container_model as M

CHUNK = 512
DEDUP = 6
VERSION = 9
KINDS = (M.HUFF, M.RAW, M.HUFF0, DEDUP)                          # what a version-9 frame may hold
FORMATS = {(VERSION, 0): (0,) + M.ELEMS, (VERSION, M.FLAG_DELTA): M.ELEMS}
GOLD = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def stream_format(version, flags, elem):
    """(Format, legal kinds) of a header triple, or None where the triple is not legal: versions 1 to 4 as ever, and 9"""
    if version == VERSION:
        if elem not in FORMATS.get((version, flags), ()):
            return None
        return M.Format(version, flags, elem, flags == M.FLAG_DELTA, DEDUP), KINDS
    fmt = M.stream_format(version, flags, elem)
    return None if fmt is None else (fmt, tuple(range(fmt.max_kind + 1)))


def nchunks(bl):
    return (bl + CHUNK - 1) // CHUNK


def mask_words(bl):
    return (nchunks(bl) + 31) // 32


def chunk_len(bl, c):
    return min(CHUNK, bl - CHUNK * c)


# ----------------------------------------------------------------------------------------------------------------------
# the hash and the map
# ----------------------------------------------------------------------------------------------------------------------
KEYS = np.array([((GOLD * (j + 1)) & MASK64) >> 32 for j in range(CHUNK // 4)], dtype=np.uint64)


def fmix64(h):
    """murmur3's finaliser over a uint64 array"""
    h = h.copy()
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xff51afd7ed558ccd)
    h ^= h >> np.uint64(33)
    h *= np.uint64(0xc4ceb9fe1a85ec53)
    h ^= h >> np.uint64(33)
    return h


def chunk_hashes(blk):
    """the 64-bit hash of every chunk of one block: the chunk zero-padded to 512 bytes as little-endian words w_0 .. w_127 counted
    from the chunk's start, k_j = the high half of GOLD * (j + 1) mod 2^64, s = sum over i < 64 of ((w_2i + k_2i) mod 2^32) *
    ((w_2i+1 + k_2i+1) mod 2^32), plus the chunk's length, mod 2^64; h = fmix64(s)"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8).reshape(-1)
    nch = nchunks(blk.size)
    padded = np.zeros(nch * CHUNK, np.uint8)
    padded[:blk.size] = blk
    w = padded.view("<u4").reshape(nch, CHUNK // 4).astype(np.uint64)
    t = (w + KEYS[None, :]) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        s = (t[:, 0::2] * t[:, 1::2]).sum(axis=1, dtype=np.uint64)
        s += np.array([chunk_len(blk.size, c) for c in range(nch)], dtype=np.uint64)
        return fmix64(s)


def map_segments(segs, max_len=None):
    """src[i * nch + c] for the segments (the blocks of one frame, in order), nch = ceil(max_len / 512): the id of the chunk's
    source under the writer's rule, or the chunk's own id when it is kept; the entry of an id past its segment's end is its own id"""
    segs = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1) for s in segs]
    max_len = max((s.size for s in segs), default=0) if max_len is None else max_len
    segs = [s[:max_len] for s in segs]
    nch = nchunks(max_len)
    src = np.arange(len(segs) * nch, dtype=np.uint32)
    first = {}                                                    # hash -> the smallest id that has it
    for i, s in enumerate(segs):
        hs = chunk_hashes(s).tolist()
        for c, h in enumerate(hs):
            g = i * nch + c
            cand = first.setdefault(h, g)
            if cand < g:
                sb, sc = divmod(cand, nch)
                a, b = s[CHUNK * c:CHUNK * c + CHUNK], segs[sb][CHUNK * sc:CHUNK * sc + CHUNK]
                if a.size == b.size and np.array_equal(a, b):
                    src[g] = cand
    return src


def fill_segments(segs, src, max_len=None):
    """what glcDedupFillSegments leaves: every chunk whose entry is smaller than its id and names a chunk of its own length is
    copied from there (from the bytes as they were); every other entry is skipped"""
    before = [np.array(s, dtype=np.uint8).reshape(-1) for s in segs]
    max_len = max((s.size for s in before), default=0) if max_len is None else max_len
    nch = nchunks(max_len)
    out = [s.copy() for s in before]
    for i, s in enumerate(before):
        L = min(s.size, max_len)
        for c in range(nchunks(L)):
            g, e = i * nch + c, int(src[i * nch + c])
            if e >= g:
                continue
            sb, sc = divmod(e, nch)
            SL = min(before[sb].size, max_len)
            if CHUNK * sc >= SL or chunk_len(SL, sc) != chunk_len(L, c):
                continue
            out[i][CHUNK * c:CHUNK * c + chunk_len(L, c)] = before[sb][CHUNK * sc:CHUNK * sc + chunk_len(L, c)]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the kind-6 record and the writer
# ----------------------------------------------------------------------------------------------------------------------
def mask_bits(mask, nch):
    """kept[c] of the nch chunks from mask words"""
    return np.unpackbits(np.asarray(mask, np.uint32).astype("<u4").view(np.uint8), bitorder="little")[:nch].astype(bool)


def mask_of(kept, bl):
    bits = np.zeros(32 * mask_words(bl), np.uint8)
    bits[:nchunks(bl)] = kept
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def klen_of(mask, bl):
    """bytes of K for this mask (its unused bits zero) over a block of bl bytes"""
    nch = nchunks(bl)
    kept = sum(bin(int(w)).count("1") for w in mask)
    last = nch and (int(mask[(nch - 1) // 32]) >> ((nch - 1) % 32)) & 1
    return CHUNK * kept - (CHUNK * nch - bl if last else 0)


def kept_bytes(blk, kept):
    nch = nchunks(blk.size)
    idx = np.arange(nch * CHUNK).reshape(nch, CHUNK)[np.asarray(kept, bool)].reshape(-1)
    return blk[idx[idx < blk.size]]


def place_kept(out, kept, K):
    """K back into the kept chunks of the block `out`, the elided chunks left as they are"""
    nch = nchunks(out.size)
    idx = np.arange(nch * CHUNK).reshape(nch, CHUNK)[np.asarray(kept, bool)].reshape(-1)
    idx = idx[idx < out.size]
    assert idx.size == len(K)
    out[idx] = K


def _raw(blk):
    return M.encode_block(blk, M.RAW)


def encode_block6(blk, src_row, b):
    """(kind, lo, hist of K, enc_off, record words) of block b of a frame as a dedup record with the sources src_row (the block's
    nch entries of the frame's map), raw when 4 * words >= blk_len"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    nch = nchunks(blk.size)
    nsub = (blk.size + M.HUFF_BLOCK - 1) // M.HUFF_BLOCK
    own = np.arange(b * nch, (b + 1) * nch, dtype=np.uint32)
    kept = np.asarray(src_row, np.uint32) == own
    refs = np.asarray(src_row, np.uint32)[~kept]
    K = kept_bytes(blk, kept)
    lo = min([b] + [int(r) // nch for r in refs])
    parts = [mask_of(kept, blk.size), refs.astype(np.uint32)]
    hist = np.zeros(256, np.uint32)
    if K.size:
        hist, stream = M.h0_encode(K)
        parts.append(stream)
    words = np.concatenate(parts)
    if 4 * words.size >= blk.size:
        return _raw(blk)
    return DEDUP, lo, hist, np.zeros(nsub, np.uint32), words


def rule_kind(src_row, b, bl):
    """rule (4): kind 6 when 15 * E >= mask words, kind 2 otherwise"""
    nch = nchunks(bl)
    E = int((np.asarray(src_row, np.uint32) != np.arange(b * nch, (b + 1) * nch, dtype=np.uint32)).sum())
    return DEDUP if 15 * E >= mask_words(bl) else M.HUFF0


def encode_frame_blocks(blocks, kinds):
    """[(kind, bwt_index, hist, enc_off, words)] of a frame's blocks; kinds[b] is 0, 1, 2, 6 or "rule" (what the dedup writer makes)"""
    src = map_segments(blocks, len(blocks[0]))
    nch = nchunks(len(blocks[0]))
    out = []
    for b, blk in enumerate(blocks):
        row = src[b * nch:(b + 1) * nch]
        k = rule_kind(row, b, blk.size) if kinds[b] == "rule" else kinds[b]
        out.append(encode_block6(blk, row, b) if k == DEDUP else M.encode_block(blk, k))
    return out


def _frame(blocks, blk_len, kinds):
    nb = len(blocks)
    T = M.tables_layout(nb, blk_len)
    W = np.zeros(T["words"], dtype=np.uint32)
    recs, pay_off = [], [0]
    for b, (blk, (kind, idx, hist, eo, words)) in enumerate(zip(blocks, encode_frame_blocks(blocks, kinds))):
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
    """The version-9 container of `data` as a writer plan of n = block_len, `rows` rows, filter element size `elem`, delta mode
    `delta`, the order-0 codec and the dedup mode on makes it.  `kinds` (cycled over the stream's blocks; each 0, 1, 2, 6 or
    "rule") forces the codec of each block instead, every one still under its raw rule."""
    elem = 0 if elem == 1 else elem
    got = stream_format(VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert got is not None
    fmt = got[0]
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


def size(data, block_len, rows, elem=0, delta=False):
    """len(write(data, block_len, rows, elem, delta)) without coding anything: every record's words follow from the map, the byte
    counts and h0_words.  For inputs of benchmark size, where write()'s bit-by-bit coder is too slow; (bytes, kinds)"""
    elem = 0 if elem == 1 else elem
    fmt = stream_format(VERSION, M.FLAG_DELTA if delta else 0, elem)[0]
    a = M._u8(data).reshape(-1)
    n, pos, total, kinds = a.size, 0, 32 + 16, []
    while pos < n:
        left = n - pos
        nb, bl = (min(rows, left // block_len), block_len) if left >= block_len else (1, left)
        f = M.filter_frame(a[pos:pos + nb * bl], fmt)
        blocks = [f[i * bl:(i + 1) * bl] for i in range(nb)]
        src, nch, P = map_segments(blocks, bl), nchunks(bl), 0
        for b, blk in enumerate(blocks):
            row = src[b * nch:(b + 1) * nch]
            kind = rule_kind(row, b, bl)
            if kind == DEDUP:
                kept = row == np.arange(b * nch, (b + 1) * nch, dtype=np.uint32)
                K = kept_bytes(blk, kept)
                words = mask_words(bl) + int((~kept).sum()) + (M.h0_words(np.bincount(K, minlength=256)) if K.size else 0)
            else:
                words = M.h0_words(np.bincount(blk, minlength=256))
            if 4 * words >= bl:
                kind, words = M.RAW, M.raw_words(bl)
            kinds.append(kind)
            P += words
        total += 32 + 4 * M.tables_layout(nb, bl)["words"] + 4 * M._pad2(P)
        pos += nb * bl
    return total, kinds


# ----------------------------------------------------------------------------------------------------------------------
# the reader
# ----------------------------------------------------------------------------------------------------------------------
def check_dedup_fields(b, lo_blk, eo, hist, pay, lo, hi, bl, kept_of):
    """the field checks of kind-6 block b in the device's order (behind the legal kind and the payload offsets); True = refused.
    kept_of(block) -> the kept bits of an earlier block of the frame (all ones for a kind other than 6), or None where that
    block's own record does not hold its mask.  The mask and the refs are read only once the record is known to hold them."""
    mw, nch = mask_words(bl), nchunks(bl)
    if bool(np.asarray(eo).any()) or hi - lo < mw:
        return True
    mask = pay[lo:lo + mw]
    kept = mask_bits(mask, nch)
    E = nch - int(kept.sum())
    if hi - lo < mw + E:
        return True
    if nch % 32 and int(mask[-1]) >> (nch % 32):
        return True
    refs = pay[lo + mw:lo + mw + E].tolist()
    for c, r in zip(np.nonzero(~kept)[0].tolist(), refs):
        sb, sc = divmod(r, nch)
        if r >= b * nch + c or sb < lo_blk or sb > b or chunk_len(bl, sc) != chunk_len(bl, c):
            return True
        sk = kept if sb == b else kept_of(sb)
        if sk is None or not sk[sc]:
            return True
    if lo_blk > b:
        return True
    klen = klen_of(mask, bl)
    if int(np.asarray(hist, np.uint64).sum()) != klen:
        return True
    return hi - lo != mw + E + (M.h0_words(hist) if klen else 0)


def read(buf, with_kinds=False, max_version=VERSION):
    """decoded bytes of a container of versions 1 to 4 and 9, up to max_version, or ContainerError(what, frame, block)"""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise M.ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    got = stream_format(ver, flags, elem)
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20
            or got is None or ver > max_version):
        raise M.ContainerError(M.STREAM_HEADER)
    fmt, legal = got
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
        nsub, mw, nch = T["nsub"], mask_words(bl), nchunks(bl)

        def offsets_bad(b):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            return kind not in legal or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)

        def kept_of(b):
            if offsets_bad(b):
                return None
            if int(W[T["kind"] + b]) != DEDUP:
                return np.ones(nch, bool)
            lo, hi = int(po[b]), int(po[b + 1])
            return mask_bits(pay[lo:lo + mw], nch) if hi - lo >= mw else None

        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            idx = int(W[T["bwt"] + b])
            wrong = offsets_bad(b)
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == DEDUP:
                wrong = check_dedup_fields(b, idx, eo, hist, pay, lo, hi, bl, kept_of)
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
        frame = np.zeros(nb * bl, np.uint8)
        copies = []                                             # (destination id, source id): the one copy pass behind the joins
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            blk = frame[b * bl:(b + 1) * bl]
            if kind == M.RAW:
                blk[:] = pay[lo:hi].view(np.uint8)[:bl]
            elif kind == DEDUP:
                kept = mask_bits(pay[lo:lo + mw], nch)
                E = nch - int(kept.sum())
                klen = klen_of(pay[lo:lo + mw], bl)
                K = M.h0_decode(hist, pay[lo + mw + E:hi], klen)[0] if klen else np.zeros(0, np.uint8)
                place_kept(blk, kept, K)
                copies += [(b * nch + int(c), int(r)) for c, r in zip(np.nonzero(~kept)[0], pay[lo + mw:lo + mw + E])]
            elif kind == M.HUFF0:
                blk[:], used = M.h0_decode(hist, pay[lo:hi], bl)
                assert (used + 31) // 32 + 1 == hi - lo
            else:
                blk[:] = M.O.decompress(int(W[T["bwt"] + b]), hist, W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)], pay[lo:hi], bl)
            kinds.append(kind)
        for g, r in copies:
            (db, dc), (sb, sc) = divmod(g, nch), divmod(r, nch)
            n = chunk_len(bl, dc)
            frame[db * bl + CHUNK * dc:db * bl + CHUNK * dc + n] = frame[sb * bl + CHUNK * sc:sb * bl + CHUNK * sc + n]
        for b in range(nb):
            if zlib.crc32(frame[b * bl:(b + 1) * bl].tobytes()) != int(W[T["crc_raw"] + b]):
                raise M.ContainerError(M.DECODED_CRC, fi, b)
        out.append(M.unfilter_frame(frame, fmt))
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
# range reads: which blocks of a frame are decoded for the needed blocks [first, last] (csrc/dedup_rule.h)
# ----------------------------------------------------------------------------------------------------------------------
def first_block(kinds, bwt_index, first, last):
    """the first block to decode: the smallest bwt_index of a needed kind-6 block, or first; the blocks in front of `first` are
    sources only -- decoded and joined, neither filled nor compared with their crc_raw"""
    return min([first] + [int(bwt_index[b]) for b in range(first, last + 1) if kinds[b] == DEDUP])


def blocks_decoded(kinds, bwt_index, first, last):
    return last - first_block(kinds, bwt_index, first, last) + 1


# ----------------------------------------------------------------------------------------------------------------------
# the refusal cases of version 9, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def frame_tables(c, fr):
    """(T, W) of a frame of M.layout(c): the table layout and a copy of the table words"""
    T = M.tables_layout(fr["nb"], fr["blk_len"])
    return T, np.frombuffer(c[fr["tables"][0]:fr["tables"][1]], np.uint32).copy()


def record_parts(c, fr, b):
    """(mask, refs, stream) of kind-6 block b of a frame of M.layout(c)"""
    s, e, kind = fr["records"][b]
    assert kind == DEDUP
    words = np.frombuffer(c[s:e], np.uint32)
    mw, nch = mask_words(fr["blk_len"]), nchunks(fr["blk_len"])
    E = nch - int(mask_bits(words[:mw], nch).sum())
    return words[:mw].copy(), words[mw:mw + E].copy(), words[mw + E:].copy()


def refusal_cases(c9, elem):
    """[(name, container, (what, frame, block))] from the valid version-9 container c9 (header flags as written), and its layout.
    It needs a kind-6 block that is not the last of its frame, whose block length is no multiple of 512 and whose chunk count is
    none of 32, with a kept chunk, two full elided chunks and a source in an earlier block; and a kind-2 block."""
    lay = M.layout(c9)
    flags = struct.unpack("<H", c9[6:8])[0]

    def pick():
        for fi, fr in enumerate(lay["frames"]):
            bl, nch = fr["blk_len"], nchunks(fr["blk_len"])
            T, W = frame_tables(c9, fr)
            for b, (s, e, kind) in enumerate(fr["records"]):
                if kind != DEDUP or b + 1 >= fr["nb"] or bl % CHUNK == 0 or nch % 32 == 0 or int(W[T["bwt"] + b]) >= b:
                    continue
                mask, refs, stream = record_parts(c9, fr, b)
                el = np.nonzero(~mask_bits(mask, nch))[0]
                if stream.size and (el < nch - 1).sum() >= 2:
                    return fi, fr, b
        raise AssertionError("the container lacks the block the refusal cases need")

    fi, fr, b = pick()
    bl, nch, mw = fr["blk_len"], nchunks(fr["blk_len"]), mask_words(fr["blk_len"])
    T, W0 = frame_tables(c9, fr)
    t0 = fr["tables"][0]
    s, e, _ = fr["records"][b]
    mask, refs, stream = record_parts(c9, fr, b)
    elided = np.nonzero(~mask_bits(mask, nch))[0]
    full = [i for i, c in enumerate(elided) if c < nch - 1]       # positions in refs of two full elided chunks
    lo = int(W0[T["bwt"] + b])

    def poke(word_off, value):
        x = bytearray(c9)
        x[t0 + 4 * word_off:t0 + 4 * word_off + 4] = struct.pack("<I", value & 0xFFFFFFFF)
        return M.retable(bytes(x), fr["start"])

    def record(mask2, refs2):
        """the block's record with another mask or other refs, its record CRC remade: only the field checks see it"""
        words = np.concatenate([mask2, refs2, stream]).astype(np.uint32)
        assert 4 * words.size == e - s
        x = bytearray(c9)
        x[s:e] = words.tobytes()
        x[t0 + 4 * (T["crc_rec"] + b):t0 + 4 * (T["crc_rec"] + b) + 4] = struct.pack("<I", zlib.crc32(words.tobytes()))
        return M.retable(bytes(x), fr["start"])

    def with_ref(i, value):
        r = refs.copy()
        r[i] = value
        return record(mask, r)

    def resize(d):
        x = bytearray(c9)
        W = W0.copy()
        po = W[T["pay_off"]:T["pay_off"] + 2 * (fr["nb"] + 1)].view(np.uint64)
        po[b + 1] = np.uint64(int(po[b + 1]) + d)
        x[t0:t0 + 4 * T["words"]] = W.tobytes()
        return M.retable(bytes(x), fr["start"])

    def first_of(kind):
        for i, f in enumerate(lay["frames"]):
            for j, (_, _, k) in enumerate(f["records"]):
                if k == kind:
                    return i, f, j
        raise AssertionError("the container lacks a block of kind %d" % kind)

    own = b * nch + int(elided[full[1]])
    other = b * nch + int(elided[full[0]])                        # an elided chunk of smaller id and equal length
    bad_bit = mask.copy()
    bad_bit[-1] |= np.uint32(1 << (nch % 32))
    kept_other = [g for g in range(lo * nch, b * nch) if g % nch < nch - 1 and g != int(refs[full[0]])][0]
    f6 = first_of(DEDUP)
    f2i, f2, f2b = first_of(M.HUFF0)
    T2 = M.tables_layout(f2["nb"], f2["blk_len"])

    def poke2(kind):
        x = bytearray(c9)
        o = f2["tables"][0] + 4 * (T2["kind"] + f2b)
        x[o:o + 4] = struct.pack("<I", kind)
        return M.retable(bytes(x), f2["start"])

    flipped = bytearray(c9)
    flipped[e - 6] ^= 0x20                                       # inside the stream, behind the mask and the refs
    refused = (M.FRAME_TABLE, fi, b)
    cases = [("kind 6 under a version-%d header" % (4 if flags else 3), M.with_header(c9, 4, flags, elem) if flags else M.with_header(c9, 3, 0, elem),
              (M.FRAME_TABLE, f6[0], f6[2])),
             ("version 9 with flags 2", M.with_header(c9, VERSION, 2, elem), (M.STREAM_HEADER, -1, -1)),
             ("version 9 with flags 3", M.with_header(c9, VERSION, 3, elem), (M.STREAM_HEADER, -1, -1)),
             ("version 9 with elem 3", M.with_header(c9, VERSION, flags, 3), (M.STREAM_HEADER, -1, -1)),
             ("version 10", M.with_header(c9, 10, flags, elem), (M.STREAM_HEADER, -1, -1)),
             ("kind 3 under version 9", poke2(3), (M.FRAME_TABLE, f2i, f2b)),
             ("kind 4 under version 9", poke2(4), (M.FRAME_TABLE, f2i, f2b)),
             ("kind 5 under version 9", poke2(5), (M.FRAME_TABLE, f2i, f2b)),
             ("kind 7", poke2(7), (M.FRAME_TABLE, f2i, f2b)),
             ("enc_off set", poke(T["enc_off"] + T["nsub"] * b, 1), refused),
             ("a ref equal to its own id", with_ref(full[1], own), refused),
             ("a ref into a later block", with_ref(full[0], (b + 1) * nch), refused),
             ("a ref past the frame", with_ref(full[0], 0xFFFFFFFF), refused),
             ("a ref to an elided chunk", with_ref(full[1], other), refused),
             ("a full chunk sourced from a short one", with_ref(full[0], (b - 1) * nch + nch - 1), refused),
             ("a ref below bwt_index", poke(T["bwt"] + b, lo + 1), refused),
             ("bwt_index above the block", poke(T["bwt"] + b, b + 1), refused),
             ("an unused mask bit set", record(bad_bit, refs), refused),
             ("a wrong sum of hist", poke(T["hist"] + 256 * b, int(W0[T["hist"] + 256 * b]) + 1), refused),
             ("one word too many", resize(1), refused),
             ("one word too few", resize(-1), refused),
             ("a flipped stream bit", bytes(flipped), (M.RECORD_CRC, fi, b)),
             ("a ref to another kept chunk", with_ref(full[0], kept_other), (M.DECODED_CRC, fi, b)),
             ("cut inside the mask", c9[:s + 2], (M.TRUNCATED, fi, -1))]
    if flags == 0 and elem == 0:
        cases.append(("version 9, flags 1, elem 0", M.with_header(c9, VERSION, 1, 0), (M.STREAM_HEADER, -1, -1)))
    return cases, lay
