"""Pure Python + numpy model of the rANS order-0 record (kind 5) and of format version 7 of the BWT container,
built from container_model's parts: its CRCs, tables_layout, encode_block, filter_frame, ContainerError.

A block of n bytes has 12-bit probabilities q[s] quantised from its byte counts (quantise), cum[s] their running sum; slot k of
the 4096 belongs to the symbol s with cum[s] <= k < cum[s] + q[s].  The block is cut into chunks of 32768 bytes; a chunk is coded
by 64 interleaved 32-bit states (lower bound 2^16, 16-bit units), symbol i of the chunk in lane i % 64 at step i // 64.  The
encoder runs from the last step to step 0 and every lane starts at 2^16; the decoder runs from step 0 up, and the order of a
chunk's units is the decoder's: by step, then by lane.  A record is u32 units[nch], then for every chunk its 64 states and its
units, two to a word, zero-padded.  The writer's rule: kind 5 unless 4 * words >= n, then raw.

This file's reader is the reader of a plan with the mode on: versions 1 to 4 and 7."""
import struct
import zlib

import numpy as np

import container_model as M

ANS = 5
VERSION = 7
PROB_BITS, TOTAL = 12, 4096
LOW = 1 << 16
CHUNK, LANES = 32768, 64
MAX_LEN = 1 << 20
FORMATS = dict(M.FORMATS)
FORMATS.update({(VERSION, 0): ((0,) + M.ELEMS, ANS), (VERSION, M.FLAG_DELTA): (M.ELEMS, ANS)})
ILLEGAL_KINDS = {VERSION: (3, 4)}                               # kinds at or below a version's max_kind that it does not take


def stream_format(version, flags, elem):
    elems, max_kind = FORMATS.get((version, flags), ((), M.RAW))
    return M.Format(version, flags, elem, flags == M.FLAG_DELTA, max_kind) if elem in elems else None


def nchunks(n):
    return (n + CHUNK - 1) // CHUNK


def chunk_len(n, c):
    return min(CHUNK, n - c * CHUNK)


def bound_words(n):
    """room for the largest record of n bytes (glcAnsBoundWords)"""
    return nchunks(n) * (1 + LANES) + (n + 1) // 2 + nchunks(n)


def words_of(units):
    """the record's word count from its chunks' unit counts"""
    return len(units) + sum(LANES + (int(u) + 1) // 2 for u in units)


def quantise(hist, n):
    """q[256] summing to 4096 with q >= 1 exactly where hist > 0; also whether the R < 0 path was taken"""
    q = [0 if int(h) == 0 else max(1, int(h) * TOTAL // n) for h in hist]
    R = TOTAL - sum(q)
    took = R < 0
    if R > 0:
        q[max(range(256), key=lambda s: (q[s], -s))] += R
    while R < 0:
        i = max(range(256), key=lambda s: (q[s], -s))
        t = min(q[i] - 1, -R)
        q[i] -= t
        R += t
    return np.asarray(q, np.int64), took


def tables(hist, n):
    """(q, cum, slot -> symbol)"""
    q, _ = quantise(hist, n)
    cum = np.concatenate([[0], np.cumsum(q)[:-1]]).astype(np.int64)
    return q, cum, np.repeat(np.arange(256, dtype=np.int64), q)


def _steps(blk):
    """the block as [nch, 512, 64] symbols and the mask of the places that hold one"""
    n, nch = blk.size, nchunks(blk.size)
    pad = np.zeros(nch * CHUNK, np.int64)
    pad[:n] = blk
    act = np.arange(nch * CHUNK) < n
    return pad.reshape(nch, CHUNK // LANES, LANES), act.reshape(nch, CHUNK // LANES, LANES)


def encode_record(blk):
    """(hist u32[256], record words u32) of one block"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8).reshape(-1)
    n, nch = blk.size, nchunks(blk.size)
    assert 1 <= n <= MAX_LEN
    hist = np.bincount(blk, minlength=256).astype(np.uint32)
    q, cum, _ = tables(hist, n)
    sym, act = _steps(blk)
    x = np.full((nch, LANES), LOW, np.int64)
    emitted = np.zeros(sym.shape, bool)
    unit = np.zeros(sym.shape, np.int64)
    for t in range(sym.shape[1] - 1, -1, -1):
        s, a = sym[:, t], act[:, t]
        f, c = np.where(a, q[s], 1), cum[s]
        e = a & (x >= f << 20)
        emitted[:, t], unit[:, t] = e, x & 0xFFFF
        x = np.where(e, x >> 16, x)
        x = np.where(a, (x // f << PROB_BITS) + x % f + c, x)
    parts = [np.asarray([int(emitted[c].sum()) for c in range(nch)], np.uint32)]
    for c in range(nch):
        u = unit[c][emitted[c]].astype(np.uint16)                # C order: by step, then by lane
        parts += [x[c].astype(np.uint32), np.concatenate([u, np.zeros(u.size & 1, np.uint16)]).view(np.uint32)]
    return hist, np.concatenate(parts)


def decode_record(hist, words, n):
    """n bytes from a record whose fields have passed the checks; a lane that asks for a unit beyond its chunk's count gets 0"""
    words = np.asarray(words, np.uint32)
    nch = nchunks(n)
    q, cum, slot = tables(hist, n)
    counts = words[:nch].astype(np.int64)
    x = np.zeros((nch, LANES), np.int64)
    maxu = int(counts.max()) if nch else 0
    units = np.zeros((nch, maxu + 1), np.int64)
    so = nch
    for c in range(nch):
        x[c] = words[so:so + LANES]
        u = words[so + LANES:so + LANES + (int(counts[c]) + 1) // 2].view(np.uint16)[:int(counts[c])]
        units[c, :u.size] = u
        so += LANES + (int(counts[c]) + 1) // 2
    act = (np.arange(nch * CHUNK) < n).reshape(nch, CHUNK // LANES, LANES)
    out = np.zeros(act.shape, np.uint8)
    pos = np.zeros(nch, np.int64)
    for t in range(act.shape[1]):
        a = act[:, t]
        k = x & (TOTAL - 1)
        s = slot[k]
        out[:, t] = s
        nx = q[s] * (x >> PROB_BITS) + k - cum[s]
        need = a & (nx < LOW)
        idx = pos[:, None] + np.cumsum(need, axis=1) - need
        u = np.where(idx < counts[:, None], np.take_along_axis(units, np.minimum(idx, maxu), axis=1), 0)
        x = np.where(a, np.where(need, (nx << 16) | u, nx), x)
        pos += need.sum(axis=1)
    return out.reshape(-1)[:n]


def encode_block5(blk):
    """(kind, 0, hist, enc_off, record words) of one block as an rANS record, raw when 4 * words >= blk_len"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8)
    hist, words = encode_record(blk)
    if 4 * words.size >= blk.size:
        return M.encode_block(blk, M.RAW)
    return ANS, 0, hist, np.zeros((blk.size + M.HUFF_BLOCK - 1) // M.HUFF_BLOCK, np.uint32), words


def encode_block(blk, codec):
    """codec 0, 1, 2: container_model's; 5 or "rule": what the rANS writer makes"""
    return encode_block5(blk) if codec in (ANS, "rule") else M.encode_block(blk, codec)


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
    tables_ = W.tobytes()
    payload = b"".join(w.tobytes() for w in recs) + (b"\0\0\0\0" if P & 1 else b"")
    return hdr24 + struct.pack("<II", zlib.crc32(hdr24 + tables_), 0) + tables_ + payload


def write(data, block_len, rows, elem=0, delta=False, kinds=None):
    """The version-7 container of `data` as a writer plan of n = block_len, `rows` rows, filter element size `elem`, delta mode
    `delta`, the order-0 codec and the rANS mode on makes it.  `kinds` (cycled over the stream's blocks; each 0, 1, 2 or 5)
    forces the codec of each block instead, every one still under its raw rule."""
    elem = 0 if elem == 1 else elem
    fmt = stream_format(VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert fmt is not None
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= MAX_LEN and rows >= 1
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


def check_ans_fields(idx, eo, hist, pay, lo, hi, bl):
    """the field checks 2 to 7 of a kind-5 block in the specified order; True = refused.  The counts are read only once the
    record is known to hold them."""
    nch = nchunks(bl)
    if int(np.asarray(hist, np.uint64).sum()) != bl or idx != 0 or bool(np.asarray(eo).any()) or hi - lo < nch:
        return True
    units = pay[lo:lo + nch]
    if any(int(units[c]) > chunk_len(bl, c) for c in range(nch)):
        return True
    return words_of(units) != hi - lo


def read(buf, with_kinds=False):
    """decoded bytes of a container of version 1 to 4 or 7, or ContainerError(what, frame, block)"""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise M.ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    fmt = stream_format(ver, flags, elem)
    if magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20 or fmt is None:
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
            wrong = (kind > fmt.max_kind or kind in ILLEGAL_KINDS.get(ver, ()) or lo > hi or hi > P or (b == 0 and lo != 0)
                     or (b == nb - 1 and hi != P))
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == ANS:
                wrong = check_ans_fields(idx, eo, hist, pay, lo, hi, bl)
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
            elif kind == ANS:
                blk = decode_record(hist, pay[lo:hi], bl)
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
# the refusal cases of version 7, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
def refusal_cases(c7, elem):
    """[(name, container, (what, frame, block))] from the valid version-7 container c7 (header flags as written), as the reader
    of a plan with the mode on sees them.  It needs a kind-5 block that is not the last of its frame."""
    lay = M.layout(c7)
    flags = struct.unpack("<H", c7[6:8])[0]

    def block5(pred):
        for fi, fr in enumerate(lay["frames"]):
            for b, (s, e, kind) in enumerate(fr["records"]):
                if kind == ANS and pred(fr, b):
                    return fi, fr, b, s, e
        raise AssertionError("the container lacks the block a refusal case needs")

    fi, fr, b, s, e = block5(lambda fr, b: b + 1 < fr["nb"])
    T = M.tables_layout(fr["nb"], fr["blk_len"])
    t0 = fr["tables"][0]
    nch = nchunks(fr["blk_len"])

    def poke(word_off, value):
        x = bytearray(c7)
        x[t0 + 4 * word_off:t0 + 4 * word_off + 4] = struct.pack("<I", value)
        return M.retable(bytes(x), fr["start"])

    def resize(d=None, to=None):
        x = bytearray(c7)
        W = np.frombuffer(bytes(x[t0:t0 + 4 * T["words"]]), np.uint32).copy()
        po = W[T["pay_off"]:T["pay_off"] + 2 * (fr["nb"] + 1)].view(np.uint64)
        po[b + 1] = np.uint64(int(po[b]) + to if d is None else int(po[b + 1]) + d)
        x[t0:t0 + 4 * T["words"]] = W.tobytes()
        return M.retable(bytes(x), fr["start"])

    def hist_at(sym):
        off = t0 + 4 * (T["hist"] + 256 * b + sym)
        return struct.unpack("<I", c7[off:off + 4])[0]

    def record_word(i, value):
        x = bytearray(c7)
        x[s + 4 * i:s + 4 * i + 4] = struct.pack("<I", value)
        return bytes(x)

    present = [sym for sym in range(256) if hist_at(sym)]
    big = max(present, key=hist_at)
    other = min(range(256), key=hist_at)                          # (the sum stays; the probabilities do not)
    traded = bytearray(c7)
    for sym, v in ((big, hist_at(other)), (other, hist_at(big))):
        off = t0 + 4 * (T["hist"] + 256 * b + sym)
        traded[off:off + 4] = struct.pack("<I", v)
    flipped = bytearray(c7)
    flipped[e - 6] ^= 0x20
    first5 = block5(lambda *a: True)
    none = (M.STREAM_HEADER, -1, -1)
    low = M.with_header(c7, 4, flags, elem) if flags else M.with_header(c7, 3, 0, elem)
    cases = [("version 8", M.with_header(c7, 8, flags, elem), none),
             ("version 7 with flags 2", M.with_header(c7, VERSION, 2, elem), none),
             ("version 7 with flags 3", M.with_header(c7, VERSION, 3, elem), none),
             ("kind 5 under a version-%d header" % (4 if flags else 3), low, (M.FRAME_TABLE, first5[0], first5[2])),
             ("kind 5 under a version-5 header", M.with_header(c7, 5, flags, elem), none),     # (this reader does not speak 5 or 6)
             ("kind 5 under a version-6 header", M.with_header(c7, 6, flags, elem), none),
             ("kind 3 under version 7", poke(T["kind"] + b, 3), (M.FRAME_TABLE, fi, b)),
             ("kind 4 under version 7", poke(T["kind"] + b, 4), (M.FRAME_TABLE, fi, b)),
             ("kind 6", poke(T["kind"] + b, 6), (M.FRAME_TABLE, fi, b)),
             ("a count too many", poke(T["hist"] + 256 * b + big, hist_at(big) + 1), (M.FRAME_TABLE, fi, b)),
             ("bwt_index set", poke(T["bwt"] + b, 1), (M.FRAME_TABLE, fi, b)),
             ("enc_off set", poke(T["enc_off"] + T["nsub"] * b, 1), (M.FRAME_TABLE, fi, b)),
             ("a record shorter than its counts", resize(to=nch - 1), (M.FRAME_TABLE, fi, b)),
             ("more units than symbols", record_word(nch - 1, chunk_len(fr["blk_len"], nch - 1) + 1), (M.FRAME_TABLE, fi, b)),
             ("one word too many", resize(1), (M.FRAME_TABLE, fi, b)),
             ("one word too few", resize(-1), (M.FRAME_TABLE, fi, b)),
             ("a flipped unit bit", bytes(flipped), (M.RECORD_CRC, fi, b)),
             ("two counts traded", M.retable(bytes(traded), fr["start"]), (M.DECODED_CRC, fi, b)),
             ("cut inside the counts", c7[:s + 2], (M.TRUNCATED, fi, -1))]
    if flags == 0 and elem == 0:
        cases.append(("version 7, flags 1, elem 0", M.with_header(c7, VERSION, 1, 0), none))
    return cases, lay
