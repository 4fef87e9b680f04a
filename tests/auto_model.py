"""Pure Python + numpy model of the auto mode of the container's order-0 codec and of format version 8 of the BWT container
(INTEGRATION.md 4b), built from the parts of container_model, sparse_model and ans_model: their records, field checks, filters
and CRCs.  Version 8 changes no record: a frame may hold kinds 0, 1, 2, 3 and 5 in any mix (not 4), and the writer picks a kind
per block from the block's statistics alone:

  H = the block's byte counts, fill = its most frequent byte (lowest on a tie), E = its 64-byte chunks that are all fill.
  Candidate S is what version 5's writer makes (kind 3 when 32 E >= nch, else kind 2, then the raw rule); wS its exact words,
  known from H and E without touching the data.  Candidate A is kind 5: with q the kind-5 quantiser of H and
  cost(q) = 3072 - (bit_length(q ** 256) - 1), i.e. 12 - log2 q in 1/256 bit rounded up,
  wA = 65 * ceil(bl / 32768) + ceil(ceil(sum H[s] cost(q[s]) / 256) / 32).  The block is coded as kind 5 when wA < wS, else as S;
  a block coded as kind 5 still falls under kind 5's raw rule on its actual words.

This file's reader is the reader of a plan with the mode on (versions 1 to 5, 7 and 8); `reads` names what a plan speaks beyond
version 4, so it also models the sparse-only and the rANS-only readers."""
import struct
import zlib

import numpy as np

import ans_model as A
import container_model as M
import sparse_model as S

VERSION = 8
AUTO_KINDS = (M.HUFF, M.RAW, M.HUFF0, S.SPARSE, A.ANS)
# what a version takes: its legal kinds
LEGAL_KINDS = {1: (0, 1), 2: (0, 1), 3: (0, 1, 2), 4: (0, 1, 2), 5: (0, 1, 2, 3), 7: (0, 1, 2, 5), VERSION: AUTO_KINDS}
# what a reading plan must have on to speak a version beyond 4, and what each setting gives
NEEDS = {5: "sparse", 6: "runs", 7: "ans", VERSION: "auto"}
READS_AUTO = frozenset(("sparse", "ans", "auto"))
FORMATS = dict(A.FORMATS)
FORMATS.update(S.FORMATS)
FORMATS.update({(6, 0): ((0,) + M.ELEMS, 4), (6, M.FLAG_DELTA): (M.ELEMS, 4)})
FORMATS.update({(VERSION, 0): ((0,) + M.ELEMS, A.ANS), (VERSION, M.FLAG_DELTA): (M.ELEMS, A.ANS)})
FORMATS.update({(7, 0): ((0,) + M.ELEMS, A.ANS), (7, M.FLAG_DELTA): (M.ELEMS, A.ANS)})

COST_ONE = 256                                                   # cost() counts 1/256 bit


def cost(q):
    """12 - log2 q in 1/256 bit, rounded up, by exact integer arithmetic (1 <= q <= 4096)"""
    assert 1 <= q <= A.TOTAL
    return 12 * COST_ONE - ((q ** 256).bit_length() - 1)


COST = np.asarray([0] + [cost(q) for q in range(1, A.TOTAL + 1)], np.int64)       # (entry 0 is never read: q = 0 only where H = 0)


def stream_format(version, flags, elem):
    elems, max_kind = FORMATS.get((version, flags), ((), M.RAW))
    return M.Format(version, flags, elem, flags == M.FLAG_DELTA, max_kind) if elem in elems else None


def probe(blk):
    """(hist[256], uniform[256]) of one segment: uniform[v] = its 64-byte chunks (the last may be short) made of byte v alone"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8).reshape(-1)
    hist = np.bincount(blk, minlength=256).astype(np.int64)
    uniform = np.zeros(256, np.int64)
    whole = blk.size // S.CHUNK * S.CHUNK
    if whole:
        c = blk[:whole].reshape(-1, S.CHUNK)
        uniform += np.bincount(c[(c == c[:, :1]).all(axis=1), 0], minlength=256)
    if whole < blk.size and bool((blk[whole:] == blk[whole]).all()):
        uniform[int(blk[whole])] += 1
    return hist, uniform


def words_a(hist, bl):
    """wA: the estimate of a kind-5 record's words from the counts alone"""
    hist = np.asarray(hist, np.int64)
    q, _ = A.quantise(hist, bl)
    bits = (int((hist * COST[q]).sum()) + COST_ONE - 1) // COST_ONE
    return 65 * A.nchunks(bl) + (bits + 31) // 32


def candidate_s(blk):
    """(kind, wS) of what version 5's writer makes of the block, from H, fill and the elided bytes: no coding pass"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8).reshape(-1)
    bl, nch, mw = blk.size, S.nchunks(blk.size), S.mask_words(blk.size)
    hist = np.bincount(blk, minlength=256).astype(np.int64)
    fill, mask, K = S.split(blk)
    E = nch - sum(bin(int(w)).count("1") for w in mask)
    if 32 * E >= nch:
        k = hist.copy()
        k[fill] -= bl - K.size                                       # K's counts: only the fill's change, by the elided bytes
        kind, w = S.SPARSE, mw + (M.h0_words(k) if K.size else 0)
    else:
        kind, w = M.HUFF0, M.h0_words(hist)
    return (M.RAW, M.raw_words(bl)) if 4 * w >= bl else (kind, w)


def rule(blk):
    """(what the block is coded as: 5 or "S", wS, wA)"""
    blk = np.ascontiguousarray(blk, dtype=np.uint8).reshape(-1)
    _, ws = candidate_s(blk)
    wa = words_a(np.bincount(blk, minlength=256), blk.size)
    return (A.ANS if wa < ws else "S"), ws, wa


def encode_block(blk, codec):
    """codec 0, 1, 2, 3, 5: that kind under its raw rule; "rule": what the auto writer makes"""
    if codec == "rule":
        codec = rule(blk)[0]
    if codec == A.ANS:
        return A.encode_block5(blk)
    return S.encode_block(blk, "rule" if codec == "S" else codec)


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
    """The version-8 container of `data` as a writer plan of n = block_len, `rows` rows, filter element size `elem`, delta mode
    `delta`, the order-0 codec and the auto mode on makes it.  `kinds` (cycled over the stream's blocks; each 0, 1, 2, 3 or 5)
    forces the codec of each block instead, every one still under its raw rule."""
    elem = 0 if elem == 1 else elem
    fmt = stream_format(VERSION, M.FLAG_DELTA if delta else 0, elem)
    assert fmt is not None
    a = M._u8(data).reshape(-1)
    assert 1 <= block_len <= A.MAX_LEN and rows >= 1
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


def read(buf, with_kinds=False, max_version=VERSION, reads=READS_AUTO):
    """decoded bytes of a container, or ContainerError(what, frame, block).  `reads` is what the reading plan has on ("sparse",
    "ans", "auto"; the auto mode implies the other two): a version beyond 4 that it does not name, and any version beyond
    max_version, is a stream-header failure.  No reader here speaks version 6."""
    buf = bytes(buf)
    L = len(buf)
    if L < 48:
        raise M.ContainerError(M.TRUNCATED)
    h = buf[:32]
    magic, ver, flags, block_len, elem, total = struct.unpack("<4sHHIIQ", h[:24])
    hcrc, z2 = struct.unpack("<II", h[24:])
    fmt = stream_format(ver, flags, elem)
    if (magic != M.MAGIC_STREAM or z2 or hcrc != zlib.crc32(h[:24]) or not 1 <= block_len <= 1 << 20 or fmt is None
            or ver > max_version or ver not in LEGAL_KINDS or (ver in NEEDS and NEEDS[ver] not in reads)):
        raise M.ContainerError(M.STREAM_HEADER)
    legal = LEGAL_KINDS[ver]
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
        nsub, mw = T["nsub"], S.mask_words(bl)
        bad = []
        for b in range(nb):
            kind, lo, hi = int(W[T["kind"] + b]), int(po[b]), int(po[b + 1])
            eo = W[T["enc_off"] + nsub * b: T["enc_off"] + nsub * (b + 1)]
            hist = W[T["hist"] + 256 * b: T["hist"] + 256 * (b + 1)]
            idx = int(W[T["bwt"] + b])
            wrong = kind not in legal or lo > hi or hi > P or (b == 0 and lo != 0) or (b == nb - 1 and hi != P)
            if not wrong and kind == M.RAW:
                wrong = hi - lo != M.raw_words(bl)
            elif not wrong and kind == S.SPARSE:
                wrong = S.check_sparse_fields(idx, eo, hist, pay, lo, hi, bl)
            elif not wrong and kind == A.ANS:
                wrong = A.check_ans_fields(idx, eo, hist, pay, lo, hi, bl)
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
            elif kind == S.SPARSE:
                mask = pay[lo:lo + mw]
                klen = S.klen_of(mask, bl)
                K = M.h0_decode(hist, pay[lo + mw:hi], klen)[0] if klen else np.zeros(0, np.uint8)
                blk = S.join(int(W[T["bwt"] + b]), mask, K, bl)
            elif kind == A.ANS:
                blk = A.decode_record(hist, pay[lo:hi], bl)
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
# the refusal cases of version 8, made from a valid container
# ----------------------------------------------------------------------------------------------------------------------
_HEADER_CASES = ("version ", "kind 3 under a version", "kind 5 under a version", "kind 3 under version 7", "kind 4 under version 7")


def refusal_cases(c8, elem):
    """[(name, container, (what, frame, block))] from the valid version-8 container c8, as the reader of a plan with the mode on
    sees them: the header's own cases, kind 4 and kind 6 under version 8, and every field check of kinds 3 and 5 as sparse_model
    and ans_model make it, with the triple it always had.  c8 needs what those two ask for: a kind-3 block with kept and elided
    chunks that is not the last of its frame, one whose last chunk is short, and a kind-5 block that is not the last of its
    frame."""
    lay = M.layout(c8)
    flags = struct.unpack("<H", c8[6:8])[0]
    none = (M.STREAM_HEADER, -1, -1)
    cases = [("version 9", M.with_header(c8, 9, flags, elem), none),
             ("version 6", M.with_header(c8, 6, flags, elem), none),
             ("version 8 with flags 2", M.with_header(c8, VERSION, 2, elem), none),
             ("version 8 with flags 3", M.with_header(c8, VERSION, 3, elem), none),
             ("version 8 with elem 3", M.with_header(c8, VERSION, flags, 3), none)]
    if flags == 0 and elem == 0:
        cases.append(("version 8, flags 1, elem 0", M.with_header(c8, VERSION, 1, 0), none))
    # under the header of an older version the first block of a kind that version lacks is refused
    first = {}
    for fi, fr in enumerate(lay["frames"]):
        for b, (_, _, kind) in enumerate(fr["records"]):
            first.setdefault(kind, (fi, b))
    for ver, lacks in ((4 if flags else 3, (S.SPARSE, A.ANS)), (5, (A.ANS,)), (7, (S.SPARSE,))):
        at = min(first[k] for k in lacks if k in first)
        cases.append(("under a version-%d header" % ver, M.with_header(c8, ver, flags, elem), (M.FRAME_TABLE,) + at))
    fi, b = first[A.ANS]
    fr = lay["frames"][fi]
    T = M.tables_layout(fr["nb"], fr["blk_len"])

    def poke(kind):
        x = bytearray(c8)
        off = fr["tables"][0] + 4 * (T["kind"] + b)
        x[off:off + 4] = struct.pack("<I", kind)
        return M.retable(bytes(x), fr["start"])

    cases += [("kind 4 under version 8", poke(4), (M.FRAME_TABLE, fi, b)), ("kind 6", poke(6), (M.FRAME_TABLE, fi, b))]
    for model in (S, A):
        for name, cont, want in model.refusal_cases(c8, elem)[0]:
            if not name.startswith(_HEADER_CASES):
                cases.append(("kind %d: %s" % (S.SPARSE if model is S else A.ANS, name), cont, want))
    return cases, lay
