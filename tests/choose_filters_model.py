"""The CHOOSE codec with filters (INTEGRATION.md 4b "choose with filters", csrc/class_rule.h) in numpy and Python integers: the class
of a block, the frames the writer cuts, the reports, and the writer at every level, built from choose_model, container_model,
auto_model and the filter_*_model writers.  There is no new format and no reader here: what write() makes at level 1 to 5 is format
version 8, 10, 13, 14 or 16, and the model reader of that version reads it (read() below only picks it).

  level  0: choose_model.write (version 3).  1: the order-0 frames take the auto mode.  2 .. 5: and filter-auto, filter-lag,
         filter-grid, filter-byte; the blocks of a super-frame are then sorted into classes and a frame is cut wherever the key changes
  A block of L bytes is
    typed    when L >= MIN_LEN, level >= 2 and the walk over its costs picks a candidate other than (1, 0): filter_auto_model.pick
             over the seven costs, at level 5 an eighth candidate behind them -- the byte predictor at (the block's best lag, stride
             0), its cost that of the histogram of its output (NO_COST below 1024 counted bytes) -- under filter_byte_model's margin
             rule for a byte candidate.  Its element size e is the pick's: 2, 4, 8, or 1 for the byte candidate
    BWT      when it is not typed and choose_model.is_bwt says so
    order-0  otherwise, e = 0
  key = BWT or e.  A BWT run is a version-1 frame of kind-0 / kind-1 records with the frame word 0; an order-0 run is the frame the
  order-0 plan with the level's settings makes of it, its filter picked by that level's rule over the whole run."""
import struct
import zlib

import numpy as np

import auto_model as U
import choose_model as C
import container_model as M
import filter_auto_model as F
import filter_byte_model as B
import filter_grid_model as Q
import filter_lag_model as FL

MAX_LEVEL = 5
BWT = 0xFF                                                        # the key of a BWT block; the others are e = 0, 1, 2, 4, 8
VERSIONS = (3, U.VERSION, F.VERSION, FL.VERSION, Q.VERSION, B.VERSION)
assert VERSIONS == (3, 8, 10, 13, 14, 16)
READS = (frozenset(), frozenset(("sparse", "ans", "auto")), F.READS, FL.READS, Q.READS, B.READS)      # what a plan at the level speaks


def block_costs(blk, level):
    """the costs the class of a block is made from: the seven of the filter probe, at level 5 the byte candidate's behind them"""
    c = F.costs(F.probe(blk))
    if level >= 5:
        x = FL._counted(blk)
        lag = int(np.argmin(np.asarray(B.lag_sums(blk), np.uint64))) + 1
        c.append(F.plane_cost(B.byte_planes(blk, (lag, 0))[0]) if x.size >= B.MIN_LEN else B.NO_COST)
    return c


def typed(level, L, cost):
    """the element size of a typed block, 0 where it is not typed"""
    if level < 2 or L < C.MIN_LEN:
        return 0
    p = F.pick(cost[:7])
    if level >= 5 and ((F.MARGIN_NUM * cost[7] < F.MARGIN_DEN * cost[0]) if p == 0 else cost[7] < cost[p]):
        return 1
    return F.CANDS[p][0] if p else 0


def key_from(level, L, cost, stats):
    """class_key(): the key from a block's length, its costs (eight; the last is read at level 5 alone) and its bigram stats"""
    e = typed(level, L, cost)
    if e:
        return e
    return BWT if C.is_bwt(L, stats) else 0


def key(blk, level):
    blk = M._u8(blk).reshape(-1)
    probed = level >= 2 and blk.size >= C.MIN_LEN                 # (the writer probes no block that cannot be typed)
    return key_from(level if probed else 0, blk.size, block_costs(blk, level) if probed else None, C.stats(blk))


def plan(data, block_len, rows, level):
    """[(pos, nb, bl, key)] of the frames the writer makes: every super-frame cut into its maximal runs of blocks of one key"""
    a = M._u8(data).reshape(-1)
    frames = []
    for pos, nb, bl in C.super_frames(a.size, block_len, rows):
        keys = [key(a[pos + i * bl: pos + (i + 1) * bl], level) for i in range(nb)]
        i = 0
        while i < nb:
            j = i + 1
            while j < nb and keys[j] == keys[i]:
                j += 1
            frames.append((pos + i * bl, j - i, bl, keys[i]))
            i = j
    return frames


def _ops(level):
    """(the rule's pick of a segment, the filter, the frame word, no filter) of the order-0 frames at a level of 2 or more"""
    if level == 2:
        return (lambda seg: F.rule(seg[:F.MAX_LEN])[0], lambda a, p: M.filter_frame(a, F.word_format(F.frame_word(p))), F.frame_word, 0)
    m = {3: FL, 4: Q, 5: B}[level]
    return (lambda seg: m.picked(seg[:F.MAX_LEN]), m.filter_frame, m.frame_word, m.NO_FILTER)


def picks_of(data, block_len, rows, level, frames=None):
    """the filter of every frame, as the level's filter model names it (level 2: an index into filter_auto_model.CANDS; above: a
    candidate tuple); a BWT frame has no filter.  Below level 2: None for every frame"""
    a = M._u8(data).reshape(-1)
    frames = plan(a, block_len, rows, level) if frames is None else frames
    if level < 2:
        return [None] * len(frames)
    picked, _, _, none = _ops(level)
    return [none if k == BWT else picked(a[pos:pos + nb * bl]) for pos, nb, bl, k in frames]


def last_choice(frames):
    """glcContainerLastChoice of plan()'s frames: (blocks to the BWT codec, blocks to the order-0 codec, frames)"""
    return (sum(nb for _, nb, _, k in frames if k == BWT), sum(nb for _, nb, _, k in frames if k != BWT), len(frames))


def reports(picks, level):
    """(glcContainerLastFilters, LastLagFilters, LastGridFilters, LastByteFilters) of a compress with these picks"""
    n = len(picks)
    z4, z3 = (0, 0, 0, 0), (0, 0, 0)
    if level < 2:
        return (n, 0, 0, 0, 0, 0, 0, n), z4, z4, z3
    if level == 2:
        return F.last_filters(picks), z4, z4, z3
    if level == 3:
        return FL.last_filters(picks), FL.last_lag_filters(picks), z4, z3
    if level == 4:
        return Q.last_filters(picks), Q.last_lag_filters(picks), Q.last_grid_filters(picks), z3
    return B.last_filters(picks), B.last_lag_filters(picks), B.last_grid_filters(picks), B.last_byte_filters(picks)


def write(data, block_len, rows, level, with_plan=False, picks=None):
    """the container a writer plan with the CHOOSE codec and glcPlanSetContainerChooseFilters(level) makes of `data`; with_plan:
    (container, plan()'s frames, picks_of()'s picks) for the reports.  `picks` (one per frame, as picks_of() names them) forces the
    frames' filters instead of the level's rule -- the frames are cut by the classes either way"""
    a = M._u8(data).reshape(-1)
    assert 0 <= level <= MAX_LEVEL and 1 <= block_len <= 1 << 20 and rows >= 1
    if level == 0:
        c = C.write(a, block_len, rows)
        fr = [(pos, nb, bl, BWT if k == M.HUFF else 0) for pos, nb, bl, k in C.plan(a, block_len, rows)]
        return (c, fr, [None] * len(fr)) if with_plan else c
    frames = plan(a, block_len, rows, level)
    picks = picks_of(a, block_len, rows, level, frames) if picks is None else [tuple(p) if isinstance(p, (list, tuple)) else p for p in picks]
    assert len(picks) == len(frames)
    hdr24 = M.MAGIC_STREAM + struct.pack("<HHII", VERSIONS[level], 0, block_len, 0) + struct.pack("<Q", a.size)
    out = [hdr24 + struct.pack("<II", zlib.crc32(hdr24), 0)]
    for (pos, nb, bl, k), p in zip(frames, picks):
        seg = a[pos:pos + nb * bl]
        if k == BWT:
            out.append(U._frame([seg[i * bl:(i + 1) * bl] for i in range(nb)], bl, [M.HUFF] * nb))
            continue
        if level == 1:
            out.append(U._frame([seg[i * bl:(i + 1) * bl] for i in range(nb)], bl, ["rule"] * nb))
            continue
        _, filt, word, _ = _ops(level)
        f = filt(seg, p)
        fr = bytearray(U._frame([f[i * bl:(i + 1) * bl] for i in range(nb)], bl, ["rule"] * nb))
        fr[12:16] = struct.pack("<I", word(p))
        out.append(M.retable(bytes(fr), 0))                       # (table_crc covers the word)
    t12 = M.MAGIC_END + struct.pack("<II", len(frames), zlib.crc32(a.tobytes()))
    out.append(t12 + struct.pack("<I", zlib.crc32(t12)))
    c = b"".join(out)
    return (c, frames, picks) if with_plan else c


def read(buf, level):
    """the decoded bytes of a container as the EXISTING model reader of the level's version sees it (none is added here)"""
    if level == 0:
        return M.read(buf, max_version=3)
    if level == 1:
        return U.read(buf)
    return {2: F, 3: FL, 4: Q, 5: B}[level].read(buf)


def order0_write(data, block_len, rows, level):
    """the container of the order-0 plan with the level's settings (auto mode; filter-auto up to the level's step)"""
    if level == 1:
        return U.write(data, block_len, rows)
    return {2: F, 3: FL, 4: Q, 5: B}[level].write(data, block_len, rows)
