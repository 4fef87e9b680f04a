"""Model of the container's range reads (include/glc_container.h): which blocks of a frame a byte range of
its output needs, written twice.

A frame of nb blocks of bl bytes holds F = nb * bl bytes; [a, b) is the part of a range inside it, in frame-relative bytes.  Without
a filter the needed blocks are those that intersect [a, b).  With a filter of element size e, q = F // e:
    i0 = a // e, rounded down to a multiple of 2048 when the delta flag is set (the delta restarts there)
    i1 = min(q, ceil(b / e))
and the needed blocks are those that intersect one of the filtered byte ranges [j q + i0, j q + i1), 0 <= j < e, plus those of
[q e, F) when b > q e.  One corner is pinned here: a range that lies wholly inside the last F % e bytes (a // e >= q) touches no
element, so it needs no plane run, with or without the delta -- the formula's i0 < i1 is tested before i0 is rounded down.

needed_blocks() is that closed form, the one csrc/container_api.cpp computes.  needed_blocks_brute() finds the same set from the
filter itself: the index of every byte of the frame goes through container_model.filter_frame (the shuffle moves bytes and does
nothing else, so a filtered position knows the original byte it holds), the wanted original bytes are those of the whole elements
the range touches -- widened to the start of the delta's run of 2048 elements -- and the tail, and the blocks are wherever those
bytes ended up."""
import numpy as np

import container_model as M
import sparse_model as S

RUN = M.RUN


def stats_of(frames, offset, count, version, flags, elem):
    """(frames overlapped, needed blocks summed) of a read of [offset, offset + count) over frames [(nb, bl)] in stream order"""
    nf = nblk = 0
    pos, end = 0, offset + count
    for nb, bl in frames:
        lo, hi = max(offset, pos), min(end, pos + nb * bl)
        if count and lo < hi:
            nf += 1
            nblk += len(needed_blocks(version, flags, elem, nb, bl, lo - pos, hi - pos))
        pos += nb * bl
    return nf, nblk


def _blocks(ranges, bl):
    out = set()
    for lo, hi in ranges:
        if lo < hi:
            out.update(range(lo // bl, (hi - 1) // bl + 1))
    return sorted(out)


def needed_blocks(version, flags, elem, nb, bl, a, b):
    """sorted block indices of the frame that bytes [a, b) of it need"""
    fmt = S.stream_format(version, flags, elem)
    assert fmt is not None and 0 <= a <= b <= nb * bl
    if a == b:
        return []
    F = nb * bl
    if not fmt.elem:
        return _blocks([(a, b)], bl)
    e, q = fmt.elem, F // fmt.elem
    i0, i1 = a // e, min(q, -(-b // e))
    ranges = []
    if i0 < i1:
        if fmt.delta:
            i0 -= i0 % RUN
        ranges += [(j * q + i0, j * q + i1) for j in range(e)]
    if b > q * e:
        ranges.append((q * e, F))
    return _blocks(ranges, bl)


def filtered_origin(fmt, F):
    """origin[p] = the index of the original byte of an F-byte frame that filtered byte p holds (or, with the delta, is a
    difference of): the frame's byte indices, a byte of the index at a time, through the filter's byte movement"""
    plain = M.Format(fmt.version, 0, fmt.elem, False, fmt.max_kind)           # (the delta changes values, not places)
    idx = np.arange(F, dtype=np.int64)
    origin = np.zeros(F, dtype=np.int64)
    for k in range(3):
        plane = ((idx >> (8 * k)) & 255).astype(np.uint8)
        origin |= np.asarray(M.filter_frame(plane, plain), dtype=np.int64) << (8 * k)
    assert F < 1 << 24 and np.array_equal(np.sort(origin), idx)
    return origin


def needed_blocks_brute(version, flags, elem, nb, bl, a, b):
    fmt = S.stream_format(version, flags, elem)
    assert fmt is not None and 0 <= a <= b <= nb * bl
    if a == b:
        return []
    F = nb * bl
    origin = filtered_origin(fmt, F)
    wanted = np.zeros(F, dtype=bool)
    if not fmt.elem:
        wanted[a:b] = True
    else:
        e = fmt.elem
        qe = F - F % e
        elems = np.unique(np.arange(a, min(b, qe)) // e)                       # the whole elements the range touches
        if elems.size:
            first = int(elems[0])
            if fmt.delta:
                first -= first % RUN                                           # an element is the sum of its run up to it
            wanted[first * e:(int(elems[-1]) + 1) * e] = True
        if b > qe:
            wanted[qe:F] = True
    return sorted(set((np.nonzero(wanted[origin])[0] // bl).tolist()))
